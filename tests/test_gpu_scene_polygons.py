"""Triangles and parallelograms in runtime scenes (pt_set_scene_ex) on the GPU (cases: tests/scene_poly_model.py).

A. The production three-phase kernels' polygon instances against pt_trace_paths on the same handle, bit for bit.
B. pt_trace_paths against the float64 model at the project's rule 2 R (spread + 2e-6 scale), R = 0.68 (tests/scene_model.py).
C. Closed forms: a diffuse, a mirror and an emissive parallelogram that fill the view, and the triangle that is half of one.
D. A table of spheres and discs through pt_set_scene_ex is pt_set_scene's scene; a rejected table keeps the scene in force.
E. Feature buffers and the denoiser.   F. The two guides.   G. NIF sharing and the memo.   H. The CLI.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import features_model as FM
from tests import scene_model as M
from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
F32 = np.float32
ENV32 = np.array(PM.ENV, F32)
E32 = np.array(PM.EMISSION, F32)
L_SKY = (0.75, 1.5, 3.0)        # few mantissa bits: L x 1 is exact
W, H = PM.W, PM.H


def _ids(cases):
    return ["%s-%s-%s" % (s, c, "half" if h else "float") for s, c, h in cases]


def _nif(r):
    r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())


def _renderer(P, scene, camera, half, spp=1, ipb=0, env=True, extra=()):
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT, iterations_per_batch=ipb)
    if env:
        r.set_constant_env(PM.ENV)
    else:
        _nif(r)
    r.init_render_settings(seed=PM.SEED, samples_per_step=spp, aa_noise_scale=PM.AA_SCALE)
    r.set_scene(PM.world_scene(scene, camera, extra))
    if PM.CAMERAS[camera] is not None:
        r.set_camera(**PM.CAMERAS[camera])
    return r


def _radiance(p, emission=E32, env=ENV32):
    """One binary32 multiply per channel, as emit_escaped / shade_hit: env x T, E x T, or nothing."""
    want = np.zeros((len(p), 3), F32)
    for code, col in ((1, env), (2, emission)):
        m = p["escaped"] == code
        want[m] = col[None, :] * p["throughput"][m]
    return want


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _step(P, r):
    rec = P.worklist(W, H)
    r.setup(rec)
    r.path_trace()
    return rec, r.read_results(rec)


# ---- A

@pytest.mark.parametrize("scene,camera,half", PM.CASES_A, ids=_ids(PM.CASES_A))
def test_production_kernels_equal_trace_paths(ptmi_lib, scene, camera, half):
    P = ptmi_lib
    r = _renderer(P, scene, camera, half)
    try:
        assert P.has_polygon(r.scene_ex())
        seen = set()
        for step in range(3):
            rec, st = _step(P, r)
            assert st.first_sample == step
            p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
            assert np.array_equal(rec["pathLength"], p["length"])
            got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
            assert np.array_equal(_bits(got), _bits(_radiance(p)))
            assert np.all(rec["sampleCount"] == 1)
            assert st.paths == W * H and st.segments == int(p["length"].sum())
            assert st.escaped == np.count_nonzero(p["escaped"] == 1)
            seen |= set(np.unique(p["escaped"]).tolist())
    finally:
        r.close()
    # not vacuous: a lone polygon is hit and missed; the two large scenes show every outcome
    big = scene in ("cornell", "mixed32")
    assert seen >= ({0, 1, 2} if big else {1})
    assert p["length"].max() >= (4 if big else 2) and (big or p["length"].min() == 1)


@pytest.mark.parametrize("scene,camera", [("cornell", "lens_moved"), ("mixed32", "moved")])
def test_three_steps_with_a_ragged_last_batch(ptmi_lib, scene, camera):
    P = ptmi_lib
    spp = 5
    r = _renderer(P, scene, camera, True, spp=spp, ipb=2)
    try:
        for step in range(3):
            rec, st = _step(P, r)
            assert st.first_sample == step * spp and st.trace_launches >= 3          # 5 = 2 + 2 + 1
            paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
            assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
            assert st.paths == spp * W * H and st.segments == sum(int(p["length"].sum()) for p in paths)
            assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
            terms = np.stack([_radiance(p).astype(np.float64) for p in paths])
            got = np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64)
            assert np.all(np.abs(got - terms.sum(0)) <= 5 * 2.0 ** -24 * np.abs(terms).sum(0))      # any order of summation
    finally:
        r.close()


@pytest.mark.parametrize("scene,camera", [("cornell", "none"), ("cornell", "moved"), ("mixed32", "lens_moved")])
def test_nif_environment(ptmi_lib, scene, camera):
    P = ptmi_lib
    r = _renderer(P, scene, camera, True, env=False)
    try:
        rec, st = _step(P, r)
        p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
        esc = p["escaped"] == 1
        bgr = r.nif_infer(p["uv"][esc, 0], p["uv"][esc, 1])
    finally:
        r.close()
    assert np.array_equal(rec["pathLength"], p["length"]) and st.escaped == esc.sum() and esc.sum() > 300
    got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
    emitted, dead = p["escaped"] == 2, p["escaped"] == 0
    assert emitted.sum() > 30 and dead.sum() > 30
    assert np.array_equal(_bits(got[emitted]), _bits(_radiance(p)[emitted]))
    assert np.all(_bits(got[dead]) == 0)
    np.testing.assert_allclose(got[esc], bgr[:, ::-1] * p["throughput"][esc], rtol=2e-2, atol=1e-6)     # (nif_infer gives B, G, R)


# ---- B

@pytest.mark.parametrize("scene,camera,half", PM.CASES_B, ids=_ids(PM.CASES_B))
def test_trace_paths_against_the_float64_model(oracle, ptmi_lib, scene, camera, half):
    """Largest ratio measured on an MI355X over the twelve cases: see profiles/r20_polygons.txt."""
    P = ptmi_lib
    uu, vv, ss, cam, plain, fragile, spread = PM.case_b(scene, camera, half)
    r = _renderer(P, scene, camera, half)
    try:
        stored = r.scene_ex()
        p = r.trace_paths(uu, vv, ss)
    finally:
        r.close()
    # the model ran on the CPU's copy of the inputs: the table as the library stores it and the camera rays it forms are those
    assert stored.tobytes() == PM.stored_scene_ex(PM.world_scene(scene, camera)).tobytes()
    assert np.array_equal(p["cam"], cam)
    same, ratio = PM.compare(p, plain, fragile, spread)
    ok = ~fragile
    print("%s / %s / %s: fragile %.2f %%, largest ratio %.3f of %.3f allowed; mismatching outcomes %d" % (
        scene, camera, "half" if half else "float", 100 * fragile.mean(), ratio, M.GPU_FACTOR,
        np.count_nonzero((p["length"] != plain["length"])[ok] | (p["escaped"] != plain["escaped"])[ok])))
    assert fragile.mean() <= M.FRAGILE_CAP
    assert same
    assert ratio <= M.GPU_FACTOR


# ---- C

def _par(v0, v1, v2, material, colour=(1, 1, 1)):
    return {"shape": "parallelogram", "material": material, "vertices": (v0, v1, v2), "colour": colour}


A_, B_, C_ = (-2.0, -2.0, -1.0), (2.0, -2.0, -1.0), (-2.0, 2.0, -1.0)      # the plane z = -1 over x, y in [-2, 2]: it fills the view
FRONT, BEHIND = (A_, B_, C_), (A_, C_, B_)                                  # the normal towards the camera (+z), and away from it


def _render(P, scene, const, spp, depth=8, roulette=8, precision=None, steps=1):
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette,
                   sample_precision=P.SAMPLES_FLOAT if precision is None else precision, iterations_per_batch=4)
    try:
        r.set_constant_env(const)
        r.init_render_settings(seed=5, samples_per_step=spp)
        r.set_scene(scene)
        rec = P.worklist(W, H)
        r.setup(rec)
        stats = []
        for _ in range(steps):
            r.path_trace()
            stats.append(r.read_results(rec).as_dict())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)[0].copy()
        return rec, film, stats
    finally:
        r.close()


@pytest.mark.parametrize("roulette", [8, 1])
@pytest.mark.parametrize("side", ["front", "behind"])
def test_furnace_on_a_parallelogram(ptmi_lib, roulette, side):
    """A diffuse parallelogram of colour c that fills the view under a constant L: E[cos theta] = 1/2 over the hemisphere and every
    bounce leaves the plane, so the mean is c L / 2 (the variance formula of test_gpu_scene.py::test_furnace)."""
    P = ptmi_lib
    spp = 20                                                   # 64 x 48 x 20 = 61440 samples: the statistic asks for >= 50000
    c, L = np.array([0.8, 0.5, 0.25]), 2.0
    verts = FRONT if side == "front" else BEHIND
    rec, film, st = _render(P, [_par(*verts, "diffuse", tuple(c))], (L, L, L), spp, roulette=roulette)
    n = W * H * spp
    assert n >= 50000 and st[0]["paths"] == n
    mean = film.astype(np.float64).mean(axis=0)[::-1]          # RGB
    stop = float(np.float16(0.3))
    second = 1.0 / 3.0 / (1.0 - stop) if roulette == 1 else 1.0 / 3.0
    sigma = c * L * np.sqrt((second - 0.25) / n)
    print("furnace %s, roulette %d: mean / (c L / 2) = %s, 5 sigma = %s of it" % (side, roulette, mean / (c * L / 2), 5 * sigma / (c * L / 2)))
    assert np.all(np.abs(mean - c * L / 2) < 5 * sigma), (mean, c * L / 2, sigma)
    if roulette == 1:
        assert st[0]["escaped"] < st[0]["paths"]               # roulette really stopped some paths
    else:
        assert st[0]["escaped"] == st[0]["paths"] and np.all(rec["pathLength"] == 2 * spp)


@pytest.mark.parametrize("verts", [FRONT, BEHIND], ids=["front", "behind"])
def test_mirror_and_emitter_in_closed_form(ptmi_lib, verts):
    P = ptmi_lib
    spp = 8
    sky = np.float32([L_SKY[2], L_SKY[1], L_SKY[0]])           # BGR
    rec, film, st = _render(P, [_par(*verts, "specular")], L_SKY, spp, depth=6, roulette=6)
    assert np.all(film == sky)
    assert np.all(rec["pathLength"] == 2 * spp)                # one bounce, then the sky
    assert st[0]["escaped"] == st[0]["paths"] == W * H * spp and st[0]["segments"] == 2 * st[0]["paths"]
    E = (0.5, 1.0, 2.0)
    rec, film, st = _render(P, [_par(*verts, "emissive", E)], L_SKY, spp, depth=6, roulette=6)
    assert np.all(film == np.float32(E[::-1]))
    assert np.all(rec["pathLength"] == spp) and st[0]["escaped"] == 0 and st[0]["segments"] == st[0]["paths"]
    # the triangle that is half of it: a + b <= 1 is x + y <= 0 on the plane z = -1
    tri = {"shape": "triangle", "material": "emissive", "vertices": verts, "colour": E}
    rec, film, st = _render(P, [tri], L_SKY, spp, depth=6, roulette=6)
    x = (2.0 * (rec["u"] + 0.5) - W) / W
    y = -((2.0 * (rec["v"] + 0.5) - H) / H) * (H / W)
    margin = 4 * 2.0 / W                                       # four pixels along the diagonal: the AA noise has sigma 0.3 of one
    inside, outside = x + y < -margin, x + y > margin
    assert inside.sum() > 1000 and outside.sum() > 1000
    assert np.all(film[inside] == np.float32(E[::-1])) and np.all(film[outside] == sky)
    assert np.all(rec["pathLength"] == spp)                    # length 1 either way
    assert 0 < st[0]["escaped"] < st[0]["paths"]


# ---- D

def _everything(P, setter, camera="lens_moved"):
    """Records, film, stats and pt_trace_paths bytes of two steps of `crowd` (spheres and discs), the scene given by `setter`."""
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE, iterations_per_batch=2)
    try:
        _nif(r)
        r.init_render_settings(seed=PM.SEED, samples_per_step=4)
        setter(r)
        if camera:
            r.set_camera(**M.CAMERAS[camera])
        rec = P.worklist(W, H)
        r.setup(rec)
        stats = []
        for _ in range(2):
            r.path_trace()
            s = r.read_results(rec).as_dict()
            stats.append((s["paths"], s["segments"], s["escaped"], s["trace_launches"]))
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)[0].copy()
        paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 3, np.uint32))
        feat = r.feature_buffers()
        return rec.tobytes(), film.tobytes(), stats, paths.tobytes(), b"".join(feat[k].tobytes() for k in sorted(feat))
    finally:
        r.close()


def test_spheres_and_discs_through_set_scene_ex_are_the_same_scene(ptmi_lib):
    P = ptmi_lib
    objs = M.world_scene("crowd", "lens_moved")
    plain = P.scene_array(objs)
    wide = P.scene_array_ex(plain)
    assert wide.dtype == P.SCENE_EX_DTYPE and not P.has_polygon(wide)
    wide["vertex"] = 7.5                                       # a sphere's or disc's vertices are ignored
    old = _everything(P, lambda r: r.set_scene(plain))
    new = _everything(P, lambda r: r.set_scene(wide))          # an ex array goes through pt_set_scene_ex
    assert old == new
    # the built-in table through it equals no call
    none = _everything(P, lambda r: None, camera=None)
    builtin = _everything(P, lambda r: r.set_scene(P.builtin_scene_ex()), camera=None)
    assert none == builtin and none != old


def test_rejection_keeps_the_scene_and_get_scene_points_to_get_scene_ex(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    r = P.Renderer(32, 32)
    try:
        r.set_scene(PM.world_scene("cornell", "none"))
        before = r.scene_ex()
        assert len(before) == 11 and list(before["shape"][:6]) == [3] * 6 and list(before["shape"][-2:]) == [2, 2]
        assert np.array_equal(before["centre"][before["shape"] >= 2], before["vertex"][before["shape"] >= 2, 0])
        assert not before["vertex"][before["shape"] < 2].any() and np.all(before["radius"][before["shape"] >= 2] == 0)
        bad = PM.world_scene("cornell", "none")
        bad[9] = dict(bad[9], vertices=((0, 0, -1), (1, 1, -2), (2, 2, -3)))
        with pytest.raises(P.PtError) as e:
            r.set_scene(bad)
        assert e.value.code == -1 and "scene object 9: vertices are collinear" in str(e.value)
        assert r.scene_ex().tobytes() == before.tobytes()
        # pt_set_scene keeps refusing the new shapes, and the scene stays
        narrow = np.zeros(1, P.SCENE_DTYPE)
        narrow[0]["shape"], narrow[0]["radius"], narrow[0]["colour"] = 2, 1, 1
        assert lib.pt_set_scene(r.handle, narrow.ctypes.data, 1) == -1
        assert "shape must be 0 (sphere) or 1 (disc) (got 2)" in lib.pt_last_error(r.handle).decode()
        assert r.scene_ex().tobytes() == before.tobytes()
        # pt_get_scene: the count, but no copy
        n = C.c_uint32()
        assert lib.pt_get_scene(r.handle, None, 0, C.byref(n)) == 0 and n.value == 11
        with pytest.raises(P.PtError) as e:
            r.scene()
        assert "use pt_get_scene_ex" in str(e.value)
        # a table of spheres and discs, or the built-in scene, and pt_get_scene copies again
        r.set_scene(P.scene_array_ex(P.builtin_scene()))
        assert r.scene().tobytes() == P.builtin_scene().tobytes()
        r.set_scene(PM.world_scene("triangle", "none"))
        assert lib.pt_set_scene_ex(r.handle, None, 0, 84) == 0
        assert r.scene().tobytes() == P.builtin_scene().tobytes() and r.scene_ex().tobytes() == P.builtin_scene_ex().tobytes()
    finally:
        r.close()


# ---- E

def test_feature_buffers_and_the_denoiser_on_cornell(oracle, ptmi_lib):
    P = ptmi_lib
    camera = "moved"
    r = _renderer(P, "cornell", camera, True, spp=8)
    try:
        r.init_render_settings(seed=PM.SEED, samples_per_step=8, aa_noise_scale=PM.AA_SCALE, fov_degrees=FM.FOV_DEGREES)
        f = r.feature_buffers()
        stored = r.scene_ex()
        rec, st = _step(P, r)
        r.film_accumulate()
        film = np.zeros((H, W, 3), F32)
        film[rec["v"], rec["u"]] = r.gather_hdr(W * H, P.HDR_FILM)[0]
        out = r.denoise(source="film", demodulate=0)
    finally:
        r.close()
    ids, depth, nrm, good = PM.first_hit(stored, PM.CAMERAS[camera], FM.camera_rays(W, H))
    ids, depth, nrm, good = ids.reshape(H, W), depth.reshape(H, W), nrm.reshape(H, W, 3), good.reshape(H, W)
    # away from silhouettes and edges: every pixel of the 3 x 3 block around it shows the same object in the model
    core = np.zeros((H, W), bool)
    core[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            core[1:-1, 1:-1] &= ids[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] == ids[1:-1, 1:-1]
    assert core.mean() > 0.6 and set(np.unique(ids[core]).tolist()) >= set(range(10))      # (the model's own figures: 0.74, all but the last)
    assert np.array_equal(f["object_id"][core], ids[core])
    cmp_ = core & good & (ids >= 0)
    assert cmp_.sum() > 2000
    assert np.max(np.abs(f["depth"][cmp_] - depth[cmp_]) / depth[cmp_]) <= FM.DEPTH_TOL
    assert np.max(np.abs(f["normal"][cmp_] - nrm[cmp_])) <= FM.NORMAL_TOL
    poly = cmp_ & (stored["shape"][np.maximum(ids, 0)] >= 2)
    assert poly.sum() > 1000                                   # mostly walls
    # albedo: the material rule (B, G, R)
    for k in (0, 3, 5, 6, 7, 9):                               # floor, left wall, lamp (emissive), mirror, glass, a wedge triangle
        sel = core & (ids == k)
        assert sel.any()
        want = stored[k]["colour"][::-1] if stored[k]["material"] in (0, 2) else np.ones(3, F32)
        assert np.all(f["albedo"][sel] == want), k
    # the denoiser needs nothing: it runs, and without demodulation every output lies within the range of its inputs
    assert out.shape == film.shape and np.isfinite(out).all() and not np.array_equal(out, film)
    slack = 1e-5 * film.max()
    assert np.all(out >= film.min(axis=(0, 1)) - slack) and np.all(out <= film.max(axis=(0, 1)) + slack)


# ---- F

def _bytes_of_steps(P, r, steps=2):
    out = []
    for _ in range(steps):
        rec, st = _step(P, r)
        out.append((rec.tobytes(), st.paths, st.segments, st.escaped))
    return out


LAMP = [M._sph((0.05, 0.1, -0.3), 0.03, PM.EMISSIVE, (30.0, 30.0, 30.0))]      # a small sphere lamp inside the box (camera space)


@pytest.mark.parametrize("camera", ["none", "lens_moved"])
def test_guides_at_zero_give_the_unguided_bits(ptmi_lib, camera):
    P = ptmi_lib
    sun = np.full((16, 32, 3), 0.1, F32)
    sun[3, 5] = 50.0
    runs = {}
    for name in ("off", "env0", "light0", "plain", "light_inert"):
        r = _renderer(P, "cornell", camera, True, spp=4, ipb=2, extra=() if name in ("plain", "light_inert") else LAMP)
        try:
            if name == "env0":
                r.set_env_guide(sun, rows=8, cols=16, alpha=0.0)
            elif name in ("light0", "light_inert"):
                r.set_light_guide(0.0 if name == "light0" else 0.5)
                info = r.light_guide_info()
                if name == "light0":
                    # the emissive parallelogram (object 5) is skipped: the table lists the sphere lamp alone
                    assert info["n_lights"] == 1 and list(info["object_index"]) == [11] and info["active"]
                else:
                    assert info["n_lights"] == 0 and not info["active"]        # cornell's only emitter is a polygon: inert
            runs[name] = _bytes_of_steps(P, r)
        finally:
            r.close()
    assert runs["env0"] == runs["off"] and runs["light0"] == runs["off"]
    assert runs["light_inert"] == runs["plain"] and runs["plain"] != runs["off"]


def test_light_guide_agrees_with_the_unguided_mean(ptmi_lib):
    """cornell with the sphere lamp, beta 0.5 against no guide: the image means agree within 5 combined standard errors of the
    step means, and the guided production kernels are pt_trace_paths' guided twin bit for bit."""
    P = ptmi_lib
    steps, spp = 12, 16
    films = {}
    for beta in (0.0, 0.5):
        r = _renderer(P, "cornell", "none", False, spp=spp, extra=LAMP)
        try:
            if beta:
                r.set_light_guide(beta)
                assert r.light_guide_info()["n_lights"] == 1
            means = []
            for _ in range(steps):
                rec, st = _step(P, r)
                means.append(np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64).mean(axis=0) / spp)
            films[beta] = np.array(means)
            if beta:      # ... and the guided production kernels are pt_trace_paths' guided twin: lengths and escapes bit for bit
                r.init_render_settings(seed=PM.SEED + 1, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
                rec, st = _step(P, r)
                p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
                assert np.array_equal(rec["pathLength"], p["length"]) and st.escaped == np.count_nonzero(p["escaped"] == 1)
                esc = p["escaped"] == 1
                got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
                assert np.array_equal(_bits(got[esc]), _bits(_radiance(p)[esc])) and np.count_nonzero(p["escaped"] == 2) > 30
        finally:
            r.close()
    off, on = films[0.0], films[0.5]
    se = np.sqrt(off.var(axis=0, ddof=1) / steps + on.var(axis=0, ddof=1) / steps)
    z = (on.mean(axis=0) - off.mean(axis=0)) / se
    print("light guide on cornell: off %s on %s, difference / combined se %s, variance ratio off / on %s" % (
        off.mean(axis=0), on.mean(axis=0), z, off.var(axis=0, ddof=1) / on.var(axis=0, ddof=1)))
    assert np.all(np.abs(z) <= 5.0) and not np.array_equal(off, on)


# ---- G

def test_nif_sharing_and_the_memo_are_bit_identical_to_off(ptmi_lib):
    P = ptmi_lib
    films = {}
    for name in ("off", "batch", "step", "memo"):
        r = _renderer(P, "cornell", "moved", True, spp=6, ipb=2, env=False)
        try:
            r.set_nif_sharing("off" if name == "memo" else name)
            if name == "memo":
                r.set_nif_memo(1 << 26)
            rec = P.worklist(W, H)
            r.setup(rec)
            stats = []
            for _ in range(3):
                r.path_trace()
                s = r.read_results(rec)
                stats.append((s.paths, s.segments, s.escaped))
                r.film_accumulate()
            films[name] = (r.gather_hdr(W * H, P.HDR_FILM)[0].tobytes(), rec.tobytes(), stats)
        finally:
            r.close()
    assert films["off"][2][0][2] > 500                         # paths do reach the NIF through the open front
    assert films["off"] == films["batch"] == films["step"] == films["memo"]


# ---- H

def _read_exr(path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=np.float32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert L.pth_read_exr(str(path).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    return film


def test_cli_renders_a_polygon_scene_file(ptmi_lib, tmp_path):
    P = ptmi_lib
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    spp = 8
    objects = []
    for o in PM.world_scene("cornell", "none"):
        o = dict(o)
        o["shape"] = {0: "sphere", 1: "disc", 2: "triangle", 3: "parallelogram"}[o["shape"]]
        o["material"] = {0: "diffuse", 1: "specular", 2: "refractive", 3: "emissive"}[o["material"]]
        for k in ("centre", "colour", "normal"):
            if k in o:
                o[k] = [float(x) for x in o[k]]
        if "vertices" in o:
            o["vertices"] = [[float(x) for x in q] for q in o["vertices"]]
        objects.append(o)
    camera = {"position": [0.05, 0.02, 0.15], "look_at": [0.0, -0.02, -0.3], "up": [0.05, 1, 0]}
    path = tmp_path / "cornell.json"
    path.write_text(json.dumps({"objects": objects, "camera": camera}))
    base = [exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in L_SKY), "-w", str(W), "-h", str(H),
            "-s", str(spp), "--samples-per-step", str(spp), "--max-path-length", "7", "-o", str(tmp_path / "box.png"),
            "--save-interval", "1"]
    r = subprocess.run(base + ["--scene", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    exr = _read_exr(tmp_path / "box.exr")
    lib_r = P.Renderer(W, H, max_path_length=7, roulette_depth=3, iterations_per_batch=2)
    try:
        lib_r.set_constant_env(L_SKY)
        lib_r.init_render_settings(seed=1, samples_per_step=spp)
        lib_r.set_scene(objects)
        lib_r.set_camera(**camera)
        rec = P.worklist(W, H)
        lib_r.setup(rec)
        lib_r.path_trace()
        lib_r.read_results(rec)
        lib_r.film_accumulate()
        image = np.zeros((H, W, 3), F32)
        image[rec["v"], rec["u"]] = lib_r.gather_hdr(W * H, P.HDR_FILM)[0]
    finally:
        lib_r.close()
    assert np.array_equal(exr, image) and len(np.unique(image.reshape(-1, 3), axis=0)) > 1000
    # collinear vertices: refused with the library's message and a non-zero exit
    objects[10]["vertices"] = [[0, 0, -1], [1, 1, -2], [2, 2, -3]]
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"objects": objects}))
    r = subprocess.run(base + ["--scene", str(bad)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "scene object 10: vertices are collinear" in r.stdout
