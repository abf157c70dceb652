"""Polygon lamps of the emitter guide on the device (pt_set_light_guide_ex, PT_LIGHT_GUIDE_POLYGONS; model:
tests/light_guide_poly_model.py).

1. The hooks pt_light_guide_sample / pt_light_guide_eval against the model, under a moved camera (they stay in world space).
2. Nothing moves by default: pt_set_light_guide, flags = 0 and beta = 0 give the bytes they gave before.
3. The polygon-lamp production kernels against guided pt_trace_paths, bit for bit.
4. The estimator in closed form: a parallel rectangular lamp (the configuration factor) and a triangle (the model's quadrature).
5. cornell with its own lamp: guide on against off.
6. An occluded lamp, pt_set_scene_ex / pt_set_scene while the guide is set, the rest of the library, the CLI.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import env_guide_model as G
from tests import light_guide_model as LG
from tests import light_guide_poly_model as LP
from tests import scene_model as M
from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
F32 = np.float32
W, H = PM.W, PM.H
E32 = np.array(PM.EMISSION, F32)
ENV32 = np.array(PM.ENV, F32)
SUN = G.sun_map()
E1 = (5.0, 4.0, 3.0)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _sph(c, r, material, colour):
    return dict(shape="sphere", material=material, centre=tuple(float(x) for x in c), radius=float(r), colour=tuple(float(x) for x in colour))


def _dsc(c, n, r, material, colour):
    return dict(shape="disc", material=material, centre=tuple(float(x) for x in c), normal=tuple(float(x) for x in n), radius=float(r),
                colour=tuple(float(x) for x in colour))


def _poly(shape, v0, v1, v2, material, colour):
    return dict(shape=shape, material=material, vertices=tuple(tuple(float(x) for x in v) for v in (v0, v1, v2)),
                colour=tuple(float(x) for x in colour))


def _par(v0, v1, v2, material="emissive", colour=E1):
    return _poly("parallelogram", v0, v1, v2, material, colour)


def _tri(v0, v1, v2, material="emissive", colour=E1):
    return _poly("triangle", v0, v1, v2, material, colour)


def _step(P, r, w=W, h=H):
    rec = P.worklist(w, h)
    r.setup(rec)
    r.path_trace()
    return rec, r.read_results(rec)


def _set_ex(P, r, beta, flags):
    g = P.LightGuideEx(12, beta, flags)
    r._check(r._lib.pt_set_light_guide_ex(r.handle, C.byref(g)))


# ---- 1. the hooks against the model

def _f32_error(fn):
    """Largest |f32 - f64| of the same numpy formulas: the figure the project's tolerances are eight times of."""
    a, b = fn(np.float32), fn(np.float64)
    return max(float(np.max(np.abs(x.astype(np.float64) - y))) for x, y in zip(a, b))


def _ring_32():
    """32 emitters on a ring, sphere / disc / triangle / parallelogram in turn, one in five without luminance."""
    out = []
    for k in range(32):
        a = 2 * np.pi * k / 32
        c = np.array([3.0 * np.cos(a), 1.0 + 0.3 * (k % 3), 3.0 * np.sin(a)])
        col = (0.0, 0.0, 0.0) if k % 5 == 4 else (1.0 + k % 4, 2.0, 0.5 + k % 3)
        t = np.array([-np.sin(a), 0.0, np.cos(a)])                       # along the ring
        up = np.array([0.1 * np.cos(a), 1.0, 0.1 * np.sin(a)])
        if k % 4 == 0:
            out.append(_sph(c, 0.1 + 0.02 * (k % 5), "emissive", col))
        elif k % 4 == 1:
            out.append(_dsc(c, (np.cos(a), 0.4, np.sin(a)), 0.25, "emissive", col))
        elif k % 4 == 2:
            out.append(_tri(c - 0.2 * t, c + 0.2 * t, c + 0.35 * up, "emissive", col))
        else:
            out.append(_par(c - 0.15 * t - 0.1 * up, c + 0.15 * t - 0.1 * up, c - 0.15 * t + 0.2 * up, "emissive", col))
    return out


# case -> (objects, origin box (centre, half extent), normal: None = random unit vectors, else fixed)
HOOK_CASES = {
    "rect_face_on": ([_par((-.5, 3, -.5), (.5, 3, -.5), (-.5, 3, .5))], ((0, 0, 0), (.5, .3, .5)), None),
    "tri_grazing": ([_tri((-.9, .4, -3), (.9, .4, -3), (0, .45, -3.9))], ((0, 0, 0), (.5, .1, .5)), None),
    "straddling": ([_par((3, -.5, -.4), (3, .7, -.4), (3, -.5, .4))], ((0, 0, 0), (.5, .05, .5)), (0.0, 1.0, 0.0)),
    "sliver": ([_tri((0, 2, 0), (2, 2.5, 0), (2, 2.5, .01))], ((0, 0, 0), (.5, .3, .5)), None),
    "near": ([_par((-1, .05, -1), (1, .05, -1), (-1, .05, 1))], ((0, 0, 0), (.3, 0, .3)), None),
    "small_far": ([_tri((0, 8, 0), (.1, 8, 0), (0, 8, .1))], ((0, 0, 0), (.5, .3, .5)), None),
    "in_the_polygons_plane": ([_par((-.5, 1, -.5), (.5, 1, -.5), (-.5, 1, .5)), _sph((2.0, 2.0, 0), 0.3, "emissive", E1)],
                              ((0, 1.0, 0), (3.0, 0.0, 3.0)), None),
    "below_the_horizon": ([_tri((-.5, -3, -.5), (.5, -3, -.5), (0, -3, .5))], ((0, 0, 0), (.5, .2, .5)), (0.0, 1.0, 0.0)),
    "zero_luminance": ([_par((1.5, 2, -.5), (2.5, 2, -.5), (1.5, 2, .5), colour=(0, 0, 0)), _tri((-.6, 3, -.5), (.6, 3, -.5), (0, 3.2, .6)),
                        _sph((-2.0, 1.0, 1.0), 0.3, "emissive", (0, 0, 0))], ((0, 0, 0), (.5, .3, .5)), None),
    "mixed_32": (_ring_32(), ((0, 0, 0), (0.8, 0.5, 0.8)), None),
}
ELIGIBILITY_SLACK = 1e-5      # (x, n) this close to a boundary of eligibility, relative to the terms added up, is left out
EDGE_SLACK = 1e-4             # a direction whose smallest barycentric margin is below this is left out
RIM_SLACK_SPHERE, RIM_SLACK_DISC = 2e-6, 2e-5                      # tests/test_gpu_light_guide.py's, for the spheres and discs of mixed_32
NOTHING_DRAWN = ("below_the_horizon",)


def _hook_inputs(case):
    objects, (oc, oh), fixed_n = HOOK_CASES[case]
    stored = LP.stored(objects)
    T = LP.Table(stored, 0.5)
    rng = np.random.default_rng(77)
    n = 1 << 14
    x = (np.asarray(oc) + (rng.random((n, 3)) * 2 - 1) * np.asarray(oh)).astype(F32)
    if fixed_n is None:
        nn = rng.normal(size=(n, 3))
        nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(F32)
    else:
        nn = np.broadcast_to(np.asarray(fixed_n, F32), (n, 3)).copy()
    g1, g2, g3 = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    x64, n64 = x.astype(np.float64), nn.astype(np.float64)
    want_dir, want_rank = LP.sample(T, stored, x64, n64, g1, g2, g3)
    rnd = rng.normal(size=(n, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    w = np.where((want_rank >= 0)[:, None] & (rng.random(n) < 0.7)[:, None], want_dir, rnd).astype(F32)
    # what is left out: a condition on the case, settled on the CPU
    keep = np.ones(n, bool)
    for k in range(T.n_draw):
        o = stored[T.index[k]]
        keep &= LP.eligibility_margin(o, x64, n64) > ELIGIBILITY_SLACK
        keep &= LP.eligible(o, x, nn, np.float32)[0] == LP.eligible(o, x64, n64)[0]   # float32 numpy against float64 numpy alone
    keep_eval = keep.copy()
    w64 = w.astype(np.float64)
    for k in range(T.n_draw):
        o = stored[T.index[k]]
        ok, v, aux = LP.eligible(o, x64, n64)
        if LP.is_polygon(o):
            near = ok & ~(LP.barycentric_margin(o, x64, w64) > EDGE_SLACK)
        else:
            margin = LG.inside_margin(o, x64, v, aux, w64)
            slack = RIM_SLACK_DISC * (o["radius"] ** 2 + np.sum((np.asarray(o["centre"]) - x64) ** 2, axis=1)) if o["shape"] == "disc" else RIM_SLACK_SPHERE
            near = ok & ~(margin > slack)
        g32 = LP.density(o, x, *LP.eligible(o, x, nn, np.float32)[1:], w, np.float32)
        g64 = LP.density(o, x64, v, aux, w64)
        near |= ok & ((g32 > 0) != (g64 > 0))
        keep_eval &= ~near
    return dict(objects=objects, stored=stored, T=T, n=n, x=x, nn=nn, g=(g1, g2, g3), w=w, want_dir=want_dir, want_rank=want_rank,
                keep=keep, keep_eval=keep_eval)


@pytest.mark.parametrize("case", list(HOOK_CASES))
def test_hooks_against_the_model(ptmi_lib, case):
    P = ptmi_lib
    I = _hook_inputs(case)
    T, stored, x, nn, w, keep, keep_eval = I["T"], I["stored"], I["x"], I["nn"], I["w"], I["keep"], I["keep_eval"]
    g1, g2, g3 = I["g"]
    want_dir, want_rank = I["want_dir"], I["want_rank"]
    print("%s: %.3f %% of the inputs left out of sample, %.3f %% of eval (cap 1 %%)" % (case, 100 * (1 - keep.mean()), 100 * (1 - keep_eval.mean())))
    assert keep.mean() >= 0.99 and keep_eval.mean() >= 0.99             # checked before the device is touched
    x64, n64, w64 = x.astype(np.float64), nn.astype(np.float64), w.astype(np.float64)
    r = P.Renderer(16, 16)
    try:
        r.set_scene(I["objects"])
        r.set_light_guide(0.5, polygons=True)
        r.set_camera(**M.MOVED)                                                       # the hooks are in world space whatever the camera
        info = r.light_guide_info()
        flags = r.light_guide_flags()
        got_dir, got_rank = r.light_guide_sample(x, nn, g1, g2, g3)
        got_sum, got_pe = r.light_guide_eval(x, nn, w)
    finally:
        r.close()
    assert flags == P.LIGHT_GUIDE_POLYGONS
    assert info["active"] and info["n_lights"] == T.n and list(info["object_index"]) == T.index
    assert np.array_equal(info["threshold"][:T.n_draw - 1], T.threshold[:T.n_draw - 1]) and np.array_equal(info["probability"], T.p)
    # sample: the rank exactly, the direction within 8 x the float32 error of the same formulas on the same inputs
    assert np.array_equal(got_rank[keep], want_rank[keep])
    assert np.all((got_rank >= -1) & (got_rank < T.n_draw))
    assert not np.any(T.p[got_rank[got_rank >= 0]] == 0)                              # an emitter without luminance is never drawn
    drew = keep & (want_rank >= 0)
    if case in NOTHING_DRAWN:
        assert not drew.any() and np.all(got_rank[keep] == -1) and not np.any(got_dir[keep])
    if case == "in_the_polygons_plane":
        assert not np.any(got_rank[keep] == 0) and np.any(got_rank[keep] == 1)
    if drew.any():
        tol = 8 * _f32_error(lambda t: (LP.sample(T, stored, x[drew].astype(t), nn[drew].astype(t), g1[drew], g2[drew], g3[drew], t)[0],))
        err = float(np.max(np.abs(got_dir[drew] - want_dir[drew])))
        print("%s: direction error %.3g of %.3g allowed, %d drawn" % (case, err, tol, drew.sum()))
        assert 0 < tol < 1e-3 and err <= tol
        assert np.max(np.abs(np.linalg.norm(got_dir[drew].astype(np.float64), axis=1) - 1.0)) < 1e-5
    # eval: P_E exactly (the same binary32 sum in the same order), the sum within the same kind of bound
    want_sum, want_pe = LP.mixture(T, stored, x64, n64, w64)
    pe32 = LP.mixture(T, stored, x, nn, w, dtype=np.float32)[1]
    assert np.array_equal(_bits(got_pe[keep]), _bits(pe32[keep]))
    k = keep_eval
    tol = 8 * _f32_error(lambda t: (LP.mixture(T, stored, x[k].astype(t), nn[k].astype(t), w[k].astype(t), dtype=t)[0],))
    err = float(np.max(np.abs(got_sum[k] - want_sum[k])))
    print("%s: sum error %.3g of %.3g allowed, %d of %d directions inside an emitter" % (case, err, tol, np.count_nonzero(want_sum[k] > 0), k.sum()))
    assert err <= tol
    if case not in NOTHING_DRAWN:
        assert 0 < tol < 1e-3 * max(1.0, float(np.max(want_sum[k]))) and np.count_nonzero(want_sum[k] > 0) > 100


# ---- 2. nothing moves by default

def _renderer(P, objects, camera="none", half=True, env="const", spp=1, ipb=0):
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT, iterations_per_batch=ipb)
    if env == "nif":
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
    else:
        r.set_constant_env(PM.ENV)
    r.init_render_settings(seed=PM.SEED, samples_per_step=spp, aa_noise_scale=PM.AA_SCALE)
    r.set_scene(objects)
    if PM.CAMERAS[camera] is not None:
        r.set_camera(**PM.CAMERAS[camera])
    return r


def _rewind(r, spp=1):
    r.init_render_settings(seed=PM.SEED + 1, samples_per_step=spp, aa_noise_scale=PM.AA_SCALE)
    r.init_render_settings(seed=PM.SEED, samples_per_step=spp, aa_noise_scale=PM.AA_SCALE)


@pytest.mark.parametrize("camera", ["none", "lens_moved"])
def test_nothing_moves_by_default(ptmi_lib, camera):
    """cornell's only emitter is parallelogram 5."""
    P = ptmi_lib
    spp = 3
    r = _renderer(P, PM.world_scene("cornell", camera), camera, spp=spp, ipb=2)
    try:
        def run():
            _rewind(r, spp)
            rec, st = _step(P, r)
            p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 1, np.uint32))
            return rec.tobytes(), p.tobytes(), (st.paths, st.segments, st.escaped)
        plain = run()
        r.set_light_guide(0.5)
        old = run(), r.light_guide_info(), r.light_guide_flags()
        _set_ex(P, r, 0.5, 0)
        ex0 = run(), r.light_guide_info(), r.light_guide_flags()
        _set_ex(P, r, 0.0, P.LIGHT_GUIDE_POLYGONS)
        zero = run(), r.light_guide_info(), r.light_guide_flags()
        r.set_light_guide(0.5, polygons=True)
        on = run(), r.light_guide_info(), r.light_guide_flags()
        with pytest.raises(P.PtError) as e:                               # a rejection keeps the guide and its flags
            _set_ex(P, r, 0.5, 2)
        assert "flags" in str(e.value)
        kept = run(), r.light_guide_info(), r.light_guide_flags()
        r.set_light_guide(None)
        cleared = run(), r.light_guide_flags()
    finally:
        r.close()
    for got in (old, ex0):
        assert got[0] == plain and got[1]["set"] and not got[1]["active"] and got[1]["n_lights"] == 0 and got[2] == 0
    assert zero[0] == plain and zero[1]["active"] and zero[1]["n_lights"] == 1 and zero[2] == 1      # listed, but beta = 0 draws nothing
    assert on[1]["active"] and on[1]["n_lights"] == 1 and list(on[1]["object_index"]) == [5] and on[2] == 1
    assert on[1]["probability"][0] == 1.0
    assert on[0][0] != plain[0] and on[0][1] != plain[1]
    assert kept[0] == on[0] and kept[2] == 1
    assert cleared == (plain, 0)


def test_alpha_plus_beta_is_checked_after_the_flags(ptmi_lib):
    P = ptmi_lib
    r = P.Renderer(16, 16)
    try:
        r.set_constant_env((1, 1, 1))
        r.set_env_guide(SUN, rows=8, cols=16, alpha=0.5)
        for flags, word in ((2, "flags"), (1, "alpha + beta")):
            with pytest.raises(P.PtError) as e:
                _set_ex(P, r, 0.5, flags)
            assert e.value.code == -1 and word in str(e.value)
        _set_ex(P, r, 0.4, 1)
        assert r.light_guide_flags() == 1
    finally:
        r.close()


# ---- 3. the production kernels against guided pt_trace_paths

def _lamps_32(camera):
    """mixed32 with polygon lamps: three more triangles / parallelograms and a sphere of the lattice emit (all with the one
    emission, so that a path's radiance is one multiply), beside the parallelogram lamp it has."""
    objs = PM.world_scene("mixed32", camera)
    turned, sphere = 0, False
    for i, o in enumerate(objs):
        if i < 8 or i == 31:
            continue
        if "vertices" in o and turned < 3 and i % 2 == 0:
            objs[i] = dict(o, material=PM.EMISSIVE, colour=PM.EMISSION)
            turned += 1
        elif "vertices" not in o and not sphere:
            objs[i] = dict(o, material=PM.EMISSIVE, colour=PM.EMISSION)
            sphere = True
    assert turned == 3 and sphere
    return objs


def _scene(name, camera):
    return _lamps_32(camera) if name == "mixed32_lamps" else PM.world_scene(name, camera)


def _radiance(p, env):
    want = np.zeros((len(p), 3), F32)
    if env == "const":
        want[p["escaped"] == 1] = ENV32[None, :] * p["throughput"][p["escaped"] == 1]
    want[p["escaped"] == 2] = E32[None, :] * p["throughput"][p["escaped"] == 2]
    return want


# (scene, camera, half, env, spp, ipb, env guide too): scenes x cameras x sample precisions, the environment alternating; a
# constant case holds the ragged batch split (5 = 2 + 2 + 1), a NIF case one sample per pixel (each value to the NIF's tolerance)
CASES_3 = []
for _i, (_s, _c, _h) in enumerate((s, c, h) for s in ("cornell", "mixed32_lamps") for c in ("none", "moved", "lens_moved") for h in (True, False)):
    _e = "nif" if (_i // 2 + _i) % 3 == 0 else "const"
    CASES_3.append((_s, _c, _h, _e, 1 if _e == "nif" else 5, 0 if _e == "nif" else 2, False))
CASES_3 += [("cornell", "moved", True, "const", 5, 2, True), ("mixed32_lamps", "lens_moved", False, "const", 5, 2, True)]


@pytest.mark.parametrize("scene,camera,half,env,spp,ipb,both", CASES_3,
                         ids=["%s-%s-%s-%s-%dspp%s" % (s, c, "half" if h else "float", e, n, "-both" if b else "") for s, c, h, e, n, _, b in CASES_3])
def test_production_kernels_equal_guided_trace_paths(ptmi_lib, scene, camera, half, env, spp, ipb, both):
    P = ptmi_lib
    r = _renderer(P, _scene(scene, camera), camera, half, env, spp=spp, ipb=ipb)
    try:
        if both:
            r.set_env_guide(SUN, rows=16, cols=32, alpha=0.3)
        r.set_light_guide(0.4 if both else 0.5, polygons=True)
        info = r.light_guide_info()
        rec, st = _step(P, r)
        paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
        bgr = [r.nif_infer(p["uv"][p["escaped"] == 1, 0], p["uv"][p["escaped"] == 1, 1]) for p in paths] if env == "nif" else None
        r.set_light_guide(0.4 if both else 0.5)                          # the default: the polygons leave the table
        default = r.light_guide_info()
        plain = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
    finally:
        r.close()
    if scene == "cornell":
        assert info["n_lights"] == 1 and default["n_lights"] == 0
    else:
        assert info["n_lights"] == 5 and default["n_lights"] == 1
    if spp > 1:
        assert st.trace_launches >= 3
    terms = [_radiance(p, env) for p in paths]
    assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
    assert st.paths == spp * W * H and st.segments == sum(int(p["length"].sum()) for p in paths)
    assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
    got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
    p = paths[0]
    if env == "nif":
        esc, emit, dead = p["escaped"] == 1, p["escaped"] == 2, p["escaped"] == 0
        assert np.array_equal(_bits(got[emit]), _bits(terms[0][emit])) and np.all(_bits(got[dead]) == 0)
        np.testing.assert_allclose(got[esc], bgr[0][:, ::-1] * p["throughput"][esc], rtol=2e-2, atol=1e-6)
    else:
        t = np.stack(terms).astype(np.float64)
        assert np.all(np.abs(got - t.sum(0)) <= 5 * 2.0 ** -24 * np.abs(t).sum(0))   # any order of summation
    on_lamp, on_lamp_plain = np.count_nonzero(p["escaped"] == 2), np.count_nonzero(plain["escaped"] == 2)
    died = (p["escaped"] == 0) & (plain["escaped"] != 0)
    print("paths ending on an emitter: %d with polygon lamps, %d by default; %d died that did not before" % (on_lamp, on_lamp_plain, died.sum()))
    assert on_lamp > on_lamp_plain
    assert np.all(_bits(p["throughput"][p["escaped"] == 0]) == 0) and np.all((p["length"] >= 1) & (p["length"] <= PM.DEPTH))


# ---- 4. the estimator, in closed form

COLOUR = np.array([0.8, 0.5, 0.25])
SKY = 0.02
RECT_LAMP = _par((0.8, 0.4, 2.5), (1.6, 0.4, 2.5), (0.8, 1.0, 2.5), "emissive", (100.0, 100.0, 100.0))   # behind the camera, parallel to the wall
CASES_4 = {"rect_off": (RECT_LAMP, None), "rect_default_inert": (RECT_LAMP, "default"), "rect_b0.5": (RECT_LAMP, 0.5),
           "tri_off": (dict(RECT_LAMP, shape="triangle"), None), "tri_b0.5": (dict(RECT_LAMP, shape="triangle"), 0.5)}


@pytest.mark.parametrize("case", list(CASES_4))
def test_estimator_in_closed_form(ptmi_lib, case):
    """A view-filling diffuse disc at z = -1 that faces the camera, a lamp of radiance E in the plane z = 2.5 behind the camera, a
    dim constant sky: every path is hit -> one bounce -> lamp or sky.  Per pixel E[X] = colour (E F / 2 + L_sky (1 - F) / 2),
    F the configuration factor of the rectangle seen from the hit point: int over the lamp of cos dw / 2 pi = F / 2, and the rest
    of the cosine's integral 1 / 2 goes to the sky.  The triangle (half the rectangle) takes its mean from the model's quadrature.
    Mean within 5, variance within 6 standard errors (those of tests/test_gpu_light_guide.py: the variance of a variance estimate
    from the model's fourth moment).  Model figures (float64), mean / variance: rectangle 0.35639 / 25.564 unguided, 0.12711 at
    beta 0.5; triangle 0.19190 / 13.687 unguided, 0.033577 at beta 0.5."""
    P = ptmi_lib
    lamp, beta = CASES_4[case]
    n_pix, n_samples = 32, 1024
    paths = n_pix * n_pix * n_samples
    wall = _dsc((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 100.0, "diffuse", COLOUR)
    r = P.Renderer(n_pix, n_pix, max_path_length=4, roulette_depth=4, sample_precision=P.SAMPLES_FLOAT)
    try:
        r.set_constant_env((SKY, SKY, SKY))
        r.init_render_settings(seed=3, aa_noise_scale=0.0)
        r.set_scene([wall, lamp])
        if beta == "default":
            r.set_light_guide(0.5)
        elif beta is not None:
            r.set_light_guide(beta, polygons=True)
        vv, uu = np.divmod(np.arange(n_pix * n_pix), n_pix)
        p = r.trace_paths(np.tile(uu, n_samples).astype(np.uint16), np.tile(vv, n_samples).astype(np.uint16),
                          np.repeat(np.arange(n_samples), n_pix * n_pix).astype(np.uint32))
    finally:
        r.close()
    guided = isinstance(beta, float)
    cam = p["cam"][:n_pix * n_pix].astype(np.float64)
    x = np.concatenate([cam, -np.ones((len(cam), 1))], axis=1)                        # the ray (camx, camy, -1) meets z = -1 at t = 1
    c = float(F32(COLOUR[0]))
    mean, var, mu4, want_dead = LP.one_bounce_moments([lamp], x, (0.0, 0.0, 1.0), c, beta if guided else 0.0, sky=SKY, q=64, guided=guided)
    E = 100.0
    if lamp["shape"] == "parallelogram":                                              # the closed form, and the quadrature against it
        v = np.array(lamp["vertices"], np.float64)
        Fm = np.array([LP.rectangle_form_factor(q, v[0], v[1] - v[0], v[2] - v[0], (0.0, 0.0, 1.0)) for q in x])
        closed = float(np.mean(c * (E * Fm / 2 + SKY * (1 - Fm) / 2)))
        assert abs(mean - closed) < 1e-4 * closed
        mean = closed
    if guided:
        unguided_var = LP.one_bounce_moments([lamp], x[::16], (0.0, 0.0, 1.0), c, 0.0, sky=SKY, q=64, guided=False)[1]
        assert var < unguided_var / 5
    esc, emit = p["escaped"] == 1, p["escaped"] == 2
    assert np.all(p["length"][esc | emit] == 2) and np.all(p["length"][~(esc | emit)] == 1)
    X = p["throughput"][:, 0].astype(np.float64) * np.where(emit, E, np.where(esc, SKY, 0.0))
    got_mean, got_var = X.mean(), X.var()
    se_mean, se_var = np.sqrt(var / paths), np.sqrt((mu4 - var * var) / paths)
    print("%s: mean %.5f (expected %.5f, %.2f se)  variance %.5g (model %.5g, %.2f se)  on the lamp %.3f %%" % (
        case, got_mean, mean, (got_mean - mean) / se_mean, got_var, var, (got_var - var) / se_var, 100 * emit.mean()))
    assert abs(got_mean - mean) <= 5 * se_mean
    assert abs(got_var - var) <= 6 * se_var
    assert want_dead == 0.0 and (esc | emit).all()                                    # the lamp is wholly above the wall's horizon
    if guided:
        assert emit.mean() > beta                                                     # every light draw reaches the lamp, and some others


# ---- 5. and 6. films

FW, FH, FSPP, FSTEPS = 64, 48, 64, 12
OCCLUSION = [_dsc((0.0, -1.0, -4.0), (0.0, 1.0, 0.0), 6.0, "diffuse", (0.8, 0.8, 0.8)),          # a floor
             _sph((0.0, 0.0, -4.0), 0.9, "diffuse", (0.7, 0.4, 0.3)),                              # hides the lamp from part of it
             _par((-0.3, 2.6, -4.3), (0.3, 2.6, -4.3), (-0.3, 2.6, -3.7), "emissive", (40.0, 40.0, 40.0))]


def _films(P, scene, beta, env=(0.05, 0.05, 0.05), depth=10):
    """FSTEPS independent step means, [FSTEPS, FH, FW, 3] float64 (B, G, R)."""
    r = P.Renderer(FW, FH, max_path_length=depth)
    try:
        r.set_constant_env(env)
        r.init_render_settings(samples_per_step=FSPP)
        r.set_scene(scene)
        if beta:
            r.set_light_guide(beta, polygons=True)
        out = []
        for _ in range(FSTEPS):
            rec, st = _step(P, r, FW, FH)
            assert np.all(rec["sampleCount"] == FSPP)
            img = np.zeros((FH, FW, 3))
            for k, ch in enumerate("bgr"):
                img[rec["v"], rec["u"], k] = rec[ch].astype(np.float64) / FSPP
            out.append(img)
        return np.array(out)
    finally:
        r.close()


def _agree(films, regions):
    """Per region and channel: |mean on - mean off| in combined standard errors of the FSTEPS step means; the worst."""
    worst = 0.0
    for name, sel in regions.items():
        off = films["off"][:, sel].mean(axis=1)
        on = films["on"][:, sel].mean(axis=1)
        se = np.sqrt(off.var(axis=0, ddof=1) / FSTEPS + on.var(axis=0, ddof=1) / FSTEPS)
        z = (on.mean(axis=0) - off.mean(axis=0)) / se
        print("%s: off %s on %s, difference / combined se %s, variance ratio off / on %s" % (
            name, off.mean(axis=0), on.mean(axis=0), z, off.var(axis=0, ddof=1) / on.var(axis=0, ddof=1)))
        worst = max(worst, float(np.max(np.abs(z))))
    return worst


def test_cornell_films_agree(ptmi_lib):
    """cornell with its own lamp, 12 step means of 64 spp, guide on against off: per channel within 5 combined standard errors."""
    scene = PM.world_scene("cornell", "none")
    films = {"off": _films(ptmi_lib, scene, 0.0, PM.ENV, PM.DEPTH), "on": _films(ptmi_lib, scene, 0.5, PM.ENV, PM.DEPTH)}
    assert _agree(films, {"whole": np.ones((FH, FW), bool)}) <= 5.0
    assert films["on"].tobytes() != films["off"].tobytes()
    pix = films["off"].var(axis=0, ddof=1).mean() / films["on"].var(axis=0, ddof=1).mean()
    print("cornell: per-pixel variance of a 64 spp step mean, off / on = %.3f" % pix)


@pytest.fixture(scope="module")
def occlusion_films(ptmi_lib):
    return {"off": _films(ptmi_lib, OCCLUSION, 0.0), "on": _films(ptmi_lib, OCCLUSION, 0.5)}


def test_occluded_lamp_films_agree(occlusion_films):
    """A rectangular lamp above a sphere that shadows the floor under it: a direction drawn towards the hidden lamp hits the
    occluder and the path goes on."""
    rows, cols = np.arange(FH)[:, None], np.arange(FW)[None, :]
    regions = {"whole": np.ones((FH, FW), bool), "upper": np.broadcast_to(rows < FH // 2, (FH, FW)),
               "lower_left": (rows >= FH // 2) & (cols < FW // 2), "lower_right": (rows >= FH // 2) & (cols >= FW // 2),
               "lower_middle": (rows >= FH // 2) & (np.abs(cols - FW // 2) < FW // 6)}
    assert _agree(occlusion_films, regions) <= 5.0
    assert np.any(occlusion_films["on"] != occlusion_films["off"])


def test_the_guide_follows_the_scene(ptmi_lib):
    P = ptmi_lib
    cornell = PM.world_scene("cornell", "none")
    lamp_sphere = PM.world_scene("cornell", "none", [M._sph((0.05, 0.1, -0.4), 0.02, PM.EMISSIVE, PM.EMISSION)])
    crowd = M.world_scene("crowd", "none")
    r = _renderer(P, cornell, spp=2)
    try:
        def run():
            _rewind(r, 2)
            rec, st = _step(P, r)
            return rec.tobytes(), (st.paths, st.segments, st.escaped)
        r.set_light_guide(0.5, polygons=True)
        a, guided = r.light_guide_info(), run()
        r.set_scene(lamp_sphere)                                          # pt_set_scene_ex: the table follows
        b = r.light_guide_info()
        r.set_scene(crowd)                                                # pt_set_scene, no polygon: the flag survives,
        c, flags_c, crowd_ex = r.light_guide_info(), r.light_guide_flags(), run()
        r.set_light_guide(0.5)                                            # ... and the existing instances run: the same bytes
        crowd_plain = run()
        r.set_light_guide(0.5, polygons=True)
        r.set_scene(cornell)
        d, back = r.light_guide_info(), run()
        r.set_scene(None)
        e, flags_e = r.light_guide_info(), r.light_guide_flags()
    finally:
        r.close()
    T = LP.Table(LP.stored(lamp_sphere), 0.5)
    assert a["active"] and list(a["object_index"]) == [5]
    assert list(b["object_index"]) == [5, 11] == T.index and np.array_equal(b["probability"], T.p) and np.array_equal(b["threshold"][:1], T.threshold[:1])
    assert list(c["object_index"]) == [12, 18, 25] and flags_c == 1 and crowd_ex == crowd_plain
    assert list(d["object_index"]) == [5] and back == guided
    assert e["set"] and not e["active"] and flags_e == 1


def test_sharing_memo_features_and_denoiser_do_not_notice_the_flag(ptmi_lib):
    P = ptmi_lib
    spp = 4
    r = _renderer(P, PM.world_scene("cornell", "moved"), "moved", True, "nif", spp=spp, ipb=2)
    try:
        r.set_light_guide(0.5)
        feat0 = r.feature_buffers()
        noisy = np.random.default_rng(1).random((H, W, 3)).astype(F32)
        den0 = r.denoise(image=noisy)
        r.set_light_guide(0.5, polygons=True)
        feat1 = r.feature_buffers()
        den1 = r.denoise(image=noisy)
        films = {}
        for mode, memo in (("off", 0), ("again", 0), ("step", 0), ("memo", 1 << 20)):
            r.set_nif_sharing("step" if mode == "step" else "off")
            r.set_nif_memo(memo)
            _rewind(r, spp)
            rec, st = _step(P, r)
            films[mode] = (rec.tobytes(), st.paths, st.segments, st.escaped)
        shared = r.nif_sharing_stats()
    finally:
        r.close()
    for k in feat0:
        assert feat0[k].tobytes() == feat1[k].tobytes(), k
    assert den0.tobytes() == den1.tobytes()
    assert films["again"] == films["off"]            # one seed, one result
    assert films["step"] == films["off"] and films["memo"] == films["off"]
    assert shared["evaluations"] <= shared["escaped"]


def test_cli_light_guide_polygons(occlusion_films, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    objs = []
    for o in OCCLUSION:
        q = {k: (list(map(list, v)) if k == "vertices" else list(v) if isinstance(v, tuple) else v) for k, v in o.items()}
        objs.append(q)
    scene = tmp_path / "lamp.json"
    scene.write_text(json.dumps({"objects": objs}))
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    means = {}
    for name, extra in (("off", []), ("default", ["--light-guide-beta", "0.5"]), ("on", ["--light-guide-beta", "0.5", "--light-guide-polygons"])):
        out = tmp_path / (name + ".png")
        r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", "0.05,0.05,0.05", "--scene", str(scene), "-w", str(FW), "-h", str(FH),
                            "-s", str(FSPP * FSTEPS), "--samples-per-step", str(FSPP), "-o", str(out), "--save-interval", str(FSTEPS)]
                           + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert ("light guide: beta 0.5, 1 emitters, polygons included" in r.stdout + r.stderr) == (name == "on")
        film = np.zeros((FH, FW, 3), dtype=np.float32)
        ww, hh = C.c_size_t(), C.c_size_t()
        assert L.pth_read_exr(str(tmp_path / (name + ".exr")).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
        assert (ww.value, hh.value) == (FW, FH)
        means[name] = film.astype(np.float64).reshape(-1, 3).mean(axis=0)
    off = occlusion_films["off"].mean(axis=(1, 2))
    on = occlusion_films["on"].mean(axis=(1, 2))
    se = np.sqrt(off.var(axis=0, ddof=1) / FSTEPS + on.var(axis=0, ddof=1) / FSTEPS)
    print("CLI means off %s on %s, difference / combined se %s" % (means["off"], means["on"], (means["on"] - means["off"]) / se))
    assert np.all(means["default"] == means["off"])                                   # the default skips the polygon: the same film
    assert np.all(np.abs(means["on"] - means["off"]) <= 5 * se)
    assert np.all(means["on"] != means["off"])
