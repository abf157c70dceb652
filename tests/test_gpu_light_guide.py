"""Emitter-guided diffuse sampling on the device (pt_set_light_guide; model: tests/light_guide_model.py).

1. Nothing moves by default: no guide, a guide set then cleared, beta = 0, and a guide on a scene without emitters give the same
   bytes; an environment guide plus beta = 0 equals the environment guide alone.
2. The hooks pt_light_guide_sample / pt_light_guide_eval against the model.
3. The light-guided production kernels against light-guided pt_trace_paths, path for path.
4. The estimator is the one stated: mean and variance of 2^20 one-bounce paths against float64 quadrature.
5. Unbiased where the guide is useless: a furnace, an occluded lamp, multi-bounce films.
6. pt_set_scene while a guide is set.
7. Sharing, the memo, the feature buffers and the denoiser do not notice the guide; one seed, one result.
8. The CLI end to end.

The closed-form case with BOTH guides under a sun map is test_estimator_with_both_guides.
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
from tests import scene_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
F32 = np.float32
W, H = 48, 36
SEED = 11
SUN = G.sun_map()


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _set_env(r, env):
    if env == "nif":
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
    elif env == "map":
        r.set_env_map(SUN, "nearest")
    else:
        r.set_constant_env(M.ENV)


def _renderer(P, scene="builtin", camera="none", half=True, env="map", spp=1, ipb=0, w=W, h=H, depth=M.DEPTH, roulette=M.ROULETTE):
    r = P.Renderer(w, h, max_path_length=depth, roulette_depth=roulette,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT, iterations_per_batch=ipb)
    _set_env(r, env)
    r.init_render_settings(seed=SEED, samples_per_step=spp, aa_noise_scale=M.AA_SCALE)
    if scene != "builtin":
        r.set_scene(M.world_scene(scene, camera))
    if M.CAMERAS[camera] is not None:
        r.set_camera(**M.CAMERAS[camera])
    return r


def _rewind(r, spp=1):
    """The sample cursor back to 0: a new seed resets it."""
    r.init_render_settings(seed=SEED + 1, samples_per_step=spp, aa_noise_scale=M.AA_SCALE)
    r.init_render_settings(seed=SEED, samples_per_step=spp, aa_noise_scale=M.AA_SCALE)


def _step(P, r, w=W, h=H):
    rec = P.worklist(w, h)
    r.setup(rec)
    r.path_trace()
    st = r.read_results(rec)
    return rec, st


def _sph(c, r, material, colour):
    return dict(shape="sphere", material=material, centre=tuple(float(x) for x in c), radius=float(r), colour=tuple(float(x) for x in colour))


def _dsc(c, n, r, material, colour):
    return dict(shape="disc", material=material, centre=tuple(float(x) for x in c), normal=tuple(float(x) for x in n), radius=float(r),
                colour=tuple(float(x) for x in colour))


# ---- 1. nothing moves by default

@pytest.mark.parametrize("scene", ["builtin", "crowd"])
@pytest.mark.parametrize("env", ["nif", "map"])
@pytest.mark.parametrize("camera", ["none", "moved"])
def test_nothing_moves_by_default(ptmi_lib, scene, env, camera):
    P = ptmi_lib
    spp = 3
    r = _renderer(P, scene, camera, True, env, spp=spp, ipb=2)
    try:
        def run():
            _rewind(r, spp)
            rec, st = _step(P, r)
            p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 1, np.uint32))
            return rec.tobytes(), p.tobytes(), (st.paths, st.segments, st.escaped)
        base = run()
        r.set_light_guide(0.5)
        info = r.light_guide_info()
        guided = run()
        r.set_light_guide(None)
        cleared = run()
        r.set_light_guide(0.0)
        zero = run()
        r.set_light_guide(None)
        r.set_env_guide(SUN, rows=8, cols=16, alpha=0.5)
        env_alone = run()
        r.set_light_guide(0.0)
        env_and_zero = run()
    finally:
        r.close()
    assert cleared == base and zero == base
    assert env_and_zero == env_alone and env_alone != base
    assert info["set"]
    if scene == "builtin":                                       # no emitter: accepted, inert, the same bytes
        assert not info["active"] and info["n_lights"] == 0 and guided == base
    else:                                                        # not vacuous: the guide does change the paths
        assert info["active"] and info["n_lights"] == 3
        assert guided[0] != base[0] and guided[1] != base[1]


# ---- 2. the hooks against the model

def _f32_error(fn):
    """Largest |f32 - f64| of the same numpy formulas: the figure the project's tolerances are eight times of."""
    a, b = fn(np.float32), fn(np.float64)
    return max(float(np.max(np.abs(x.astype(np.float64) - y))) for x, y in zip(a, b))


E1 = (5.0, 4.0, 3.0)


def _lamp_ring():
    """32 emitters on a ring, spheres and discs alternating, one in five without luminance."""
    out = []
    for k in range(32):
        a = 2 * np.pi * k / 32
        c = (3.0 * np.cos(a), 1.0 + 0.3 * (k % 3), 3.0 * np.sin(a))
        col = (0.0, 0.0, 0.0) if k % 5 == 4 else (1.0 + k % 4, 2.0, 0.5 + k % 3)
        out.append(_sph(c, 0.1 + 0.02 * (k % 5), "emissive", col) if k % 2 == 0 else
                   _dsc(c, (np.cos(a), 0.4, np.sin(a)), 0.25, "emissive", col))
    return out


# case -> (objects, origin box (centre, half extent), normal: None = random unit vectors, else fixed)
HOOK_CASES = {
    "small_far_sphere": ([_sph((0, 6.0, 0), 0.19, "emissive", E1)], ((0, 0, 0), (0.5, 0.3, 0.5)), None),            # s^2 ~ 1e-3
    "near_sphere": ([_sph((0, 2.0, 0), 1.0, "emissive", E1)], ((0, 0.95, 0), (0.0, 0.0, 0.0)), None),               # D = 1.05 r
    "inside_a_sphere": ([_sph((0, 0, 0), 2.0, "emissive", E1)], ((0, 0, 0), (0.9, 0.9, 0.9)), None),
    "below_the_horizon": ([_sph((0, -3.0, 0), 0.5, "emissive", E1)], ((0, 0, 0), (0.5, 0.2, 0.5)), (0.0, 1.0, 0.0)),
    "straddling_the_horizon": ([_sph((3.0, 0.1, 0), 0.6, "emissive", E1), _dsc((-3.0, 0.1, 0.0), (1.0, 0.1, 0.2), 0.8, "emissive", E1)],
                               ((0, 0, 0), (0.5, 0.05, 0.5)), (0.0, 1.0, 0.0)),
    "disc_face_on": ([_dsc((0, 3.0, 0), (0, -1.0, 0), 0.7, "emissive", E1)], ((0, 0, 0), (0.5, 0.3, 0.5)), None),
    "disc_grazing": ([_dsc((0, 0.4, -3.0), (0, 1.0, 0.05), 0.9, "emissive", E1)], ((0, 0, 0), (0.5, 0.1, 0.5)), None),
    "in_the_discs_plane": ([_dsc((0, 1.0, 0), (0, 1.0, 0), 0.5, "emissive", E1), _sph((2.0, 2.0, 0), 0.3, "emissive", E1)],
                           ((0, 1.0, 0), (3.0, 0.0, 3.0)), None),
    "zero_luminance": ([_sph((2.0, 2.0, 0), 0.4, "emissive", (0, 0, 0)), _dsc((0, 3.0, 0), (0, -1.0, 0.2), 0.7, "emissive", E1),
                        _sph((-2.0, 1.0, 1.0), 0.3, "emissive", (0, 0, 0))], ((0, 0, 0), (0.5, 0.3, 0.5)), None),
    "32_emitters": (_lamp_ring(), ((0, 0, 0), (0.8, 0.5, 0.8)), None),
}
ELIGIBILITY_SLACK = 1e-5      # (x, n) this close to a boundary of eligibility, relative to the terms added up, is left out
RIM_SLACK_SPHERE = 2e-6       # a direction with |w . a - cm| below this is left out (binary32 rounds w . a to ~1e-7)
RIM_SLACK_DISC = 2e-5         # ... or with |R^2 - |p - c|^2| below this x (R^2 + |c - x|^2)


@pytest.mark.parametrize("case", list(HOOK_CASES))
def test_hooks_against_the_model(ptmi_lib, case):
    P = ptmi_lib
    objects, (oc, oh), fixed_n = HOOK_CASES[case]
    stored = LG.stored(objects)
    T = LG.Table(stored, 0.5)
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
    want_dir, want_rank = LG.sample(T, stored, x64, n64, g1, g2, g3)
    # directions to evaluate: those just drawn (inside an emitter, some at its rim) and random ones
    rnd = rng.normal(size=(n, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    w = np.where((want_rank >= 0)[:, None] & (rng.random(n) < 0.7)[:, None], want_dir, rnd).astype(F32)
    r = P.Renderer(16, 16)
    try:
        with pytest.raises(P.PtError) as e:
            r.light_guide_sample(x, nn, g1, g2, g3)
        assert e.value.code == -5                                                     # PT_ERR_NOT_READY without a guide
        r.set_light_guide(0.5)
        with pytest.raises(P.PtError) as e:                                           # ... and with an inert one (the built-in scene)
            r.light_guide_eval(x, nn, w)
        assert e.value.code == -5
        r.set_scene(objects)
        r.set_camera(**M.MOVED)                                                       # the hooks are in world space whatever the camera
        info = r.light_guide_info()
        got_dir, got_rank = r.light_guide_sample(x, nn, g1, g2, g3)
        got_sum, got_pe = r.light_guide_eval(x, nn, w)
        assert r.light_guide_sample(x[:0], nn[:0], g1[:0], g2[:0], g3[:0])[0].shape == (0, 3)   # n == 0 is a no-op
    finally:
        r.close()
    # the table is the model's
    assert info["active"] and info["n_lights"] == T.n and list(info["object_index"]) == T.index
    assert np.array_equal(info["threshold"][:T.n_draw - 1], T.threshold[:T.n_draw - 1]) and np.array_equal(info["probability"], T.p)
    # inputs within rounding of a boundary of eligibility of any emitter are left out: a condition on the case, checked on the CPU
    keep = np.ones(n, bool)
    for k in range(T.n_draw):
        o = stored[T.index[k]]
        keep &= LG.eligibility_margin(o, x64, n64) > ELIGIBILITY_SLACK
        ok32 = LG.eligible(o, x, nn, np.float32)[0]
        keep &= ok32 == LG.eligible(o, x64, n64)[0]                                   # float32 numpy against float64 numpy alone
    keep_eval = keep.copy()
    w64 = w.astype(np.float64)
    for k in range(T.n_draw):
        o = stored[T.index[k]]
        ok, v, aux = LG.eligible(o, x64, n64)
        margin = LG.inside_margin(o, x64, v, aux, w64)
        if o["shape"] == "disc":
            slack = RIM_SLACK_DISC * (o["radius"] ** 2 + np.sum((np.asarray(o["centre"]) - x64) ** 2, axis=1))
        else:
            slack = RIM_SLACK_SPHERE
        near = ok & ~(margin > slack)
        g32 = LG.density(o, x, *LG.eligible(o, x, nn, np.float32)[1:], w, np.float32)
        g64 = LG.density(o, x64, v, aux, w64)
        near |= ok & ((g32 > 0) != (g64 > 0))
        keep_eval &= ~near
    print("%s: %.3f %% of the inputs left out of sample, %.3f %% of eval (cap 1 %%)" % (case, 100 * (1 - keep.mean()), 100 * (1 - keep_eval.mean())))
    assert keep.mean() >= 0.99 and keep_eval.mean() >= 0.99
    # sample: the rank exactly, the direction within 8 x the float32 error of the same formulas on the same inputs
    assert np.array_equal(got_rank[keep], want_rank[keep])
    assert np.all((got_rank >= -1) & (got_rank < T.n_draw))
    assert not np.any(T.p[got_rank[got_rank >= 0]] == 0)                              # an emitter without luminance is never drawn
    drew = keep & (want_rank >= 0)
    if case in ("inside_a_sphere", "below_the_horizon"):
        assert not drew.any() and np.all(got_rank[keep] == -1) and not np.any(got_dir[keep])
    if case == "in_the_discs_plane":
        assert not np.any(got_rank[keep] == 0)
    if drew.any():
        tol = 8 * _f32_error(lambda t: (LG.sample(T, stored, x[drew].astype(t), nn[drew].astype(t), g1[drew], g2[drew], g3[drew], t)[0],))
        err = float(np.max(np.abs(got_dir[drew] - want_dir[drew])))
        print("%s: direction error %.3g of %.3g allowed, %d drawn" % (case, err, tol, drew.sum()))
        assert 0 < tol < 1e-3 and err <= tol
        assert np.max(np.abs(np.linalg.norm(got_dir[drew].astype(np.float64), axis=1) - 1.0)) < 1e-5
    # eval: P_E exactly (the same binary32 sum in the same order), the sum within the same kind of bound
    want_sum, want_pe = LG.mixture(T, stored, x64, n64, w64)
    pe32 = LG.mixture(T, stored, x, nn, w, dtype=np.float32)[1]
    assert np.array_equal(_bits(got_pe[keep]), _bits(pe32[keep]))
    k = keep_eval
    tol = 8 * _f32_error(lambda t: (LG.mixture(T, stored, x[k].astype(t), nn[k].astype(t), w[k].astype(t), dtype=t)[0],))
    err = float(np.max(np.abs(got_sum[k] - want_sum[k])))
    print("%s: sum error %.3g of %.3g allowed, %d of %d directions inside an emitter" % (case, err, tol, np.count_nonzero(want_sum[k] > 0), k.sum()))
    assert err <= tol
    if case not in ("inside_a_sphere", "below_the_horizon"):
        assert tol > 0 and np.count_nonzero(want_sum[k] > 0) > 100


# ---- 3. the light-guided production kernels against light-guided pt_trace_paths

def _emission(scene):
    e = {tuple(o["colour"]) for o in M.SCENES[scene] if o["material"] == M.EMISSIVE}
    return np.array(e.pop() if e else (0, 0, 0), F32)


def _radiance(r, p, emission, env):
    """One binary32 multiply per channel: environment x T (constant or the map's nearest texel), E x T, or nothing."""
    want = np.zeros((len(p), 3), F32)
    esc, emit = p["escaped"] == 1, p["escaped"] == 2
    if env == "map":
        want[esc] = r.env_map_lookup(p["uv"][esc, 0], p["uv"][esc, 1])[:, ::-1] * p["throughput"][esc]     # (the lookup gives B, G, R)
    elif env == "const":
        want[esc] = np.array(M.ENV, F32)[None, :] * p["throughput"][esc]
    want[emit] = emission[None, :] * p["throughput"][emit]
    return want


# (camera, half, env, spp, ipb, env guide too): the whole product of cameras, sample precisions and environments, the constant
# cases with the ragged batch split (5 = 2 + 2 + 1; a NIF case holds one sample per pixel, so that each value is compared to the
# NIF's own tolerance), and one case with both guides under the map, ragged too
CASES_3 = [(c, h, e, 5 if e != "nif" and (i // 3 + i) % 2 == 0 else 1, 2 if e != "nif" and (i // 3 + i) % 2 == 0 else 0, False)
           for i, (c, h, e) in enumerate((c, h, e) for c in ("none", "moved", "lens_moved") for h in (True, False) for e in ("const", "map", "nif"))]
CASES_3.append(("moved", True, "map", 5, 2, True))


@pytest.mark.parametrize("camera,half,env,spp,ipb,both", CASES_3,
                         ids=["%s-%s-%s-%dspp%s" % (c, "half" if h else "float", e, n, "-both" if b else "") for c, h, e, n, _, b in CASES_3])
def test_light_guided_production_kernels_equal_guided_trace_paths(ptmi_lib, camera, half, env, spp, ipb, both):
    P = ptmi_lib
    E = _emission("crowd")
    r = _renderer(P, "crowd", camera, half, env, spp=spp, ipb=ipb)
    try:
        if both:
            r.set_env_guide(SUN, rows=16, cols=32, alpha=0.3)
        r.set_light_guide(0.4 if both else 0.5)
        rec, st = _step(P, r)
        paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
        terms = [_radiance(r, p, E, env) for p in paths]
        bgr = [r.nif_infer(p["uv"][p["escaped"] == 1, 0], p["uv"][p["escaped"] == 1, 1]) for p in paths] if env == "nif" else None
        r.set_light_guide(None)
        r.set_env_guide(None)
        plain = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
    finally:
        r.close()
    if spp > 1:
        assert st.trace_launches >= 3                                                # 5 = 2 + 2 + 1: a ragged last batch
    assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
    assert st.paths == spp * W * H and st.segments == sum(int(p["length"].sum()) for p in paths)
    assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
    got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
    p = paths[0]
    if env == "nif":          # as tests/test_gpu_scene_paths.py: the NIF's value to its own tolerance, everything else to the bit
        esc, emit, dead = p["escaped"] == 1, p["escaped"] == 2, p["escaped"] == 0
        assert np.array_equal(_bits(got[emit]), _bits(terms[0][emit])) and np.all(_bits(got[dead]) == 0)
        np.testing.assert_allclose(got[esc], bgr[0][:, ::-1] * p["throughput"][esc], rtol=2e-2, atol=1e-6)
    elif spp == 1:
        assert np.array_equal(_bits(got), _bits(terms[0]))
    else:
        t = np.stack(terms).astype(np.float64)
        assert np.all(np.abs(got - t.sum(0)) <= 5 * 2.0 ** -24 * np.abs(t).sum(0))   # any order of summation
    # not vacuous: more paths end on an emitter than unguided, and some die at a horizon with the stated length
    on_lamp, on_lamp_plain = np.count_nonzero(p["escaped"] == 2), np.count_nonzero(plain["escaped"] == 2)
    died = (p["escaped"] == 0) & (plain["escaped"] != 0)
    print("paths ending on an emitter: %d guided, %d unguided; %d died that did not before" % (on_lamp, on_lamp_plain, died.sum()))
    assert on_lamp > on_lamp_plain
    assert died.sum() > 0 and np.all(_bits(p["throughput"][p["escaped"] == 0]) == 0)
    assert np.all((p["length"] >= 1) & (p["length"] <= M.DEPTH))
    # the stated length: a path that dies at bounce d has length d + 1, exactly the length of a path whose contribution stack fills
    # at that bounce.  So with max_path_length = L the same paths (same seed, same blocks) must still be dead with length L -- a
    # path recorded one too long would have ended earlier there, one recorded too short would escape, emit or be longer there.
    if env == "const":
        dead = p["escaped"] == 0
        for length in sorted(set(int(x) for x in p["length"][died])):
            if length == M.DEPTH:
                continue
            sel = dead & (p["length"] == length)
            r2 = _renderer(P, "crowd", camera, half, env, spp=spp, ipb=ipb, depth=length)
            try:
                r2.set_light_guide(0.5)
                cut = r2.trace_paths(rec["u"][sel], rec["v"][sel], np.full(int(sel.sum()), st.first_sample, np.uint32))
                full = r2.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
            finally:
                r2.close()
            assert np.all(cut["escaped"] == 0) and np.all(cut["length"] == length), (length, cut["length"], cut["escaped"])
            # ... and the truncated run agrees with the full one on every path that ended before its limit
            early = (p["length"] < length) | ((p["length"] == length) & (p["escaped"] != 0))
            assert np.array_equal(full["length"][early], p["length"][early]) and np.array_equal(full["escaped"][early], p["escaped"][early])


# ---- 4. the estimator, in closed form

COLOUR = np.array([0.8, 0.5, 0.25])
SKY = 0.02
YAW = np.radians(25.0)
LAMP = _sph((1.2, 0.8, 2.5), 0.2, "emissive", (100.0, 100.0, 100.0))                 # behind the camera, above the disc's horizon
DISC_LAMP = _dsc((-1.0, 0.6, 2.0), (0.3, -0.2, -1.0), 0.3, "emissive", (100.0, 100.0, 100.0))
BELOW = _sph((0.5, 0.0, -3.0), 0.2, "emissive", (100.0, 100.0, 100.0))               # behind the diffuse disc: never eligible
STRADDLE = _sph((3.0, 0.0, -0.9), 0.5, "emissive", (30.0, 30.0, 30.0))               # pokes through the disc's plane beside the view
# case -> (lamps in camera space, beta or None, yaw, quadrature points per axis)
CASES_4 = {"unguided": ([LAMP], None, None, 64), "sphere_b0.5": ([LAMP], 0.5, None, 64), "sphere_b0.9": ([LAMP], 0.9, None, 64),
           "disc_b0.5": ([DISC_LAMP], 0.5, None, 64), "two_lamps_one_below": ([BELOW, LAMP], 0.5, None, 64),
           "straddling_b0.5": ([STRADDLE], 0.5, None, 96), "sphere_b0.5_yaw": ([LAMP], 0.5, YAW, 64)}


@pytest.mark.parametrize("case", list(CASES_4))
def test_estimator_in_closed_form(ptmi_lib, case):
    """A view-filling diffuse disc that faces the camera under a dim constant sky, lamps behind the camera: every path is hit ->
    one bounce -> lamp, sky or (a lamp direction below the horizon) nothing.  X = throughput x (emission | sky); mean within 5
    and variance within 6 standard errors of the quadrature's, the errors from the model's own moments, averaged over the
    1024 hit points.  Figures of the model (float64), mean / variance: sphere lamp 0.10649 / 7.2025 unguided, 0.0087521 at
    beta 0.5, 0.00059217 at beta 0.9; disc lamp 0.30432 / 0.088394; two lamps, one below: 0.10649 / 0.028506; the straddling
    lamp 0.028611 / 0.0018182 with 18.7 % of the paths dead."""
    P = ptmi_lib
    lamps, beta, yaw, q = CASES_4[case]
    n_pix, n_samples = 32, 1024
    paths = n_pix * n_pix * n_samples
    f = np.array([0.0, 0.0, -1.0]) if yaw is None else np.array([-np.sin(yaw), 0.0, -np.cos(yaw)])
    rt = np.cross(f, [0.0, 1.0, 0.0])
    rt /= np.linalg.norm(rt)
    up = np.cross(rt, f)
    to_world = lambda c: c[0] * rt + c[1] * up - c[2] * f                             # camera space -> world (position 0)
    wall = _dsc(to_world(np.array([0.0, 0.0, -1.0])), to_world(np.array([0.0, 0.0, 1.0])), 100.0, "diffuse", COLOUR)
    world = [wall]
    for o in lamps:
        w = dict(o, centre=tuple(float(x) for x in to_world(np.asarray(o["centre"]))))
        if o["shape"] == "disc":
            w["normal"] = tuple(float(x) for x in to_world(np.asarray(o["normal"])))
        world.append(w)
    r = P.Renderer(n_pix, n_pix, max_path_length=4, roulette_depth=4, sample_precision=P.SAMPLES_FLOAT)
    try:
        r.set_constant_env((SKY, SKY, SKY))
        r.init_render_settings(seed=3, aa_noise_scale=0.0)
        r.set_scene(world)
        if yaw is not None:
            r.set_camera(position=(0.0, 0.0, 0.0), look_at=tuple(float(x) for x in f.astype(F32)))
        if beta is not None:
            r.set_light_guide(beta)
        vv, uu = np.divmod(np.arange(n_pix * n_pix), n_pix)
        u = np.tile(uu, n_samples).astype(np.uint16)
        v = np.tile(vv, n_samples).astype(np.uint16)
        s = np.repeat(np.arange(n_samples), n_pix * n_pix).astype(np.uint32)
        p = r.trace_paths(u, v, s)
    finally:
        r.close()
    # the hit point of every pixel (no AA noise: one camera ray per pixel), in camera space, float64
    cam = p["cam"][:n_pix * n_pix].astype(np.float64)
    x = np.concatenate([cam, -np.ones((len(cam), 1))], axis=1)                        # the ray (camx, camy, -1) meets z = -1 at t = 1
    mean, var, mu4, want_dead = LG.one_bounce_moments(lamps, x, (0.0, 0.0, 1.0), float(F32(COLOUR[0])), beta or 0.0, sky=SKY, q=q,
                                                      guided=beta is not None)
    if beta is not None:
        unguided_var = LG.one_bounce_moments(lamps, x[::16], (0.0, 0.0, 1.0), float(F32(COLOUR[0])), 0.0, sky=SKY, q=q, guided=False)[1]
        assert var < unguided_var / 5
    esc, emit = p["escaped"] == 1, p["escaped"] == 2
    E = float(lamps[-1]["colour"][0])
    assert np.all(p["length"][esc | emit] == 2) and np.all(p["length"][~(esc | emit)] == 1)
    X = p["throughput"][:, 0].astype(np.float64) * np.where(emit, E, np.where(esc, SKY, 0.0))
    got_mean, got_var = X.mean(), X.var()
    se_mean, se_var = np.sqrt(var / paths), np.sqrt((mu4 - var * var) / paths)
    dead = 1.0 - (esc | emit).mean()
    print("%s: mean %.5f (model %.5f, %.2f se)  variance %.5g (model %.5g, %.2f se)  dead %.4f %% (model %.4f %%)  on a lamp %.3f %%" % (
        case, got_mean, mean, (got_mean - mean) / se_mean, got_var, var, (got_var - var) / se_var, 100 * dead, 100 * want_dead, 100 * emit.mean()))
    assert abs(got_mean - mean) <= 5 * se_mean
    assert abs(got_var - var) <= 6 * se_var
    if case.startswith("straddling"):
        assert want_dead > 0.01
        assert abs(dead - want_dead) <= 5 * np.sqrt(want_dead / paths) + 2e-4         # (quadrature of a step function: 2e-4)
    else:
        assert dead == 0.0 and want_dead == 0.0
    if case == "two_lamps_one_below":                                                  # the fallback arithmetic ran: half the light draws
        assert 0.2 < emit.mean() < 0.35                                               # fall back (p = 1/2 each), so ~ beta / 2 reach the lamp


def test_estimator_with_both_guides(ptmi_lib):
    """The same wall under the 64 x 32 sun map (nearest filter) with a sphere lamp behind the camera, both guides set: alpha 0.3
    on a 32 x 64 grid, beta 0.4.  X = throughput x (emission | the map's texel).  The one statistical check of the combined
    denominator (one_minus + alpha g_env) + beta (...), with one_minus = 1 - (alpha_thr + beta_thr) / 2^32 and both thresholds
    non-zero.  Figures of the model (float64): mean 23.492, variance 772.72 against 72 562 unguided, dead 0.30 %."""
    P = ptmi_lib
    alpha, beta, E = 0.3, 0.4, 4000.0
    n_pix, n_samples = 32, 1024
    paths = n_pix * n_pix * n_samples
    lamp = dict(LAMP, colour=(E, E, E))
    env = G.Guide(SUN, 32, 64, alpha)
    L = SUN[..., 0].astype(np.float64)
    r = P.Renderer(n_pix, n_pix, max_path_length=4, roulette_depth=4, sample_precision=P.SAMPLES_FLOAT)
    try:
        r.set_env_map(SUN, "nearest")
        r.init_render_settings(seed=3, aa_noise_scale=0.0)
        r.set_scene([_dsc((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 100.0, "diffuse", COLOUR), lamp])
        r.set_env_guide(SUN, rows=32, cols=64, alpha=alpha)
        r.set_light_guide(beta)
        vv, uu = np.divmod(np.arange(n_pix * n_pix), n_pix)
        p = r.trace_paths(np.tile(uu, n_samples).astype(np.uint16), np.tile(vv, n_samples).astype(np.uint16),
                          np.repeat(np.arange(n_samples), n_pix * n_pix).astype(np.uint32))
        esc, emit = p["escaped"] == 1, p["escaped"] == 2
        Lq = r.env_map_lookup(p["uv"][esc, 0], p["uv"][esc, 1])[:, 0].astype(np.float64)
    finally:
        r.close()
    cam = p["cam"][:n_pix * n_pix].astype(np.float64)
    x = np.concatenate([cam, -np.ones((len(cam), 1))], axis=1)
    c = float(F32(COLOUR[0]))
    mean, var, mu4, want_dead = LG.both_guides_moments([lamp], x, (0.0, 0.0, 1.0), c, beta, env, L, paths=paths)
    unguided_var = LG.both_guides_moments([lamp], x[::16], (0.0, 0.0, 1.0), c, 0.0, G.Guide(SUN, 32, 64, 0.0), L, paths=paths)[1]
    assert var < unguided_var / 5
    assert np.all(p["length"][esc | emit] == 2) and np.all(p["length"][~(esc | emit)] == 1)
    X = np.zeros(paths)
    X[esc] = p["throughput"][esc, 0].astype(np.float64) * Lq
    X[emit] = p["throughput"][emit, 0].astype(np.float64) * E
    got_mean, got_var = X.mean(), X.var()
    se_mean, se_var = np.sqrt(var / paths), np.sqrt((mu4 - var * var) / paths)
    dead = 1.0 - (esc | emit).mean()
    print("both guides: mean %.4f (model %.4f, %.2f se)  variance %.2f (model %.2f, %.2f se; unguided %.0f)  dead %.4f %% (model %.4f %%)  "
          "on the lamp %.3f %%" % (got_mean, mean, (got_mean - mean) / se_mean, got_var, var, (got_var - var) / se_var, unguided_var,
                                   100 * dead, 100 * want_dead, 100 * emit.mean()))
    assert abs(got_mean - mean) <= 5 * se_mean
    assert abs(got_var - var) <= 6 * se_var
    assert abs(dead - want_dead) <= 5 * np.sqrt(want_dead / paths) + 2e-4             # (quadrature of a step function: 2e-4)
    assert emit.mean() > beta                                                         # every light draw reaches the lamp, and some others


# ---- 5. unbiased where the guide is useless

def test_furnace_with_a_small_emitter(ptmi_lib):
    """One diffuse sphere of colour c under a constant L, plus a small emitter of emission L off to the side, guided at beta 0.5:
    every direction sees radiance L, so the mean over the paths that hit the sphere is c L / 2.  Sigma from the second moment
    of the one-bounce estimator: X = c L cos / den, den >= 1 - beta on the hemisphere, so E[X^2] <= (c L)^2 / (3 (1 - beta))."""
    P = ptmi_lib
    n_samples = 1024
    c, L, beta = np.array([0.8, 0.5, 0.25]), 2.0, 0.5
    centre, radius = np.array([0.0, 0.0, -3.0]), 1.0
    r = P.Renderer(W, H, max_path_length=2, roulette_depth=8, sample_precision=P.SAMPLES_FLOAT)
    try:
        r.set_constant_env((L, L, L))
        r.init_render_settings(seed=5, aa_noise_scale=0.0)
        r.set_scene([_sph(centre, radius, "diffuse", c), _sph((2.5, 1.0, -1.5), 0.3, "emissive", (L, L, L))])
        r.set_light_guide(beta)
        vv, uu = np.divmod(np.arange(W * H), W)
        p = r.trace_paths(np.tile(uu, n_samples), np.tile(vv, n_samples), np.repeat(np.arange(n_samples), W * H))
    finally:
        r.close()
    cam = p["cam"][:W * H].astype(np.float64)
    d = np.concatenate([cam, -np.ones((W * H, 1))], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = d @ centre
    inside = b * b - (centre @ centre - radius * radius) > 0.05                      # well inside the silhouette
    mask = np.tile(inside, n_samples)
    n = int(mask.sum())
    X = np.where((p["escaped"] != 0)[:, None], p["throughput"].astype(np.float64) * L, 0.0)[mask]
    sigma = c * L * np.sqrt((1.0 / (3.0 * (1.0 - beta)) - 0.25) / n)
    mean = X.mean(axis=0)
    print("furnace: %d paths, mean / (c L / 2) = %s, 5 sigma = %s of the mean; %d paths ended on the emitter" % (
        n, mean / (c * L / 2), 5 * sigma / (c * L / 2), np.count_nonzero((p["escaped"] == 2)[mask])))
    assert np.all(5 * sigma < 0.02 * c * L / 2)
    assert np.all(np.abs(mean - c * L / 2) < 5 * sigma), (mean, c * L / 2, sigma)
    assert np.count_nonzero((p["escaped"] == 2)[mask]) > 1000                         # the guide did aim at the emitter


FW, FH, FSPP, FSTEPS = 64, 48, 64, 16
OCCLUSION = [_dsc((0.0, -1.0, -4.0), (0.0, 1.0, 0.0), 6.0, "diffuse", (0.8, 0.8, 0.8)),          # a floor
             _sph((0.0, 0.0, -4.0), 0.9, "diffuse", (0.7, 0.4, 0.3)),                              # hides the lamp from part of it
             _sph((0.0, 2.6, -4.0), 0.35, "emissive", (40.0, 40.0, 40.0))]
CLI_SCENE = {"objects": [dict(o, centre=list(o["centre"]), colour=list(o["colour"]), **({"normal": list(o["normal"])} if "normal" in o else {}))
                         for o in OCCLUSION]}


def _films(P, scene, beta):
    """FSTEPS independent step means, [FSTEPS, FH, FW, 3] float64 (B, G, R)."""
    r = P.Renderer(FW, FH)
    try:
        r.set_constant_env((0.05, 0.05, 0.05))
        r.init_render_settings(samples_per_step=FSPP)
        r.set_scene(scene)
        if beta:
            r.set_light_guide(beta)
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


@pytest.fixture(scope="module")
def occlusion_films(ptmi_lib):
    return {"off": _films(ptmi_lib, OCCLUSION, 0.0), "on": _films(ptmi_lib, OCCLUSION, 0.5)}


def _agree(films, regions):
    """Per region and channel: |mean on - mean off| <= 5 combined standard errors of the FSTEPS step means."""
    worst = 0.0
    for name, sel in regions.items():
        off = films["off"][:, sel].mean(axis=1)                                       # [FSTEPS, 3]
        on = films["on"][:, sel].mean(axis=1)
        se = np.sqrt(off.var(axis=0, ddof=1) / FSTEPS + on.var(axis=0, ddof=1) / FSTEPS)
        z = (on.mean(axis=0) - off.mean(axis=0)) / se
        print("%s: off %s on %s, difference / combined se %s, variance ratio off / on %s" % (
            name, off.mean(axis=0), on.mean(axis=0), z, off.var(axis=0, ddof=1) / on.var(axis=0, ddof=1)))
        worst = max(worst, float(np.max(np.abs(z))))
    return worst


def test_occluded_lamp_films_agree(occlusion_films):
    """A lamp above a sphere that shadows the floor under it: a direction drawn towards the hidden lamp hits the occluder and
    the path goes on.  Regions: the image's quarters (the floor's shadow lies in the lower ones) and the whole."""
    rows, cols = np.arange(FH)[:, None], np.arange(FW)[None, :]
    regions = {"whole": np.ones((FH, FW), bool), "upper": np.broadcast_to(rows < FH // 2, (FH, FW)),
               "lower_left": (rows >= FH // 2) & (cols < FW // 2), "lower_right": (rows >= FH // 2) & (cols >= FW // 2),
               "lower_middle": (rows >= FH // 2) & (np.abs(cols - FW // 2) < FW // 6)}
    assert _agree(occlusion_films, regions) <= 5.0
    assert np.any(occlusion_films["on"] != occlusion_films["off"])


def test_multi_bounce_crowd_films_agree(ptmi_lib):
    films = {"off": _films(ptmi_lib, M.world_scene("crowd", "none"), 0.0), "on": _films(ptmi_lib, M.world_scene("crowd", "none"), 0.5)}
    assert _agree(films, {"whole": np.ones((FH, FW), bool)}) <= 5.0
    assert np.any(films["on"] != films["off"])


# ---- 6. pt_set_scene while a guide is set

def test_the_guide_follows_the_scene(ptmi_lib):
    P = ptmi_lib
    crowd = M.world_scene("crowd", "none")
    no_lamps = [dict(o, material=M.DIFFUSE) if o["material"] == M.EMISSIVE else o for o in crowd]
    r = _renderer(P, "crowd", "none", True, "const", spp=2)
    try:
        def run():
            _rewind(r, 2)
            rec, st = _step(P, r)
            return rec.tobytes(), (st.paths, st.segments, st.escaped)
        r.set_scene(no_lamps)
        inert_want = run()
        r.set_scene(crowd)
        r.set_light_guide(0.5)
        a = r.light_guide_info()
        guided = run()
        again = run()
        r.set_scene(no_lamps)
        b = r.light_guide_info()
        inert = run()
        r.set_camera(**M.MOVED)
        r.set_scene(M.world_scene("crowd", "moved"))
        c = r.light_guide_info()
        r.set_camera()
        r.set_scene(crowd)
        back = run()
        r.set_scene(None)
        d = r.light_guide_info()
    finally:
        r.close()
    T = LG.Table(crowd, 0.5)
    assert a["active"] and list(a["object_index"]) == [12, 18, 25] == T.index and np.array_equal(a["probability"], T.p)
    assert np.array_equal(a["threshold"][:2], T.threshold[:2]) and a["beta"] == 0.5
    assert b["set"] and not b["active"] and b["n_lights"] == 0
    assert c["active"] and np.array_equal(c["probability"], a["probability"])          # a rigid transform does not change the table
    assert d["set"] and not d["active"]                                                 # the built-in scene
    assert again == guided and back == guided                                           # one seed, one result
    assert inert == inert_want and guided != inert


# ---- 7. independence of the rest

def test_sharing_memo_features_and_denoiser_do_not_notice_the_guide(ptmi_lib):
    P = ptmi_lib
    spp = 4
    r = _renderer(P, "crowd", "moved", True, "nif", spp=spp, ipb=2)
    try:
        feat0 = r.feature_buffers()
        noisy = np.random.default_rng(1).random((H, W, 3)).astype(F32)
        den0 = r.denoise(image=noisy)
        r.set_light_guide(0.5)
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


# ---- 8. the CLI end to end

def test_cli_light_guide(occlusion_films, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    scene = tmp_path / "lamp.json"
    scene.write_text(json.dumps(CLI_SCENE))
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    means = {}
    for name, extra in (("off", []), ("on", ["--light-guide-beta", "0.5"])):
        out = tmp_path / (name + ".png")
        r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", "0.05,0.05,0.05", "--scene", str(scene), "-w", str(FW), "-h", str(FH),
                            "-s", str(FSPP * FSTEPS), "--samples-per-step", str(FSPP), "-o", str(out), "--save-interval", str(FSTEPS)]
                           + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert ("light guide: beta 0.5, 1 emitters" in r.stdout + r.stderr) == (name == "on")
        film = np.zeros((FH, FW, 3), dtype=np.float32)
        ww, hh = C.c_size_t(), C.c_size_t()
        assert L.pth_read_exr(str(tmp_path / (name + ".exr")).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
        assert (ww.value, hh.value) == (FW, FH)
        means[name] = film.astype(np.float64).reshape(-1, 3).mean(axis=0)
    off = occlusion_films["off"].mean(axis=(1, 2))
    on = occlusion_films["on"].mean(axis=(1, 2))
    se = np.sqrt(off.var(axis=0, ddof=1) / FSTEPS + on.var(axis=0, ddof=1) / FSTEPS)
    print("CLI means off %s on %s, difference / combined se %s" % (means["off"], means["on"], (means["on"] - means["off"]) / se))
    assert np.all(np.abs(means["on"] - means["off"]) <= 5 * se)
    assert np.all(means["on"] != means["off"])
