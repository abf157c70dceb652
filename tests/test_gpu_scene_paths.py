"""Runtime scenes, poses and the lens, path for path (cases: tests/scene_model.py).

A. The production three-phase kernels (primary phase from the host-made per-object constants, two-ended survivor list, first
   shading from the packed halves, emitters that end in the primary phase, the dynamic-LDS hit table at 1 and at 32 rows) against
   pt_trace_paths on the same handle: the same device functions, so every pixel's length and radiance agree bit for bit.
B. pt_trace_paths against the float64 model, which traces in world space where the kernels trace in camera space, at the
   CPU-calibrated tolerance 2 R (spread + 2e-6 scale) on the paths the model finds well conditioned.
"""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import scene_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
ENV32 = np.array(M.ENV, F32)
_ID = ["%s-%s-%s" % (s, c, "half" if h else "float") for s, c, h in M.CASES_A]


def _renderer(P, scene, camera, half, spp=1, ipb=0, env=True):
    r = P.Renderer(M.W, M.H, max_path_length=M.DEPTH, roulette_depth=M.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT, iterations_per_batch=ipb)
    if env:
        r.set_constant_env(M.ENV)
    else:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
    r.init_render_settings(seed=M.SEED, samples_per_step=spp, aa_noise_scale=M.AA_SCALE)
    r.set_scene(M.world_scene(scene, camera))
    if M.CAMERAS[camera] is not None:
        r.set_camera(**M.CAMERAS[camera])
    return r


def _emission(scene):
    e = {tuple(o["colour"]) for o in M.SCENES[scene] if o["material"] == M.EMISSIVE}
    assert len(e) <= 1
    return np.array(e.pop() if e else (0, 0, 0), F32)


def _radiance(p, emission, env=ENV32):
    """One binary32 multiply per channel, as emit_escaped / shade_hit: env x T, E x T, or nothing."""
    want = np.zeros((len(p), 3), F32)
    for code, col in ((1, env), (2, emission)):
        m = p["escaped"] == code
        want[m] = col[None, :] * p["throughput"][m]
    return want


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("scene,camera,half", M.CASES_A, ids=_ID)
def test_production_kernels_equal_trace_paths(ptmi_lib, scene, camera, half):
    P = ptmi_lib
    E = _emission(scene)
    r = _renderer(P, scene, camera, half)
    try:
        seen, longest = set(), 0
        for step in range(3):
            rec = P.worklist(M.W, M.H)
            r.setup(rec)
            r.path_trace()
            st = r.read_results(rec)
            assert st.first_sample == step
            p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
            assert np.array_equal(rec["pathLength"], p["length"])
            got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
            assert np.array_equal(_bits(got), _bits(_radiance(p, E)))
            assert np.all(rec["sampleCount"] == 1)
            assert st.paths == M.W * M.H and st.segments == int(p["length"].sum())
            assert st.escaped == np.count_nonzero(p["escaped"] == 1)
            seen |= set(np.unique(p["escaped"]).tolist())
            longest = max(longest, int(p["length"].max()))
    finally:
        r.close()
    outcomes, length = M.EXPECT[scene]
    # not vacuous: what this scene can show, it shows (binary32 adds the odd outcome the model has not: a grazing bounce off a
    # lone sphere that meets the sphere again)
    assert outcomes <= seen and longest >= length
    assert scene != "inside" or 1 not in seen               # nothing leaves the emitting shell
    if scene == "crowd":
        first = M.case_b(scene, camera, dict((c[:2], c[2]) for c in M.CASES_B)[(scene, camera)])[4]["hits"][:len(rec), 0]
        hit = set(np.unique(first).tolist()) - {-1}
        assert len(hit) >= 20 and {0, 31} <= hit


def test_several_samples_per_step_with_a_ragged_last_batch(ptmi_lib):
    P = ptmi_lib
    scene, camera, spp = "crowd", "lens_moved", 5
    E = _emission(scene)
    r = _renderer(P, scene, camera, True, spp=spp, ipb=2)
    try:
        rec = P.worklist(M.W, M.H)
        r.setup(rec)
        r.path_trace()
        st = r.read_results(rec)
        paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
    finally:
        r.close()
    assert st.trace_launches >= 3                           # 5 = 2 + 2 + 1
    assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
    assert st.paths == spp * M.W * M.H and st.segments == sum(int(p["length"].sum()) for p in paths)
    assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
    terms = np.stack([_radiance(p, E).astype(np.float64) for p in paths])
    got = np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64)
    assert np.all(np.abs(got - terms.sum(0)) <= 5 * 2.0 ** -24 * np.abs(terms).sum(0))      # any order of summation


@pytest.mark.parametrize("camera", ["none", "moved"])
def test_nif_environment(ptmi_lib, camera):
    P = ptmi_lib
    scene = "crowd"
    E = _emission(scene)
    r = _renderer(P, scene, camera, True, env=False)
    try:
        rec = P.worklist(M.W, M.H)
        r.setup(rec)
        r.path_trace()
        st = r.read_results(rec)
        p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
        esc = p["escaped"] == 1
        bgr = r.nif_infer(p["uv"][esc, 0], p["uv"][esc, 1])
    finally:
        r.close()
    assert np.array_equal(rec["pathLength"], p["length"]) and st.escaped == esc.sum() and esc.sum() > 1000
    got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
    emitted, dead = p["escaped"] == 2, p["escaped"] == 0
    assert emitted.sum() > 50 and dead.sum() > 50
    assert np.array_equal(_bits(got[emitted]), _bits(_radiance(p, E)[emitted]))
    assert np.all(_bits(got[dead]) == 0)
    np.testing.assert_allclose(got[esc], bgr[:, ::-1] * p["throughput"][esc], rtol=2e-2, atol=1e-6)     # (nif_infer gives B, G, R)


@pytest.mark.parametrize("scene,camera,half", M.CASES_B, ids=["%s-%s-%s" % (s, c, "half" if h else "float") for s, c, h in M.CASES_B])
def test_trace_paths_against_the_float64_model(oracle, ptmi_lib, scene, camera, half):
    P = ptmi_lib
    uu, vv, ss, cam, plain, fragile, spread = M.case_b(scene, camera, half)
    r = _renderer(P, scene, camera, half)
    try:
        stored = r.scene()
        p = r.trace_paths(uu, vv, ss)
    finally:
        r.close()
    # the model ran on the CPU's copy of the inputs: the table as the library stores it and the camera rays it forms are those
    assert stored.tobytes() == M.stored_scene(M.world_scene(scene, camera)).tobytes()
    assert np.array_equal(p["cam"], cam)
    same, ratio = M.compare(p, plain, fragile, spread)
    ok = ~fragile
    print("%s / %s / %s: fragile %.2f %%, largest ratio %.3f of %.3f allowed; mismatching outcomes %d" % (
        scene, camera, "half" if half else "float", 100 * fragile.mean(), ratio, M.GPU_FACTOR,
        np.count_nonzero((p["length"] != plain["length"])[ok] | (p["escaped"] != plain["escaped"])[ok])))
    assert fragile.mean() <= M.FRAGILE_CAP
    assert same
    assert ratio <= M.GPU_FACTOR
