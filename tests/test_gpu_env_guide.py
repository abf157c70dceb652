"""Environment-guided diffuse sampling on the device (pt_set_env_guide; model: tests/env_guide_model.py).

1. Nothing moves by default: no guide, a guide set then cleared, and a guide with alpha = 0 give the same bytes.
2. The hooks pt_env_guide_sample / pt_env_guide_eval against the model.
3. The guided production kernels against guided pt_trace_paths, path for path.
4. The estimator is the one stated: sample mean and variance of 2^20 one-bounce paths against float64 quadrature.
5. Unbiased with the "wrong" guide: the furnace test guided by a sun map.
6. Multi-bounce agreement of guided and unguided films.
7. Sharing, the memo, the feature buffers and the denoiser do not notice the guide; one seed, one result.
8. The CLI end to end.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import env_guide_model as G
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
        r.set_env_guide(SUN, rows=8, cols=16, alpha=0.5)
        guided = run()
        r.set_env_guide(None)
        cleared = run()
        r.set_env_guide(SUN, alpha=0.0)          # the guided instances, multiplying by 1 / (1 - 0 + 0 g)
        zero = run()
    finally:
        r.close()
    assert cleared == base
    assert zero == base
    assert guided[0] != base[0] and guided[1] != base[1]          # not vacuous: the guide does change the paths


# ---- 2. the hooks against the model

def _f32_error(fn):
    """Largest |f32 - f64| of the same numpy formulas: the figure the project's tolerances are eight times of."""
    a, b = fn(np.float32), fn(np.float64)
    return max(float(np.max(np.abs(x.astype(np.float64) - y))) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["sun_32x64", "procedural_default", "sun_1x1"])
def test_hooks_against_the_model(ptmi_lib, case):
    P = ptmi_lib
    img, rows, cols = {"sun_32x64": (SUN, 32, 64), "procedural_default": (G.procedural_sun_map(), 256, 512), "sun_1x1": (SUN, 1, 1)}[case]
    az_deg = 40.0
    az = P.rotation_to_radians_f32(az_deg)
    model = G.Guide(img, rows, cols, 0.5)
    rng = np.random.default_rng(2024)
    n = 1 << 16
    g1, g2, g3 = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    r = P.Renderer(16, 16)
    try:
        with pytest.raises(P.PtError) as e:
            r.env_guide_sample(g1, g2, g3)
        assert e.value.code == -5                                                     # PT_ERR_NOT_READY without a guide
        r.init_render_settings(seed=1, env_rotation_degrees=az_deg)
        r.set_env_guide(img, rows=rows, cols=cols, alpha=0.5)
        uv, cell = r.env_guide_sample(g1, g2, g3)
        want_cell = G.sample_cell(model, g1, g2)
        u64, v64 = G.sample_uv(model, want_cell, g3)
        d32 = G.direction(u64, v64, az).astype(F32)
        ecell, eg = r.env_guide_eval(d32)
        r.set_env_guide(None)
        with pytest.raises(P.PtError) as e:
            r.env_guide_eval(d32)
        assert e.value.code == -5
    finally:
        r.close()
    # sample: the cell exactly, (u, v) within 8 x the float32 error of the same formulas on these inputs
    assert np.array_equal(cell, want_cell)
    tol_uv = 8 * _f32_error(lambda t: G.sample_uv(model, want_cell, g3, t))
    print("%s: (u, v) error %.3g of %.3g allowed" % (case, max(np.max(np.abs(uv[:, 0] - u64)), np.max(np.abs(uv[:, 1] - v64))), tol_uv))
    assert tol_uv < 1e-5                                  # (0 where the grid is small enough for binary32 to hold (u, v) exactly)
    assert np.max(np.abs(uv[:, 0] - u64)) <= tol_uv and np.max(np.abs(uv[:, 1] - v64)) <= tol_uv
    # eval: the sampled cell, but for directions whose (u, v) lies within the bound of a cell border (or which the rounding of
    # the direction to binary32 has itself carried into the neighbouring cell): at most 1 % of the inputs
    tol_dir = 8 * _f32_error(lambda t: G.dir_to_uv(d32.astype(t), az, t))
    ub, vb = G.dir_to_uv(d32.astype(np.float64), az)
    du, dv = G.border_distance(model, ub, vb)
    keep = (G.cell_of(model, ub, vb) == want_cell)
    if rows > 1:
        keep &= du > tol_dir
    if cols > 1:
        keep &= dv > tol_dir
    print("%s: %.3f %% of the directions left out (bound %.3g)" % (case, 100 * (1 - keep.mean()), tol_dir))
    assert keep.mean() >= 0.99
    assert np.array_equal(ecell[keep], want_cell[keep])
    assert np.all(ecell < model.n)
    # g within the same kind of bound: relative, and in units of its conditioning -- 1 - y^2 is formed in binary32, so the error
    # of g grows as 1 / sin^2(theta) towards the poles; the constant of that law is what float32 numpy shows on these inputs
    y = d32[:, 1].astype(np.float64)
    cond = 1.0 / np.maximum(1.0 - y * y, 1e-300)
    g32 = G.density(model, d32, az, np.float32)[1].astype(np.float64)
    g64 = G.density(model, d32.astype(np.float64), az)[1]
    k32 = float(np.max(np.abs(g32[keep] - g64[keep]) / g64[keep] / cond[keep]))
    kdev = float(np.max(np.abs(eg[keep] - g64[keep]) / g64[keep] / cond[keep]))
    print("%s: g relative error x sin^2(theta) %.3g of %.3g allowed" % (case, kdev, 8 * k32))
    assert 0 < k32 < 1e-6 and kdev <= 8 * k32


# ---- 3. the guided production kernels against guided pt_trace_paths

def _emission(scene):
    if scene == "builtin":
        return np.zeros(3, F32)
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


CASES_3 = [("builtin", "none", True, "map", 1, 0), ("builtin", "moved", False, "map", 1, 0), ("builtin", "lens", False, "const", 1, 0),
           ("crowd", "none", False, "map", 1, 0), ("crowd", "lens_moved", True, "map", 5, 2), ("crowd", "moved", True, "nif", 1, 0)]


@pytest.mark.parametrize("scene,camera,half,env,spp,ipb", CASES_3,
                         ids=["%s-%s-%s-%s-%dspp" % (s, c, "half" if h else "float", e, n) for s, c, h, e, n, _ in CASES_3])
def test_guided_production_kernels_equal_guided_trace_paths(ptmi_lib, scene, camera, half, env, spp, ipb):
    P = ptmi_lib
    E = _emission(scene)
    r = _renderer(P, scene, camera, half, env, spp=spp, ipb=ipb)
    try:
        r.set_env_guide(SUN, rows=16, cols=32, alpha=0.5)
        rec, st = _step(P, r)
        paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
        terms = [_radiance(r, p, E, env) for p in paths]
        bgr = [r.nif_infer(p["uv"][p["escaped"] == 1, 0], p["uv"][p["escaped"] == 1, 1]) for p in paths] if env == "nif" else None
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
    # not vacuous: the guide changes many paths, some point below the surface and end there, with the stated length
    changed = (p["length"] != plain["length"]) | np.any(_bits(p["throughput"]) != _bits(plain["throughput"]), axis=-1)
    assert changed.mean() > 0.05
    died = (p["escaped"] == 0) & (plain["escaped"] != 0)
    assert died.sum() > 5 and np.all(_bits(p["throughput"][p["escaped"] == 0]) == 0)
    assert np.all((p["length"] >= 1) & (p["length"] <= M.DEPTH))


# ---- 4. the estimator, in closed form

COLOUR = np.array([0.8, 0.5, 0.25])
YAW = np.radians(25.0)
CASES_4 = {"unguided": (None, 0.0, None), "a0.5_32x64": ((32, 64, 0.5), 0.0, None), "a0.5_8x16": ((8, 16, 0.5), 0.0, None),
           "a0.9_32x64": ((32, 64, 0.9), 0.0, None), "a0.5_32x64_azimuth_yaw": ((32, 64, 0.5), 40.0, YAW)}


@pytest.fixture(scope="module")
def unguided_variance():
    return G.one_bounce_moments(None, SUN[..., 0].astype(np.float64), (0.0, 0.0, 1.0))[1]


@pytest.mark.parametrize("case", list(CASES_4))
def test_estimator_in_closed_form(ptmi_lib, unguided_variance, case):
    """A view-filling diffuse disc that faces the camera under the 64 x 32 sun map: every path is hit -> one bounce -> escape.
    X = throughput x L(uv); mean within 5 and variance within 6 standard errors of the quadrature's, the errors from the
    predicted moments.  Float64 figures of the model: mean 24.549; variances 96 788 (unguided), 607.3, 17 092, 73.5."""
    P = ptmi_lib
    spec, az_deg, yaw = CASES_4[case]
    n_pix, n_samples = 32, 1024
    paths = n_pix * n_pix * n_samples
    if yaw is None:
        f = np.array([0.0, 0.0, -1.0])
    else:
        f = np.array([-np.sin(yaw), 0.0, -np.cos(yaw)])
    f32 = f.astype(F32)
    az = P.rotation_to_radians_f32(az_deg)
    normal = -f32.astype(np.float64) / np.linalg.norm(f32.astype(np.float64))
    model = G.Guide(SUN, *spec) if spec else None
    L = SUN[..., 0].astype(np.float64)
    mean, var, mu4 = G.one_bounce_moments(model, L, normal, azimuth=az, paths=paths)
    if spec:
        assert var < unguided_variance / 5
    r = P.Renderer(n_pix, n_pix, max_path_length=4, roulette_depth=4, sample_precision=P.SAMPLES_FLOAT)
    try:
        r.set_env_map(SUN, "nearest")
        r.init_render_settings(seed=3, env_rotation_degrees=az_deg)
        r.set_scene([dict(shape="disc", material="diffuse", centre=tuple(float(x) for x in f32), radius=100.0,
                          normal=tuple(float(-x) for x in f32), colour=tuple(COLOUR))])
        if yaw is not None:
            r.set_camera(position=(0.0, 0.0, 0.0), look_at=tuple(float(x) for x in f32))
        if spec:
            r.set_env_guide(SUN, rows=spec[0], cols=spec[1], alpha=spec[2])
        vv, uu = np.divmod(np.arange(n_pix * n_pix), n_pix)
        u = np.tile(uu, n_samples).astype(np.uint16)
        v = np.tile(vv, n_samples).astype(np.uint16)
        s = np.repeat(np.arange(n_samples), n_pix * n_pix).astype(np.uint32)
        p = r.trace_paths(u, v, s)
        esc = p["escaped"] == 1
        Lq = r.env_map_lookup(p["uv"][esc, 0], p["uv"][esc, 1])[:, 0].astype(np.float64)
    finally:
        r.close()
    assert np.all(p["length"][esc] == 2) and np.all(p["length"][~esc] == 1) and np.all(p["escaped"] <= 1)
    X = np.zeros(paths)
    X[esc] = p["throughput"][esc, 0].astype(np.float64) / float(F32(COLOUR[0])) * Lq
    got_mean, got_var = X.mean(), X.var()
    se_mean, se_var = np.sqrt(var / paths), np.sqrt((mu4 - var * var) / paths)
    dead = 1.0 - esc.mean()
    print("%s: mean %.4f (model %.4f, %.2f se)  variance %.1f (model %.1f, %.2f se)  dead %.3f %%" % (
        case, got_mean, mean, (got_mean - mean) / se_mean, got_var, var, (got_var - var) / se_var, 100 * dead))
    assert abs(got_mean - mean) <= 5 * se_mean
    assert abs(got_var - var) <= 6 * se_var
    if spec:
        want_dead = G.dead_share(model, normal, az)
        assert abs(dead - want_dead) <= 5 * np.sqrt(want_dead / paths) + 2e-4     # (quadrature of a step function: 2e-4)
    else:
        assert dead == 0.0


# ---- 5. unbiased with the "wrong" guide

def test_furnace_guided_by_a_sun_map(ptmi_lib):
    """One diffuse sphere of colour c under a constant L, guided by the sun map (which has nothing to do with that light): the
    mean over the paths that hit the sphere is c L / 2 within 5 sigma, sigma from the model's second moment of the mixture."""
    P = ptmi_lib
    n_samples = 1024
    c, L = np.array([0.8, 0.5, 0.25]), 2.0
    centre, radius = np.array([0.0, 0.0, -3.0]), 1.0
    model = G.Guide(SUN, 32, 64, 0.5)
    r = P.Renderer(W, H, max_path_length=8, roulette_depth=8, sample_precision=P.SAMPLES_FLOAT)
    try:
        r.set_constant_env((L, L, L))
        r.init_render_settings(seed=5, aa_noise_scale=0.0)
        r.set_scene([dict(shape="sphere", material="diffuse", centre=tuple(centre), radius=radius, colour=tuple(c))])
        r.set_env_guide(SUN, rows=32, cols=64, alpha=0.5)
        vv, uu = np.divmod(np.arange(W * H), W)
        p = r.trace_paths(np.tile(uu, n_samples), np.tile(vv, n_samples), np.repeat(np.arange(n_samples), W * H))
    finally:
        r.close()
    # the camera ray of every pixel (no AA noise: one ray per pixel) and where it meets the sphere, in float64
    cam = p["cam"][:W * H].astype(np.float64)
    d = np.concatenate([cam, -np.ones((W * H, 1))], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = d @ centre
    disc = b * b - (centre @ centre - radius * radius)
    inside = disc > 0.05                                                    # well inside the silhouette
    t = b[inside] - np.sqrt(disc[inside])
    normals = (d[inside] * t[:, None] - centre) / radius
    mask = np.tile(inside, n_samples)
    n = int(mask.sum())
    X = np.where((p["escaped"] == 1)[:, None], p["throughput"].astype(np.float64) * L, 0.0)[mask]
    second = G.furnace_second_moment(model, normals)
    sigma = c * L * np.sqrt((second - 0.25) / n)
    mean = X.mean(axis=0)
    print("furnace: %d paths, second moment %.4f, mean / (c L / 2) = %s, 5 sigma = %s of the mean" % (
        n, second, mean / (c * L / 2), 5 * sigma / (c * L / 2)))
    assert np.all(5 * sigma < 0.02 * c * L / 2)
    assert np.all(np.abs(mean - c * L / 2) < 5 * sigma), (mean, c * L / 2, sigma)
    assert np.count_nonzero((p["escaped"] == 0)[mask]) > 100                # the guide did send paths below the surface


# ---- 6. multi-bounce agreement, and 8. the CLI

FW, FH, FSPP, FSTEPS = 64, 48, 128, 16


@pytest.fixture(scope="module")
def film_means(ptmi_lib):
    """Per-channel whole-image means (B, G, R) of 16 independent steps of the built-in scene under the procedural sun map,
    bilinear, unguided and guided: {"off" | "on": float64 [16, 3]}."""
    P = ptmi_lib
    img = G.procedural_sun_map()
    out = {}
    for name in ("off", "on"):
        r = P.Renderer(FW, FH)
        try:
            r.set_env_map(img, "bilinear")
            r.init_render_settings(samples_per_step=FSPP)
            if name == "on":
                r.set_env_guide(img)
            means = []
            for _ in range(FSTEPS):
                rec, st = _step(P, r, FW, FH)
                assert np.all(rec["sampleCount"] == FSPP)
                means.append([rec[ch].astype(np.float64).mean() / FSPP for ch in "bgr"])
            out[name] = np.array(means)
        finally:
            r.close()
    return out


def _combined_se(film_means):
    return np.sqrt(film_means["off"].var(axis=0, ddof=1) / FSTEPS + film_means["on"].var(axis=0, ddof=1) / FSTEPS)


def test_multi_bounce_films_agree(film_means):
    off, on = film_means["off"].mean(axis=0), film_means["on"].mean(axis=0)
    se = _combined_se(film_means)
    print("film means off %s on %s, difference / combined se %s; step-mean variance ratio off / on %s" % (
        off, on, (on - off) / se, film_means["off"].var(axis=0, ddof=1) / film_means["on"].var(axis=0, ddof=1)))
    assert np.all(np.abs(on - off) <= 5 * se)
    assert np.all(on != off)


def test_cli_env_guide(film_means, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    img = G.procedural_sun_map()
    h, w, _ = img.shape
    with open(tmp_path / "sun.pfm", "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1, :, ::-1], dtype="<f4").tobytes())
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    means = {}
    for name, extra in (("off", []), ("on", ["--env-guide", "map"])):
        out = tmp_path / (name + ".png")
        r = subprocess.run([exe, "--assets", str(tmp_path), "--env-map", str(tmp_path / "sun.pfm"), "-w", str(FW), "-h", str(FH),
                            "-s", str(FSPP * FSTEPS), "--samples-per-step", str(FSPP), "-o", str(out), "--save-interval", str(FSTEPS)]
                           + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert ("Environment guide" in r.stdout + r.stderr) == (name == "on")
        film = np.zeros((FH, FW, 3), dtype=np.float32)
        ww, hh = C.c_size_t(), C.c_size_t()
        assert L.pth_read_exr(str(tmp_path / (name + ".exr")).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
        assert (ww.value, hh.value) == (FW, FH)
        means[name] = film.astype(np.float64).reshape(-1, 3).mean(axis=0)
    se = _combined_se(film_means)
    print("CLI means off %s on %s, difference / combined se %s" % (means["off"], means["on"], (means["on"] - means["off"]) / se))
    assert np.all(np.abs(means["on"] - means["off"]) <= 5 * se)
    # the CLI's runs are the library's: the same seed, steps and guide (the default grid and alpha)
    for name in ("off", "on"):
        np.testing.assert_allclose(means[name], film_means[name].mean(axis=0), rtol=1e-5)
    assert np.all(means["on"] != means["off"])


# ---- 7. independence of the rest

def test_sharing_memo_features_and_denoiser_do_not_notice_the_guide(ptmi_lib):
    P = ptmi_lib
    spp = 4
    r = _renderer(P, "crowd", "moved", True, "nif", spp=spp, ipb=2)
    try:
        feat0 = r.feature_buffers()
        noisy = np.random.default_rng(1).random((H, W, 3)).astype(F32)
        den0 = r.denoise(image=noisy)
        r.set_env_guide(SUN, rows=16, cols=32, alpha=0.5)
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
