"""HDR environment map on the GPU (pt_set_env_map, pt_env_map_lookup): lookups against numpy for both filters, with the edge
set and the seam; a constant map against the constant environment; a render against the per-path records; sharing and the
memo on a map; switching between the three kinds of environment; the CLI's --env-map."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
META = nif_assets.URBAN_ALLEY_META
EPS = 2.0 ** -24
MAP_SIZES = ((1, 1), (2, 2), (5, 3), (64, 32))   # W x H
COUNTS = (1, 63, 257, 4096)


def _map(W, H, seed=0, lo=0.0, hi=4.0):
    return np.random.default_rng(1000 * W + H + seed).uniform(lo, hi, (H, W, 3)).astype(np.float32)


def _reference(img, u, v, bilinear):
    """The mapping of include/ptmi.h in numpy: x and y from the same single fp32 multiply, clamps and wraps as stated, the lerp
    in float64.  Returns (BGR float64 [n, 3], largest corner per lookup and channel [n, 3])."""
    H, W, _ = img.shape
    u = np.asarray(u, dtype=np.float32)
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        uc = np.where(np.isnan(u), np.float32(0), np.minimum(np.maximum(u, np.float32(0)), np.float32(1))).astype(np.float32)
        vc = np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1))).astype(np.float32)
    y = uc * np.float32(H)
    x = vc * np.float32(W)
    assert y.dtype == np.float32 and x.dtype == np.float32
    y0, x0 = np.floor(y), np.floor(x)
    fy, fx = (y - y0).astype(np.float64), (x - x0).astype(np.float64)
    r0 = np.minimum(y0.astype(np.int64), H - 1)
    r1 = np.minimum(r0 + 1, H - 1)
    c0 = x0.astype(np.int64) % W
    c1 = (c0 + 1) % W
    t00, t01, t10, t11 = (img[a, b].astype(np.float64) for a, b in ((r0, c0), (r0, c1), (r1, c0), (r1, c1)))
    if not bilinear:
        return t00, t00
    top = t00 + fx[:, None] * (t01 - t00)
    bot = t10 + fx[:, None] * (t11 - t10)
    return top + fy[:, None] * (bot - top), np.maximum(np.maximum(t00, t01), np.maximum(t10, t11))


def _check_lookup(r, img, u, v, bilinear):
    got = r.env_map_lookup(u, v)
    want, M = _reference(img, u, v, bilinear)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    if not bilinear:
        assert got.tobytes() == want.astype(np.float32).tobytes()      # texel (r0, c0), bit for bit
        return
    # top and bot each err by <= 3 eps M (the difference and the fmaf round once each, the exact value is within [0, M]), the
    # result by <= 12 eps M; allowed: 16 eps M
    err = np.abs(got.astype(np.float64) - want)
    bound = 16 * EPS * M
    print("bilinear %dx%d n=%d: max err / (eps M) = %.3f" % (img.shape[1], img.shape[0], len(u), float(np.max(err / np.maximum(EPS * M, 1e-300)))))
    assert np.all(err <= bound)


def _edge_set(W):
    one_below = np.nextafter(np.float32(1), np.float32(0))
    us = np.float32([0, 1, one_below, np.nan, np.inf, -np.inf, -0.25, 1.5])
    vs = np.float32([0, 1, (W - 0.5) / W, np.nan, np.inf, -np.inf, -0.25, 1.5])
    uu, vv = np.meshgrid(us, vs, indexing="ij")
    return uu.ravel(), vv.ravel()


@pytest.fixture(scope="module")
def small(ptmi_lib):
    r = ptmi_lib.Renderer(8, 8, max_path_length=4)
    yield r
    r.close()


@pytest.mark.parametrize("size", MAP_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("filt", ("nearest", "bilinear"))
def test_lookups_match_numpy(small, size, filt):
    W, H = size
    img = _map(W, H)
    small.set_env_map(img, filt)
    rng = np.random.default_rng(W + 7 * H)
    for n in COUNTS:
        _check_lookup(small, img, rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32), filt == "bilinear")
    # the edge set: what the clamping rule defines, and finite
    u, v = _edge_set(W)
    _check_lookup(small, img, u, v, filt == "bilinear")
    want, _ = _reference(img, u, v, filt == "bilinear")
    assert np.all(np.isfinite(want))
    got = small.env_map_lookup(u, v)
    # u == 1 and everything above it is the last row, v == 1 and everything above it is column 0; NaN and negatives are 0
    last_row_col0 = img[H - 1, 0]
    for uu in (1.0, np.inf, 1.5):
        for vv in (1.0, np.inf, 1.5, 0.0, np.nan, -np.inf, -0.25):
            k = np.flatnonzero((u == np.float32(uu)) & ((v == np.float32(vv)) if not np.isnan(vv) else np.isnan(v)))
            assert k.size == 1 and np.array_equal(got[k[0]], last_row_col0)
    k = np.flatnonzero(np.isnan(u) & np.isnan(v))
    assert np.array_equal(got[k[0]], img[0, 0])
    assert small.env_map_lookup(np.zeros(0), np.zeros(0)).shape == (0, 3)      # n == 0 is a no-op


def test_seam_wraps_to_column_zero(small):
    W, H = 8, 4
    img = _map(W, H, seed=5, lo=1.0, hi=2.0)
    img[:, 0] = (1.0, 2.0, 3.0)
    img[:, W - 1] = (100.0, 200.0, 300.0)                      # 100 x column 0
    small.set_env_map(img, "bilinear")
    u = np.arange(H, dtype=np.float32) / np.float32(H)         # exactly on the rows: fy == 0
    v = np.full(H, (W - 0.5) / W, dtype=np.float32)            # 0.9375: x == 7.5 exactly, half way between columns 7 and 0
    got = small.env_map_lookup(u, v)
    assert np.array_equal(got, np.tile(np.float32([50.5, 101.0, 151.5]), (H, 1)))   # the mean of the two columns, exactly
    small.set_env_map(img, "nearest")
    assert np.array_equal(small.env_map_lookup(u, v), img[:, W - 1])
    assert np.array_equal(small.env_map_lookup(u, np.ones(H, dtype=np.float32)), img[:, 0])    # v == 1 is column 0


def test_texel_offsets_past_two_gib(small):
    """16 bytes per texel: a 16384-wide map crosses byte 2^31 of the device copy at row 8192, so 8194 rows put two rows past
    it.  The heaviest allocation of the suite (1.5 GiB on the host, 2 GiB on the device); the call takes 0.4 s on an MI355X box."""
    W, H = 16384, 8194
    img = np.empty((H, W, 3), dtype=np.float32)
    img[...] = np.arange(H, dtype=np.float32)[:, None, None]    # row r holds r
    img[:, W - 1, :] += 0.5                                     # ... and its last column r + 0.5
    try:
        small.set_env_map(img, "nearest")
        rows = np.array([0, 1, 4095, 8191, 8192, H - 1])
        u = ((rows + 0.5) / H).astype(np.float32)
        got = small.env_map_lookup(np.concatenate([u, u]), np.concatenate([np.zeros(len(rows)), np.full(len(rows), (W - 0.5) / W)]))
        assert np.array_equal(got[:len(rows), 0], rows.astype(np.float32))
        assert np.array_equal(got[len(rows):, 2], rows.astype(np.float32) + 0.5)
    finally:
        small.set_env_map(np.ones((1, 1, 3), dtype=np.float32))      # frees the 2 GiB copy, whatever failed (`small` lives on)


def test_argument_checks(small, ptmi_lib):
    good = _map(5, 3)
    small.set_env_map(good, "nearest")
    probe_u, probe_v = np.float32([0.4]), np.float32([0.7])
    before = small.env_map_lookup(probe_u, probe_v)
    lib = ptmi_lib.load_library()
    img = np.ones((2, 2, 3), dtype=np.float32)
    for w, h, f, ptr in ((0, 2, 1, img.ctypes.data), (2, 0, 1, img.ctypes.data), (16385, 1, 1, img.ctypes.data),
                         (1, 16385, 1, img.ctypes.data), (2, 2, 2, img.ctypes.data), (2, 2, -1, img.ctypes.data), (2, 2, 1, None)):
        assert lib.pt_set_env_map(small.handle, ptr, w, h, f) == -1
    for value in (np.nan, np.inf, -1.0):
        bad = _map(5, 3)
        bad[2, 3, 1] = value
        with pytest.raises(ptmi_lib.PtError) as e:
            small.set_env_map(bad)
        assert e.value.code == -1 and "row 2, column 3, channel 1" in str(e.value)
    with pytest.raises(ValueError):
        small.set_env_map(good, "cubic")
    with pytest.raises(ValueError):
        small.set_env_map(np.ones((4, 4), dtype=np.float32))
    assert np.array_equal(small.env_map_lookup(probe_u, probe_v), before)      # every rejection left the map in force
    r = ptmi_lib.Renderer(8, 8)
    try:
        with pytest.raises(ptmi_lib.PtError) as e:
            r.env_map_lookup(probe_u, probe_v)
        assert e.value.code == -5                                               # PT_ERR_NOT_READY: no map
        r.set_env_map(good)
        r.set_constant_env((1, 1, 1))                                           # the constant replaces the map
        with pytest.raises(ptmi_lib.PtError) as e:
            r.env_map_lookup(probe_u, probe_v)
        assert e.value.code == -5
    finally:
        r.close()


# ---- renders

def _step(P, W, H, env, spp=4, depth=6, ipb=0, mode="off", memo=0, seed=1, aa=0.3):
    """One step on the built-in scene; env = ("map", image, filter) | ("const", rgb) | ("nif", layers)."""
    r = P.Renderer(W, H, max_path_length=depth, iterations_per_batch=ipb)
    try:
        _set_env(r, env)
        r.init_render_settings(seed=seed, aa_noise_scale=aa, samples_per_step=spp)
        r.set_nif_sharing(mode)
        if memo:
            r.set_nif_memo(memo)
        rec = P.worklist(W, H)
        r.setup(rec)
        r.path_trace()
        st = r.read_results(rec).as_dict()
        return rec, st, r.nif_sharing_stats(), r.nif_kernel_name()
    finally:
        r.close()


def _set_env(r, env):
    if env[0] == "map":
        r.set_env_map(env[1], env[2])
    elif env[0] == "const":
        r.set_constant_env(env[1])
    else:
        r.init_nif_weights(env[1], 12, META["max"], nif_assets.folded_mean())


def _all_paths(r, W, H, spp):
    """pt_trace_paths of every sample of every pixel: [H * W, spp] records in worklist order."""
    rr, cc = np.divmod(np.arange(W * H), W)
    u = np.repeat(cc, spp)
    v = np.repeat(rr, spp)
    s = np.tile(np.arange(spp), W * H)
    return r.trace_paths(u, v, s).reshape(W * H, spp)


def test_constant_map_equals_constant_environment(ptmi_lib):
    P = ptmi_lib
    W = H = 32
    L_bgr = (0.25, 1.5, 3.0)
    const, st_c, _, _ = _step(P, W, H, ("const", L_bgr[::-1]))
    img = np.tile(np.float32(L_bgr), (3, 5, 1))                  # 5 x 3 (W x H) texels, all L
    r = P.Renderer(W, H, max_path_length=6)
    try:
        r.init_render_settings(seed=1, samples_per_step=4)
        paths = _all_paths(r, W, H, 4)
    finally:
        r.close()
    escaped = int(np.count_nonzero(paths["escaped"] == 1))
    assert escaped > 0
    for filt in ("nearest", "bilinear"):
        rec, st, share, name = _step(P, W, H, ("map", img, filt))
        assert rec.tobytes() == const.tobytes()                   # the lerp of equal corners is L exactly; the multiply is the same one
        assert st["escaped"] == escaped == st_c["escaped"]
        assert st["nif_flops_per_sample"] == 0
        assert st["nif_launches"] == st["trace_launches"] >= 1          # the N stage ran, with the map kernel
        assert share["evaluations"] == escaped
        assert name == "envmap_" + filt


def test_render_matches_the_per_path_records(ptmi_lib):
    P = ptmi_lib
    W = H = 16
    spp = 4
    img = _map(64, 32, seed=3, lo=0.5, hi=2.0)
    rec, st, _, _ = _step(P, W, H, ("map", img, "bilinear"), spp=spp, ipb=1)
    assert st["trace_launches"] == 4                               # four batches: both buffer sets are reused
    r = P.Renderer(W, H, max_path_length=6)
    try:
        r.init_render_settings(seed=1, samples_per_step=spp)
        paths = _all_paths(r, W, H, spp)
    finally:
        r.close()
    flat = paths.ravel()
    bgr, _ = _reference(img, flat["uv"][:, 0], flat["uv"][:, 1], True)
    hit = (flat["escaped"] == 1)[:, None]
    rgb = np.where(hit, bgr[:, ::-1] * flat["throughput"].astype(np.float64), 0.0).reshape(W * H, spp, 3).sum(axis=1)
    assert np.count_nonzero(rgb) > W * H
    # corners lie within 4x of any result (texels in [0.5, 2]): the lookup errs by <= 64 eps relative, the multiply adds eps,
    # the fp32 sums of four samples 3 eps: <= 68 * 2^-24 = 4.1e-6
    for k, c in enumerate("rgb"):
        rel = np.abs(rec[c].astype(np.float64) - rgb[:, k]) / np.maximum(rgb[:, k], 1e-300)
        print("channel %s: max rel err %.3e" % (c, float(np.max(np.where(rgb[:, k] > 0, rel, 0.0)))))
        np.testing.assert_allclose(rec[c], rgb[:, k], rtol=5e-6, atol=0)


def test_sharing_and_memo_are_exact_on_a_map(ptmi_lib):
    P = ptmi_lib
    W = H = 32
    a = _map(64, 32, seed=11, lo=0.5, hi=2.0)
    b = _map(64, 32, seed=12, lo=0.5, hi=2.0)
    env = ("map", a, "bilinear")
    # Sharing is between bit-identical (u, v).  With the default pixel jitter a step this small has none (the CPU oracle finds
    # 7760 distinct lookups among its 7760 escaped paths), so the jitter is switched off: the 8 samples of a pixel then leave
    # the camera along one ray, and those that reach the sky directly are the same lookup (2550 distinct of 7740 in the oracle).
    aa = 0.0
    off, st, share_off, _ = _step(P, W, H, env, spp=8, ipb=2, aa=aa)
    assert share_off["evaluations"] == st["escaped"] > 0
    for kw in (dict(mode="batch"), dict(mode="step"), dict(memo=1 << 20)):
        rec, st2, share, _ = _step(P, W, H, env, spp=8, ipb=2, aa=aa, **kw)
        assert rec.tobytes() == off.tobytes(), kw
        assert st2["escaped"] == st["escaped"]
        print(kw, "evaluations", share["evaluations"], "of", st["escaped"], "escaped")
        assert share["evaluations"] < st["escaped"], kw
    # ... and the step as it usually is, with the default jitter, where no two lookups collide: the same bytes again
    plain, st_p, _, _ = _step(P, W, H, env, spp=8, ipb=2)
    for kw in (dict(mode="batch"), dict(mode="step"), dict(memo=1 << 20)):
        rec, st2, share, _ = _step(P, W, H, env, spp=8, ipb=2, **kw)
        assert rec.tobytes() == plain.tobytes(), kw
        assert st2["escaped"] == st_p["escaped"] and 0 < share["evaluations"] <= st_p["escaped"]
    # a new map is a new memo generation: map A, then map B, equals map B without a memo
    results = []
    for memo in (1 << 20, 0):
        r = P.Renderer(W, H, max_path_length=6, iterations_per_batch=2)
        try:
            if memo:
                r.set_nif_memo(memo)
            r.set_env_map(a)
            r.init_render_settings(seed=1, aa_noise_scale=aa, samples_per_step=8)
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            gen = r.nif_memo_stats()["generation"]
            r.set_env_map(b)
            assert r.nif_memo_stats()["generation"] == gen + 1
            r.init_render_settings(seed=2, aa_noise_scale=aa, samples_per_step=8)   # another seed and back: the sample sequence restarts
            r.init_render_settings(seed=1, aa_noise_scale=aa, samples_per_step=8)
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            r.read_results(rec)
            if memo:
                assert r.nif_memo_stats()["served"] == 0              # nothing of map A's values was used
            results.append(rec)
        finally:
            r.close()
    assert results[0].tobytes() == results[1].tobytes()
    only_b, _, _, _ = _step(P, W, H, ("map", b, "bilinear"), spp=8, ipb=2, aa=aa)
    assert results[1].tobytes() == only_b.tobytes() != off.tobytes()


def test_switching_between_the_kinds_of_environment(ptmi_lib):
    P = ptmi_lib
    W = H = 32
    layers = nif_assets.synthetic_nif()
    img = _map(5, 3, seed=2, lo=0.5, hi=2.0)
    r = P.Renderer(W, H, max_path_length=6)
    try:
        def step(seed_other=7):
            r.init_render_settings(seed=seed_other, samples_per_step=2)   # another seed and back: the sample sequence restarts
            r.init_render_settings(seed=1, samples_per_step=2)
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            st = r.read_results(rec)
            return rec, st

        _set_env(r, ("nif", layers))
        nif1, st1 = step()
        assert st1.nif_flops_per_sample > 0 and r.nif_kernel_name().startswith("nif_kernel")
        r.calibrate_nif(1)
        r.set_env_map(img)
        with pytest.raises(P.PtError) as e:
            r.calibrate_nif(1)
        assert e.value.code == -5                                      # PT_ERR_NOT_READY, as with a constant environment
        m1, stm = step()
        assert stm.nif_flops_per_sample == 0 and r.nif_kernel_name() == "envmap_bilinear"
        assert m1.tobytes() != nif1.tobytes() and np.array_equal(m1["pathLength"], nif1["pathLength"])
        with pytest.raises(P.PtError) as e:
            r.calibrate_nif(1)
        assert e.value.code == -5
        # a rejected map leaves the previous one in force
        bad = img.copy()
        bad[1, 4, 2] = np.nan
        with pytest.raises(P.PtError) as e:
            r.set_env_map(bad)
        assert e.value.code == -1 and "row 1, column 4, channel 2" in str(e.value)
        m2, _ = step()
        assert m2.tobytes() == m1.tobytes()
        # ... and the same NIF again reproduces the first NIF records
        _set_env(r, ("nif", layers))
        nif2, st2 = step()
        assert nif2.tobytes() == nif1.tobytes() and st2.escaped == st1.escaped
        with pytest.raises(P.PtError):
            r.env_map_lookup(np.float32([0.5]), np.float32([0.5]))     # the NIF replaced the map
    finally:
        r.close()


def test_cli_env_map(tmp_path):
    from ipu_path_trace_amd import ptmi as P
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    W = H = 64
    spp = 4
    img = _map(16, 8, seed=9, lo=0.5, hi=2.0)
    with open(tmp_path / "sky.pfm", "wb") as f:
        f.write(b"PF\n16 8\n-1.0\n")
        f.write(np.ascontiguousarray(img[::-1, :, ::-1], dtype="<f4").tobytes())
    films = {}
    for filt in ("bilinear", "nearest"):
        out = tmp_path / (filt + ".png")
        r = subprocess.run([exe, "--assets", str(tmp_path), "--env-map", str(tmp_path / "sky.pfm"), "--env-map-filter", filt,
                            "-w", str(W), "-h", str(H), "-s", str(spp), "--samples-per-step", str(spp), "-o", str(out),
                            "--save-interval", "1"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        subprocess.check_call(["make", "-C", HOST, "-s"])
        L = C.CDLL(os.path.join(HOST, "libpthost.so"))
        L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        film = np.zeros((H, W, 3), dtype=np.float32)
        ww, hh = C.c_size_t(), C.c_size_t()
        assert L.pth_read_exr(str(tmp_path / (filt + ".exr")).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
        assert (ww.value, hh.value) == (W, H)
        rd = P.Renderer(W, H)
        try:
            rd.set_env_map(img, filt)
            rd.init_render_settings(samples_per_step=spp)
            rec = P.worklist(W, H)
            rd.setup(rec)
            rd.path_trace()
            rd.film_accumulate()
            want = rd.gather_hdr(W * H, P.HDR_FILM)[0].reshape(H, W, 3)
        finally:
            rd.close()
        assert np.count_nonzero(film) > 0
        assert film.tobytes() == want.tobytes(), filt
        films[filt] = film
    assert films["bilinear"].tobytes() != films["nearest"].tobytes()
