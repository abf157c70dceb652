"""The environment guide built from the environment in force, on the device (pt_set_env_guide_from_environment).

The contract (include/ptmi.h): the guide is pt_set_env_guide of the image I the environment gives at the grid points, clamped.
Every comparison here is exact.  The expected tables come from tests/env_guide_model.Guide over the image obtained from
Renderer.nif_infer / env_map_lookup at the grid points (a constant: that BGR), clamped in numpy; the library's other route --
set_env_guide(I) followed by env_guide_tables() -- is compared exactly too.

1. Every kernel family, a map with both filters at a size that is no power of two, a constant; grids from two lookups up to
   16 planes.
2. The clamp: a model whose decode gives +inf, NaN and negative values on parts of the grid.
3. Zero tolerance end to end: a film guided from the environment is byte-identical to the film guided by the image.
4. follow: a replaced environment rebuilds the tables; a black one leaves them stale.
5. Isolation: nothing else of the handle moves.
6. Errors.
7. The CLI.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import env_guide_model as G
from tests import nif_edge_models as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
FLT_MAX = np.finfo(F32).max
META = nif_assets.URBAN_ALLEY_META
NOT_READY, INVALID = -5, -1
ALPHA = 0.5

# (rows, cols, S): two lookups, fewer than any kernel tile; 32 lookups; four planes of 128; sixteen planes (fused family only)
GRIDS = [(1, 2, 1), (4, 8, 1), (8, 16, 2)]
GRID_16_PLANES = (8, 16, 4)


def _random_map(seed, h=24, w=40):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3)) ** 3 * 50.0).astype(F32)


MAP_A, MAP_B = _random_map(5), _random_map(6)
CONSTANT = (0.3, 0.9, 0.5)     # R, G, B as set_constant_env takes them


def _grid_uv(rows, cols, S):
    """u = ((float)r + 0.5f) / (float)(rows S), v = ((float)c + 0.5f) / (float)(cols S) of the image I, row-major."""
    hh, ww = rows * S, cols * S
    u = (np.arange(hh, dtype=F32) + F32(0.5)) / F32(hh)
    v = (np.arange(ww, dtype=F32) + F32(0.5)) / F32(ww)
    return np.repeat(u, ww), np.tile(v, hh)


def _clamp(img):
    """x' = x >= 0 ? fminf(x, FLT_MAX) : 0, and the number of values it replaced."""
    zero = np.isnan(img) | (img < 0)
    top = np.isposinf(img)
    out = img.copy()
    out[zero] = 0
    out[top] = FLT_MAX
    return out, int(zero.sum() + top.sum())


def _image(r, kind, rows, cols, S):
    """(I, I clamped, replaced): what the environment in force gives at the grid points, through the library's own lookups."""
    u, v = _grid_uv(rows, cols, S)
    if kind == "nif":
        raw = r.nif_infer(u, v)
    elif kind == "map":
        raw = r.env_map_lookup(u, v)
    else:
        raw = np.tile(np.array(kind[::-1], F32), (u.size, 1))     # (B, G, R) of the constant
    raw = raw.reshape(rows * S, cols * S, 3)
    img, replaced = _clamp(raw)
    return raw, img, replaced


def _assert_tables(r, img, rows, cols, alpha, what):
    """env_guide_tables() equals the model's tables over img, entry for entry."""
    M = G.Guide(img, rows, cols, alpha)
    thr, alias, q = r.env_guide_tables()
    assert np.array_equal(thr, M.thr), what
    assert np.array_equal(alias, M.alias), what
    assert np.array_equal(q.view(np.uint32), M.q.view(np.uint32)), what
    return thr, alias, q


def _check_build(r, kind, rows, cols, S, what, alpha=ALPHA, expect_clamped=False):
    before = r.env_guide_info()["rebuilds"]
    r.set_env_guide_from_environment(rows, cols, alpha, S, follow=False)
    info = r.env_guide_info()
    raw, img, replaced = _image(r, kind, rows, cols, S)
    print("%s: %d x %d, S = %d: build_ms %.3f, clamped %d (model %d)" % (what, rows, cols, S, info["build_ms"], info["clamped"], replaced))
    assert info["set"] and info["source"] == "environment" and (info["rows"], info["cols"], info["supersample"]) == (rows, cols, S)
    assert info["alpha"] == F32(int(np.float64(F32(alpha)) * G.TWO32) / G.TWO32) and not info["follow"] and not info["stale"]
    assert info["rebuilds"] == before + 1 and info["build_ms"] > 0
    assert info["clamped"] == replaced and (replaced > 0) == expect_clamped, what
    got = _assert_tables(r, img, rows, cols, alpha, what)
    # the library's other route: the same image through pt_set_env_guide
    r.set_env_guide(img, rows=rows, cols=cols, alpha=alpha)
    info = r.env_guide_info()
    assert info["source"] == "image" and info["supersample"] == 0 and not info["follow"] and info["clamped"] == 0
    other = r.env_guide_tables()
    for a, b in zip(got, other):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    return raw


# ---- 1. every source

def _fused():
    L = nif_assets.synthetic_nif()
    g = np.load(os.path.join(GOLD, "nif_6x320_seed2024.npz"))
    assert hashlib.sha256(L[0][0].tobytes()).digest() == g["w0_sha"].tobytes()     # the model of the golden file
    return L


NIF_SOURCES = {
    "fused_fp16": (_fused, "nif_kernel_v3<320", [GRID_16_PLANES]),
    "wide_layer_by_layer": (lambda: nif_assets.synthetic_nif(hidden=512, layer_count=3), "nifg16_layer_kernel", []),
    "float32": (lambda: nif_assets.synthetic_nif(hidden=64, layer_count=3, dtype=np.float32), "nif32_layer_kernel", []),
}


@pytest.mark.parametrize("family", list(NIF_SOURCES))
def test_nif_families(ptmi_lib, family):
    make, kernel, extra = NIF_SOURCES[family]
    r = ptmi_lib.Renderer(16, 16)
    try:
        r.init_nif_weights(make(), 12, META["max"], nif_assets.folded_mean())
        for rows, cols, S in GRIDS + extra:
            _check_build(r, "nif", rows, cols, S, family)
            assert kernel in r.nif_kernel_name(), (family, r.nif_kernel_name())
    finally:
        r.close()


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_map(ptmi_lib, filt):
    r = ptmi_lib.Renderer(16, 16)
    try:
        r.set_env_map(MAP_A, filt)
        for rows, cols, S in GRIDS:
            _check_build(r, "map", rows, cols, S, "map " + filt)
    finally:
        r.close()


def test_constant(ptmi_lib):
    r = ptmi_lib.Renderer(16, 16)
    try:
        r.set_constant_env(CONSTANT)
        for rows, cols, S in GRIDS:
            _check_build(r, CONSTANT, rows, cols, S, "constant")
    finally:
        r.close()


# ---- 2. the clamp

@pytest.mark.parametrize("case", ["nan_to_output", "nan_to_output_linear_decode"])
def test_clamp(ptmi_lib, case):
    """The head of tests/nif_edge_models.py's nan_to_output gives +inf on one part of the grid and NaN on another; with the
    linear decode also negative values and -inf.  clamped counts them and the tables are the model's over the clamped image."""
    L, log_tonemap = E.build(case, [64] * 3, 4, [np.float16] * 4)
    r = ptmi_lib.Renderer(16, 16)
    try:
        r.init_nif_weights(L, 4, META["max"], nif_assets.folded_mean(), log_tonemap=log_tonemap)
        raw = _check_build(r, "nif", 8, 16, 2, case, expect_clamped=True)
        assert np.isnan(raw).any() and np.isposinf(raw).any() and (np.isfinite(raw) & (raw > 0)).any()
        if not log_tonemap:
            assert (raw < 0).any()
    finally:
        r.close()


# ---- 3. zero tolerance end to end

def test_film_is_byte_identical_to_the_image_route(ptmi_lib):
    """sun_map() as the map, nearest filter; the guide from the environment at 32 x 64 with S = 1 looks every texel up exactly
    once (u H = r + 0.5), so it IS the guide of the image: a 64 x 64, 16 spp, depth 4 film must not differ by a bit."""
    P = ptmi_lib
    sun = G.sun_map()
    r = P.Renderer(64, 64, max_path_length=4)
    try:
        r.set_env_map(sun, "nearest")

        def film():
            r.init_render_settings(seed=12, samples_per_step=16)
            r.init_render_settings(seed=11, samples_per_step=16)      # a new seed: the sample cursor back to 0
            rec = P.worklist(64, 64)
            r.setup(rec)
            r.path_trace()
            r.read_results(rec)
            return rec.tobytes()

        unguided = film()
        r.set_env_guide_from_environment(32, 64, ALPHA, 1, follow=False)
        u, v = _grid_uv(32, 64, 1)
        assert np.array_equal(r.env_map_lookup(u, v).reshape(32, 64, 3), sun)
        from_env = film()
        r.set_env_guide(sun, rows=32, cols=64, alpha=ALPHA)
        from_image = film()
    finally:
        r.close()
    assert from_env == from_image
    assert from_env != unguided       # not vacuous: the guide does change the film


# ---- 4. follow

def _small_nif(seed=3):
    return nif_assets.synthetic_nif(hidden=64, layer_count=3, embedding_dim=4, seed=seed)


def test_follow(ptmi_lib):
    rows, cols, S = 8, 16, 2
    r = ptmi_lib.Renderer(16, 16)
    try:
        r.set_env_map(MAP_A, "bilinear")
        r.set_env_guide_from_environment(rows, cols, ALPHA, S, follow=True)
        info = r.env_guide_info()
        assert info["follow"] and info["rebuilds"] == 1
        tables_a = _assert_tables(r, _image(r, "map", rows, cols, S)[1], rows, cols, ALPHA, "map A")
        # another map
        r.set_env_map(MAP_B, "nearest")
        assert r.env_guide_info()["rebuilds"] == 2
        tables_b = _assert_tables(r, _image(r, "map", rows, cols, S)[1], rows, cols, ALPHA, "map B")
        assert not np.array_equal(tables_a[0], tables_b[0])
        # a NIF (the interactive load_nif)
        r.init_nif_weights(_small_nif(), 4, META["max"], nif_assets.folded_mean())
        info = r.env_guide_info()
        assert info["rebuilds"] == 3 and info["follow"] and not info["stale"] and info["source"] == "environment"
        tables_n = _assert_tables(r, _image(r, "nif", rows, cols, S)[1], rows, cols, ALPHA, "nif")
        # a black constant is a valid environment, not a valid guide: the call succeeds, the tables stay, stale
        r.set_constant_env((0, 0, 0))
        info = r.env_guide_info()
        assert info["stale"] and info["rebuilds"] == 3 and info["set"] and info["follow"]
        for a, b in zip(tables_n, r.env_guide_tables()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # the next environment with light in it clears it
        r.set_constant_env(CONSTANT)
        info = r.env_guide_info()
        assert not info["stale"] and info["rebuilds"] == 4
        tables_c = _assert_tables(r, _image(r, CONSTANT, rows, cols, S)[1], rows, cols, ALPHA, "constant")
        # a trained NIF installed on the handle
        r.set_env_map(MAP_A, "bilinear")
        assert r.env_guide_info()["rebuilds"] == 5
        t = r.train_nif(embedding_dim=4, hidden=32, layer_count=1, batch=256)
        t.steps(2)
        t.install()
        t.close()
        assert r.env_guide_info()["rebuilds"] == 6
        _assert_tables(r, _image(r, "nif", rows, cols, S)[1], rows, cols, ALPHA, "trained nif")
        # follow = 0: the same calls leave the tables alone
        r.set_constant_env(CONSTANT)
        r.set_env_guide_from_environment(rows, cols, ALPHA, S, follow=False)
        base = r.env_guide_info()["rebuilds"]
        r.set_env_map(MAP_B, "nearest")
        r.init_nif_weights(_small_nif(4), 4, META["max"], nif_assets.folded_mean())
        r.set_constant_env((0, 0, 0))
        info = r.env_guide_info()
        assert info["rebuilds"] == base and not info["stale"] and not info["follow"]
        for a, b in zip(tables_c, r.env_guide_tables()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # a guide from an image does not follow either, and turns follow off
        r.set_constant_env(CONSTANT)
        r.set_env_guide_from_environment(rows, cols, ALPHA, S, follow=True)
        r.set_env_guide(G.sun_map(), rows=rows, cols=cols, alpha=ALPHA)
        sun_tables = r.env_guide_tables()
        r.set_env_map(MAP_B, "nearest")
        info = r.env_guide_info()
        assert info["source"] == "image" and not info["follow"] and info["rebuilds"] == base + 1
        for a, b in zip(sun_tables, r.env_guide_tables()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        r.set_env_guide(None)
        assert not r.env_guide_info()["set"]
        with pytest.raises(ptmi_lib.PtError) as e:
            r.env_guide_tables()
        assert e.value.code == NOT_READY
    finally:
        r.close()


# ---- 5. isolation

def test_nothing_else_moves(ptmi_lib):
    P = ptmi_lib
    W = H = 48
    r = P.Renderer(W, H, max_path_length=6)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.set_nif_sharing("step")
        r.set_nif_memo(1 << 24)
        r.init_render_settings(seed=5, samples_per_step=4)
        rec = P.worklist(W, H)
        r.setup(rec)
        r.path_trace()
        r.film_accumulate()
        r.path_trace()
        feats = r.feature_buffers()

        def snapshot():
            out = P.worklist(W, H)
            st = r.read_results(out)
            return (out.tobytes(), r.gather_hdr(W * H, P.HDR_FILM).tobytes(), st.as_dict(), r.stats().as_dict(), r.nif_kernel_name(),
                    r.nif_sharing_stats(), r.nif_memo_stats())

        before = snapshot()
        r.set_env_guide_from_environment(8, 16, ALPHA, 2, follow=True)
        after = snapshot()
        assert before == after
        assert r.env_guide_info()["rebuilds"] == 1
        ms, evaluations = r.calibrate_nif(1)          # the replay state of the last step is still there
        assert evaluations > 0 and ms > 0
        again = r.feature_buffers()
        for k in feats:
            assert np.array_equal(np.asarray(feats[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8))
    finally:
        r.close()


# ---- 6. errors

def test_errors_keep_the_previous_guide(ptmi_lib):
    P = ptmi_lib
    r = P.Renderer(16, 16)
    try:
        with pytest.raises(P.PtError) as e:              # a fresh handle: no environment has ever been set
            r.set_env_guide_from_environment(8, 16, ALPHA, 2)
        assert e.value.code == NOT_READY and "no environment has been set" in str(e.value)
        assert not r.env_guide_info()["set"]
        sun = G.sun_map()
        r.set_env_guide(sun, rows=8, cols=16, alpha=0.25)
        kept = r.env_guide_tables()
        r.set_constant_env((0, 0, 0))
        with pytest.raises(P.PtError) as e:              # a black constant: refused, naming the total
            r.set_env_guide_from_environment(8, 16, ALPHA, 2)
        assert e.value.code == INVALID and "total mass" in str(e.value)
        r.set_constant_env(CONSTANT)
        r.set_light_guide(0.5)
        with pytest.raises(P.PtError) as e:              # alpha + beta against the light guide that is set
            r.set_env_guide_from_environment(8, 16, 0.5, 2)
        assert e.value.code == INVALID and "alpha + beta" in str(e.value)
        info = r.env_guide_info()
        assert info["set"] and info["source"] == "image" and info["alpha"] == 0.25 and info["rebuilds"] == 0
        for a, b in zip(kept, r.env_guide_tables()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        r.set_env_guide_from_environment(8, 16, 0.4, 2)  # 0.4 + 0.5 is within the cap
        assert r.env_guide_info()["source"] == "environment"
        with pytest.raises(P.PtError) as e:
            r._check(r._lib.pt_get_env_guide_tables(r.handle, None, None, None, 7))
        assert e.value.code == INVALID
    finally:
        r.close()


# ---- 7. the CLI

def test_cli_env_guide_env(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    assets = tmp_path / "assets.extra"
    assets.mkdir()
    nif_assets.write_metadata(str(assets / "nif_metadata.txt"))
    nif_assets.write_ptnif(str(assets / "converted.ptnif"), nif_assets.synthetic_nif(), 12)
    base = ["-w", "64", "-h", "48", "-s", "8", "--samples-per-step", "4", "--save-interval", "2", "-o", str(tmp_path / "o.png"),
            "--env-guide", "env"]
    r = subprocess.run([exe, "--assets", str(assets), "--env-guide-size", "16x32", "--env-guide-supersample", "2"] + base,
                       capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "16 x 32 cells, supersample 2, build_ms" in log, log[-4000:]
    assert (tmp_path / "o.png").exists() and (tmp_path / "o.exr").exists()
    # no environment option at all: refused with the library's message
    r = subprocess.run([exe] + base, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "no environment has been set (none of pt_upload_nif, pt_set_env_map, pt_set_constant_env" in r.stdout + r.stderr
