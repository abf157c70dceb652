"""The A-trous film denoiser (pt_denoise) on the device against the float64 model of tests/denoise_model.py, closed forms, its
three sources, and the rest of the handle's state.

The bound is derived, not tuned.  One iteration's output is a convex combination of at most 25 inputs, so its rounding error
is at most (25 + 4) 2^-23 M from the sums and the divide, M the largest value of the image the filter works on (the demodulated
one where demodulation is on).  The weights go through expf, the OCML single-precision exponential the kernel calls, documented
at 1 ulp (HIP math API accuracy table): a relative error e = 2^-23 of the weights moves a ratio of weighted sums by at most
2 e M.  That, times the iterations, plus two roundings (2 x 2^-24 M) for the division and the multiplication of the
demodulation; a demodulated result is multiplied by max(albedo, 1e-3), and so is its bound, per pixel and channel.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_model as DM
from tests import scene_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
EXP_ULP = 2.0 ** -23               # expf (OCML): 1 ulp
SIZES = [(1, 1), (7, 5), (33, 17), (64, 64)]          # W x H: three smaller than the reach of the later steps, none a multiple of the tile
OFF = dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, object_stop=0)
PARAMS = ([dict(iterations=i) for i in (1, 3, 5, 6)] + [dict(iterations=i, demodulate=0) for i in (1, 3, 5, 6)] +
          [dict(OFF, iterations=3, demodulate=d, **{k: v}) for d in (0, 1)
           for k, v in (("sigma_colour", 4.0), ("sigma_normal", 0.5), ("sigma_depth", 0.1), ("object_stop", 1))] +
          [dict(OFF, iterations=6, demodulate=0), dict(iterations=6, sigma_colour=0.7)])


def bound(params, working_max, features):
    p = dict(DM.DEFAULTS, **params)
    b = p["iterations"] * ((25 + 4) * 2.0 ** -23 + 2 * EXP_ULP) * working_max + 2 * 2.0 ** -24 * working_max
    if p["demodulate"]:
        return b * np.maximum(features["albedo"].astype(np.float64), DM.ALBEDO_FLOOR)
    return np.full(features["albedo"].shape, b)


def _crowd_renderer(P, W, H):
    r = P.Renderer(W, H, max_path_length=6, roulette_depth=2)
    r.set_constant_env((0.6, 0.8, 1.0))
    r.init_render_settings(seed=5, samples_per_step=2, aa_noise_scale=0.3)
    r.set_scene(M.world_scene("crowd", "none"))
    return r


@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_against_the_model(ptmi_lib, W, H):
    P = ptmi_lib
    rng = np.random.default_rng(W * 1000 + H)
    img = rng.uniform(0.0, 4.0, (H, W, 3)).astype(F32)
    r = _crowd_renderer(P, W, H)
    try:
        f = r.feature_buffers()
        got = [r.denoise(image=img, **p) for p in PARAMS]
        const = np.full((H, W, 3), F32(1.75)) * F32([1.0, 0.5, 2.0])
        got_const = [r.denoise(image=const, **p) for p in PARAMS[:8]]
    finally:
        r.close()
    if W >= 33:
        assert len(np.unique(f["object_id"])) >= 5 and (f["object_id"] < 0).any()        # real features: objects and misses
    worst = 0.0
    for p, g in zip(PARAMS, got):
        want, m = DM.denoise(img, f, **p)
        frac = float(np.max(np.abs(g.astype(np.float64) - want) / bound(p, m, f)))
        print("%d x %d %s: %.4f of the bound" % (W, H, p, frac))
        assert g.dtype == F32 and g.shape == (H, W, 3) and np.isfinite(g).all()
        assert frac <= 1.0, p
        worst = max(worst, frac)
        if p.get("object_stop", 1) and not p.get("demodulate", 1):
            # no pixel leaves the [min, max] of the inputs on its own object, widened by the bound
            b = bound(p, m, f)[0, 0, 0]
            for k in np.unique(f["object_id"]):
                sel = f["object_id"] == k
                assert np.all(img[sel].min(0) - b <= g[sel].min(0)) and np.all(g[sel].max(0) <= img[sel].max(0) + b)
    print("%d x %d: largest fraction %.4f" % (W, H, worst))
    # a constant image comes back
    for p, g in zip(PARAMS[:8], got_const):
        m = DM.denoise(const, f, **p)[1]
        assert np.all(np.abs(g.astype(np.float64) - const) <= bound(p, m, f)), p


def test_a_nan_stays_on_its_object(ptmi_lib):
    P = ptmi_lib
    W, H = 33, 17
    r = _crowd_renderer(P, W, H)
    try:
        f = r.feature_buffers()
        ids = f["object_id"]
        k = np.bincount(ids[ids >= 0]).argmax()                       # the object with the most pixels
        img = np.random.default_rng(2).uniform(0.0, 4.0, (H, W, 3)).astype(F32)
        y, x = np.argwhere(ids == k)[len(np.argwhere(ids == k)) // 2]
        img[y, x] = np.nan
        out = r.denoise(image=img, iterations=6, demodulate=0)
        leaky = r.denoise(image=img, iterations=6, demodulate=0, object_stop=0)
    finally:
        r.close()
    assert np.isnan(out[y, x]).all() and np.isnan(out[ids == k]).sum() > 3          # it propagates on its own object ...
    assert np.isfinite(out[ids != k]).all() and (ids != k).sum() > 100               # ... and nowhere else
    assert np.isnan(leaky[ids != k]).any()                                           # which is the object stop's doing


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_sources(ptmi_lib):
    P = ptmi_lib
    W, H, steps = 33, 17, 3
    r = _crowd_renderer(P, W, H)
    try:
        with pytest.raises(P.PtError) as e:
            r.denoise(source="accumulators")
        assert e.value.code == -5                                      # no worklist
        rec = P.worklist(W, H)
        r.setup(rec)
        with pytest.raises(P.PtError) as e:
            r.denoise(source="film")
        assert e.value.code == -5                                      # a worklist, but no film step yet
        r.path_trace()
        r.read_results(rec)
        acc = np.stack([rec["b"], rec["g"], rec["r"]], -1) * (F32(1.0) / rec["sampleCount"].astype(F32))[:, None]
        from_acc = r.denoise(source="accumulators")
        assert np.array_equal(_bits(from_acc), _bits(r.denoise(image=acc.reshape(H, W, 3))))
        assert rec["sampleCount"].min() == 2 and acc.max() > 0.5
        r.film_accumulate()
        for _ in range(steps - 1):
            r.path_trace()
            r.film_accumulate()
        film = r.gather_hdr(W * H, source=P.HDR_FILM)[0]
        host = (film * (F32(1.0) / F32(steps))).reshape(H, W, 3)
        from_film = r.denoise(source="film")
        assert np.array_equal(_bits(from_film), _bits(r.denoise(image=host)))
        assert not np.array_equal(from_film, host)                     # it filtered
        # half the pixels: the other half's inputs are 0
        half = np.ascontiguousarray(P.worklist(W, H)[::2])
        r.setup(half)
        r.path_trace()
        r.read_results(half)
        sparse = np.zeros((H, W, 3), F32)
        sparse[half["v"], half["u"]] = np.stack([half["b"], half["g"], half["r"]], -1) * (F32(1.0) / half["sampleCount"].astype(F32))[:, None]
        plain = dict(DM.DEFAULTS, iterations=1, sigma_colour=0.0, demodulate=0)
        assert np.array_equal(_bits(r.denoise(source="accumulators", **plain)), _bits(r.denoise(image=sparse, **plain)))
        assert (sparse.reshape(-1, 3)[1::2] == 0).all() and sparse.max() > 0.5
        with pytest.raises(ValueError):
            r.denoise(source="host")
        with pytest.raises(ValueError):
            r.denoise(image=np.zeros((H, W + 1, 3), F32))
    finally:
        r.close()


def test_a_render_does_not_notice_the_calls(ptmi_lib):
    """read_results and the resident film of a render with pt_feature_buffers + pt_denoise between its steps equal those of the
    same render without, byte for byte."""
    P = ptmi_lib
    W, H = 33, 17
    out = []
    for calls in (False, True):
        r = _crowd_renderer(P, W, H)
        try:
            rec = P.worklist(W, H)
            r.setup(rec)
            for step in range(3):
                r.path_trace()
                if calls:
                    r.feature_buffers()
                    r.denoise(source="accumulators")
                if step < 2:
                    r.film_accumulate()
                    if calls:
                        r.denoise(source="film", iterations=6)
            st = r.read_results(rec)
            out.append((rec.tobytes(), r.gather_hdr(W * H, source=P.HDR_FILM).tobytes(), st.paths, st.segments, st.escaped))
        finally:
            r.close()
    assert out[0] == out[1] and len(out[0][0]) == 20 * W * H


# ---- the CLI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")


def _read_exr(path, W, H):
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=F32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert L.pth_read_exr(str(path).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    assert (ww.value, hh.value) == (W, H)
    return film


def test_cli_writes_denoised_and_feature_files_beside_unchanged_outputs(ptmi_lib, tmp_path):
    P = ptmi_lib
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    W, H, spp = 64, 48, 4
    objects = [{"shape": "sphere", "centre": [0, 0, -3], "radius": 1, "material": "diffuse", "colour": [1.6, 1.2, 0.8]},
               {"shape": "disc", "centre": [0, -1.6, -5], "normal": [0, 1, 0], "radius": 3.5, "material": "specular"},
               {"shape": "sphere", "centre": [-1.5, 0.5, -3], "radius": 0.5, "material": "refractive", "colour": [0.9, 0.9, 0.7]}]
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps({"objects": objects}))
    base = [exe, "--assets", str(tmp_path), "--constant-env", "1,0.8,0.6", "--scene", str(scene), "-w", str(W), "-h", str(H),
            "-s", str(2 * spp), "--samples-per-step", str(spp), "--max-path-length", "6", "--save-interval", "2"]
    flags = ["--denoise", "--save-features", "--denoise-iterations", "3", "--denoise-sigma-colour", "2.5"]
    outs = {}
    for name, extra in (("plain", []), ("resident", flags), ("hostfilm", flags + ["--host-film"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(base + extra + ["-o", str(d / "img.png")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        outs[name] = d
    assert sorted(os.listdir(outs["plain"])) == ["img.exr", "img.png"]
    want = sorted(["img.exr", "img.png", "img_denoised.exr", "img_denoised.png", "img_normal.exr", "img_albedo.exr", "img_depth.exr"])
    for name in ("resident", "hostfilm"):
        assert sorted(os.listdir(outs[name])) == want
    # the plain outputs are byte-identical to a run without the flags (resident film against resident film)
    for f in ("img.exr", "img.png"):
        assert (outs["resident"] / f).read_bytes() == (outs["plain"] / f).read_bytes()
    # the denoised file is Renderer.denoise of the plain one, from the resident film and from the host film
    r = P.Renderer(W, H)
    try:
        r.init_render_settings()
        r.set_scene([dict(o, shape=o["shape"], material=o["material"]) for o in objects])
        f = r.feature_buffers()
        for name in ("resident", "hostfilm"):
            plain = _read_exr(outs[name] / "img.exr", W, H)
            want_img = r.denoise(image=plain, iterations=3, sigma_colour=2.5)
            assert np.array_equal(_bits(_read_exr(outs[name] / "img_denoised.exr", W, H)), _bits(want_img)), name
            assert not np.array_equal(want_img, plain)
    finally:
        r.close()
    assert np.array_equal(_read_exr(outs["resident"] / "img_normal.exr", W, H), f["normal"])
    assert np.array_equal(_read_exr(outs["resident"] / "img_albedo.exr", W, H), f["albedo"])
    assert np.array_equal(_read_exr(outs["resident"] / "img_depth.exr", W, H)[..., 1], f["depth"])
    # a bad value is refused by the option parser, before a device is attached
    r = subprocess.run(base + ["--denoise", "--denoise-iterations", "9", "-o", str(tmp_path / "bad.png")], capture_output=True, text=True)
    assert r.returncode == 1 and "--denoise-iterations must be 1..6" in r.stdout
    assert "Could not attach" not in r.stdout and "Tracebuffer" not in r.stdout and not (tmp_path / "bad.png").exists()
