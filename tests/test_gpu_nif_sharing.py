"""Exact sharing of NIF evaluations on the GPU (pt_set_nif_sharing): every mode renders the same bits as sharing off, and the
evaluation counts are the distinct (u, v) bit pairs of the escaped paths, counted independently with numpy."""
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
MODES = ("off", "batch", "step")


def _render(P, W, H, layers=None, emb=12, mode="off", depth=8, spp=24, steps=2, rotation=0.0, aa=0, ipb=0, const=None,
            capacity=None):
    """`steps` steps with the film resident; returns (records of every step, resident film, sharing stats of every step)."""
    r = P.Renderer(W, H, max_path_length=depth, aa_noise_type=aa, iterations_per_batch=ipb, diag=capacity is not None)
    try:
        if const is not None:
            r.set_constant_env(const)
        else:
            r.init_nif_weights(layers, emb, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=spp, env_rotation_degrees=rotation)
        if capacity is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_share_capacity(r.handle, capacity) == 0
        r.set_nif_sharing(mode)
        rec = P.worklist(W, H)
        r.setup(rec)
        records, stats = [], []
        for _ in range(steps):
            r.path_trace()
            stats.append(r.nif_sharing_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)
        return b"".join(records), film.tobytes(), stats
    finally:
        r.close()


def _check_modes(P, W, H, layers=None, **kw):
    ref_rec, ref_film, ref_stats = _render(P, W, H, layers, mode="off", **kw)
    for s in ref_stats:
        assert s["mode"] == "off" and s["overflowed"] == 0 and s["table_slots"] == 0
        assert s["evaluations"] == (0 if kw.get("const") is not None else s["escaped"])
    out = {}
    for mode in ("batch", "step"):
        rec, film, stats = _render(P, W, H, layers, mode=mode, **kw)
        assert rec == ref_rec, "records differ with sharing %s" % mode
        assert film == ref_film, "resident film differs with sharing %s" % mode
        for s, o in zip(stats, ref_stats):
            assert s["escaped"] == o["escaped"] and s["evaluations"] <= s["escaped"]
        out[mode] = stats
    return ref_stats, out


def test_full_size_c2_shape_is_bit_identical_in_every_mode(ptmi_lib):
    off, shared = _check_modes(ptmi_lib, 1104, 1000, nif_assets.synthetic_nif(), depth=8, spp=24, steps=2)
    for mode, stats in shared.items():
        for s in stats:
            assert s["mode"] == mode and s["table_slots"] > 0 and 0 < s["evaluations"] < s["escaped"], s
    # a step shares at least what its batches share
    assert sum(s["evaluations"] for s in shared["step"]) <= sum(s["evaluations"] for s in shared["batch"])


@pytest.mark.parametrize("name", ["wide_8x1024", "float32", "mixed", "fused_64_e4", "fused_192_e16", "rotation", "aa_uniform",
                                  "aa_truncated_normal"])
def test_reduced_size_bit_identical_across_kernel_families_and_options(ptmi_lib, name):
    emb, kw = 12, {}
    if name == "wide_8x1024":
        layers = nif_assets.synthetic_nif(hidden=1024, layer_count=8, seed=31)
    elif name == "float32":
        layers = nif_assets.synthetic_nif(hidden=128, layer_count=3, seed=17, dtype=np.float32)
    elif name == "mixed":
        f32 = nif_assets.synthetic_nif(hidden=64, layer_count=3, seed=5, dtype=np.float32)
        layers = [(k.astype(np.float16), b.astype(np.float16), relu) if i % 2 else (k, b, relu) for i, (k, b, relu) in enumerate(f32)]
    elif name == "fused_64_e4":
        emb, layers = 4, nif_assets.synthetic_nif(hidden=64, layer_count=3, embedding_dim=4, seed=3)
    elif name == "fused_192_e16":
        emb, layers = 16, nif_assets.synthetic_nif(hidden=192, layer_count=4, embedding_dim=16, seed=9)
    else:
        layers = nif_assets.synthetic_nif()
        kw = {"rotation": 47.0} if name == "rotation" else {"aa": 1 if name == "aa_uniform" else 2}
    off, shared = _check_modes(ptmi_lib, 160, 120, layers, emb=emb, depth=8, spp=12, steps=2, ipb=4, **kw)
    assert all(s["evaluations"] < s["escaped"] for s in shared["step"])


def test_constant_environment_runs_no_sharing_pass(ptmi_lib):
    off, shared = _check_modes(ptmi_lib, 96, 64, const=(0.5, 1.0, 2.0), depth=6, spp=8, steps=2)
    for stats in shared.values():
        for s in stats:
            assert s["evaluations"] == 0 and s["escaped"] > 0 and s["share_ms"] == 0.0 and s["mode"] == "off"


def _distinct_keys(paths):
    esc = paths["escaped"] != 0
    uv = np.ascontiguousarray(paths["uv"][esc]).view(np.uint32).reshape(-1, 2).astype(np.uint64)
    return (uv[:, 0] << np.uint64(32)) | uv[:, 1], int(esc.sum())


def test_evaluation_counts_are_the_distinct_uv_bit_pairs(ptmi_lib):
    """64 x 48 pixels, 32 iterations per batch, 64 spp: two batches of 32 samples.  pt_trace_paths traces every (pixel, sample)
    with the trace kernel's device functions; its uv is the queue's uv, so numpy counts what the table must find."""
    P = ptmi_lib
    W, H, spp = 64, 48, 64
    layers = nif_assets.synthetic_nif()
    r = P.Renderer(W, H, max_path_length=8, iterations_per_batch=32)
    try:
        r.init_nif_weights(layers, 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=spp)
        px = np.arange(W * H)
        batches = []
        for s0 in (0, 32):
            s = np.repeat(np.arange(s0, s0 + 32, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, 32), np.tile(px // W, 32), s)
            batches.append(_distinct_keys(paths))
        escaped = sum(n for _, n in batches)
        per_batch = sum(np.unique(k).size for k, _ in batches)
        per_step = np.unique(np.concatenate([k for k, _ in batches])).size
        first_batch = np.unique(batches[0][0]).size
        assert per_step < per_batch < escaped
        expect = {"off": escaped, "batch": per_batch, "step": per_step}
        rec = P.worklist(W, H)
        for seed, mode in enumerate(MODES):
            r.init_render_settings(seed=100 + seed, samples_per_step=spp)   # a new seed restarts the sample sequence ...
            r.init_render_settings(seed=1, samples_per_step=spp)            # ... at index 0 with seed 1
            r.set_nif_sharing(mode)
            r.setup(rec)
            r.path_trace()
            st = r.nif_sharing_stats()
            assert st["escaped"] == escaped and r.stats().escaped == escaped
            assert st["evaluations"] == expect[mode], (mode, st, expect)
            assert st["overflowed"] == 0
            if mode != "off":
                # pt_calibrate_nif replays the distinct queue of the largest batch (both are 32 iterations: batch 0)
                ms, evals = r.calibrate_nif(2)
                assert evals == first_batch and ms > 0
        lib = P.load_library()
        assert lib.pt_set_nif_sharing(r.handle, 3) == -1 and lib.pt_set_nif_sharing(r.handle, -1) == -1
        st = P.NifSharingStats()                           # struct_size not set
        assert lib.pt_get_nif_sharing_stats(r.handle, C.byref(st)) == -1
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["batch", "step"])
def test_overflowing_table_stays_exact(ptmi_lib, mode):
    """A 16-slot table (test build hook): most keys find no slot and are evaluated alone; the film does not change."""
    P = ptmi_lib
    layers = nif_assets.synthetic_nif()
    kw = dict(depth=8, spp=16, steps=2, ipb=8)
    ref_rec, ref_film, ref_stats = _render(P, 64, 48, layers, mode="off", **kw)
    rec, film, stats = _render(P, 64, 48, layers, mode=mode, capacity=16, **kw)
    assert rec == ref_rec and film == ref_film
    _, _, full = _render(P, 64, 48, layers, mode=mode, **kw)
    for s, f in zip(stats, full):
        assert s["table_slots"] == 16 and s["overflowed"] > 0 and f["overflowed"] == 0
        assert f["evaluations"] <= s["evaluations"] <= s["escaped"]


def test_lifecycle_between_steps_matches_sharing_off(ptmi_lib, oracle):
    """Mode switches, a NIF hot swap and an azimuth change between steps: no table outlives a step, so every step equals
    the off-mode step bit for bit.  Then a failed step (test build fault injection) with sharing on: the error drains the
    streams, and after pt_setup the next step equals off again."""
    P = ptmi_lib
    W, H = 96, 64
    A = nif_assets.synthetic_nif()
    B = nif_assets.synthetic_nif(hidden=128, layer_count=4, seed=77)
    mean = nif_assets.folded_mean()

    def sequence(modes):
        r = P.Renderer(W, H, max_path_length=7, iterations_per_batch=3, diag=True)
        try:
            r.init_nif_weights(A, 12, META["max"], mean)
            r.init_render_settings(samples_per_step=9)
            rec = P.worklist(W, H)
            r.setup(rec)
            out = []
            for i, mode in enumerate(modes):
                if i == 2:
                    r.init_nif_weights(B, 12, META["max"], mean)                        # hot swap
                if i == 3:
                    r.init_render_settings(samples_per_step=9, env_rotation_degrees=120.0)   # same seed: the sequence continues
                r.set_nif_sharing(mode)
                r.path_trace()
                r.read_results(rec)
                out.append(rec.tobytes())
                r.film_accumulate()
            out.append(r.gather_hdr(W * H, P.HDR_FILM).tobytes())
            # failure in the middle of the batch loop with sharing on (3 batches; batch 1 fails)
            diag = P.load_library(diag=True)
            r.set_nif_sharing("step")
            assert diag.pt_diag_inject_fault(r.handle, 1) == 0
            with pytest.raises(P.PtError) as e:
                r.path_trace()
            assert e.value.code == -3 and "injected fault" in str(e.value)
            assert diag.pt_diag_inject_fault(r.handle, -1) == 0
            r.synchronize()
            r.set_nif_sharing(modes[-1])
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            r.read_results(rec)
            out.append(rec.tobytes())
            return out
        finally:
            r.close()

    ref = sequence(["off"] * 5)
    got = sequence(["batch", "step", "step", "batch", "off"])
    assert len(ref) == len(got) == 7
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a == b, "part %d differs" % i
    got2 = sequence(["step", "off", "batch", "step", "step"])
    assert got2 == ref


def _run_cli(tmp_path, name, extra):
    exe = os.path.join(HOST, "ipu_trace")
    assets = tmp_path / "assets.extra"
    if not assets.exists():
        assets.mkdir()
        nif_assets.write_metadata(str(assets / "nif_metadata.txt"))
        nif_assets.write_ptnif(str(assets / "converted.ptnif"), nif_assets.synthetic_nif(), 12)
    r = subprocess.run([exe, "--assets", str(assets), "-w", "96", "-h", "80", "-s", "12", "--samples-per-step", "4",
                        "--max-path-length", "7", "-o", str(tmp_path / (name + ".png")), "--save-interval", "2"] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return (tmp_path / (name + ".exr")).read_bytes(), r.stdout


@pytest.mark.parametrize("devices", [[], ["--ipus", "2", "--devices", "0,0"]])
def test_cli_share_nif_evaluations_writes_the_same_exr(tmp_path, devices):
    import re
    plain, log = _run_cli(tmp_path, "plain", devices)
    shared, slog = _run_cli(tmp_path, "shared", devices + ["--share-nif-evaluations", "step"])
    assert shared == plain
    lines = re.findall(r"NIF evaluations: executed (\d+) of (\d+) escaped \(([0-9.e+-]+) % shared\)", slog)
    assert len(lines) == 2, slog[-2000:]                         # save intervals at steps 2 and 3
    for x, y, z in lines:
        assert 0 < int(x) < int(y) and 0 < float(z) < 100
    off = re.findall(r"NIF evaluations: executed (\d+) of (\d+) escaped", log)
    assert off and all(x == y for x, y in off)
    assert "Samples/sec" in slog
