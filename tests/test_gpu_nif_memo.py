"""Persistent memo of NIF evaluations across steps on the GPU (pt_set_nif_memo): every step renders the same bits as memo off,
while the keys found in the memo run no NIF row.  Compared against memo off and against step-scope sharing, step by step."""
import os
import re
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
META = nif_assets.URBAN_ALLEY_META
GIB = 1 << 30


def _render(P, W, H, layers=None, emb=12, memo=0, mode="off", depth=8, spp=12, steps=4, ipb=4, const=None, slots=None,
            rotation=0.0):
    """`steps` steps with the film resident; returns (records per step, resident film, memo stats per step, sharing stats
    per step)."""
    r = P.Renderer(W, H, max_path_length=depth, iterations_per_batch=ipb, diag=slots is not None)
    try:
        if const is not None:
            r.set_constant_env(const)
        else:
            r.init_nif_weights(layers, emb, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=spp, env_rotation_degrees=rotation)
        r.set_nif_sharing(mode)
        if memo:
            r.set_nif_memo(memo)
        if slots is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_memo_slots(r.handle, slots) == 0
        rec = P.worklist(W, H)
        r.setup(rec)
        records, mstats, sstats = [], [], []
        for _ in range(steps):
            r.path_trace()
            mstats.append(r.nif_memo_stats())
            sstats.append(r.nif_sharing_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM).tobytes()
        return records, film, mstats, sstats
    finally:
        r.close()


FAMILIES = ["fused_6x320", "narrow_3x64", "wide_8x1024", "float32", "mixed"]


def _family(name):
    if name == "fused_6x320":
        return nif_assets.synthetic_nif()
    if name == "narrow_3x64":
        return nif_assets.synthetic_nif(hidden=64, layer_count=3, seed=3)
    if name == "wide_8x1024":
        return nif_assets.synthetic_nif(hidden=1024, layer_count=8, seed=31)
    if name == "float32":
        return nif_assets.synthetic_nif(hidden=128, layer_count=3, seed=17, dtype=np.float32)
    f32 = nif_assets.synthetic_nif(hidden=64, layer_count=3, seed=5, dtype=np.float32)
    return [(k.astype(np.float16), b.astype(np.float16), relu) if i % 2 else (k, b, relu) for i, (k, b, relu) in enumerate(f32)]


@pytest.mark.parametrize("name", FAMILIES)
def test_every_kernel_family_is_bit_identical_over_several_steps(ptmi_lib, name):
    P, layers = ptmi_lib, _family(name)
    off_rec, off_film, off_m, _ = _render(P, 160, 120, layers)
    step_rec, step_film, _, step_s = _render(P, 160, 120, layers, mode="step")
    rec, film, mstats, sstats = _render(P, 160, 120, layers, memo=GIB)
    assert rec == off_rec and film == off_film and step_film == off_film
    for m in off_m:
        assert not m["enabled"] and m["served"] == 0 and m["evaluations"] == m["escaped"]
    occupied = 0
    for i, (m, s, st) in enumerate(zip(mstats, sstats, step_s)):
        assert m["enabled"] and m["slots"] > 0 and m["overflowed"] == 0 and m["retains"] == 0
        assert m["generation"] == mstats[0]["generation"]
        assert m["escaped"] == s["escaped"] == st["escaped"] and m["evaluations"] == s["evaluations"] == m["inserted"]
        assert m["memo_ms"] > 0 and s["share_ms"] == 0.0 and s["mode"] == "off"
        occupied += m["inserted"]
        assert m["occupied"] == occupied
        if i == 0:   # an empty memo is step-scope sharing
            assert m["served"] == 0 and m["evaluations"] == st["evaluations"]
        else:
            assert m["served"] > 0 and m["evaluations"] < st["evaluations"], (i, m, st)


def test_constant_environment_runs_no_memo_pass(ptmi_lib):
    off_rec, off_film, _, _ = _render(ptmi_lib, 96, 64, const=(0.5, 1.0, 2.0), depth=6, spp=8)
    rec, film, mstats, sstats = _render(ptmi_lib, 96, 64, const=(0.5, 1.0, 2.0), depth=6, spp=8, memo=GIB)
    assert rec == off_rec and film == off_film
    for m, s in zip(mstats, sstats):
        assert m["enabled"] and m["escaped"] > 0
        assert m["served"] == m["evaluations"] == m["inserted"] == m["occupied"] == m["overflowed"] == 0 and m["memo_ms"] == 0.0
        assert s["evaluations"] == 0


def test_full_size_c2_three_steps(ptmi_lib):
    P, layers = ptmi_lib, nif_assets.synthetic_nif()
    kw = dict(depth=8, spp=24, steps=3, ipb=0)
    off_rec, off_film, _, _ = _render(P, 1104, 1000, layers, **kw)
    _, _, _, step_s = _render(P, 1104, 1000, layers, mode="step", **kw)
    rec, film, mstats, _ = _render(P, 1104, 1000, layers, memo=16 * GIB, **kw)
    assert rec == off_rec and film == off_film
    ratio = mstats[2]["evaluations"] / step_s[2]["evaluations"]
    print("C2 shape, step 3: memo %d rows, step scope %d rows, ratio %.4f; served %d of %d escaped" % (
        mstats[2]["evaluations"], step_s[2]["evaluations"], ratio, mstats[2]["served"], mstats[2]["escaped"]))
    for i, m in enumerate(mstats):
        print("C2 shape, step %d: %s" % (i + 1, m))
    assert mstats[2]["evaluations"] < step_s[2]["evaluations"] and mstats[2]["served"] > 0


def test_hot_swap_invalidates_and_settings_do_not(ptmi_lib):
    """A NIF hot swap starts a new generation (served == 0, the step equals off with the new model); azimuth, fov, seed and
    pt_setup keep the generation and every step stays bit-identical to memo off."""
    P = ptmi_lib
    W, H = 96, 64
    A = nif_assets.synthetic_nif()
    B = nif_assets.synthetic_nif(hidden=128, layer_count=4, seed=77)
    mean = nif_assets.folded_mean()

    def sequence(memo):
        r = P.Renderer(W, H, max_path_length=7, iterations_per_batch=3)
        try:
            r.init_nif_weights(A, 12, META["max"], mean)
            r.init_render_settings(samples_per_step=9)
            if memo:
                r.set_nif_memo(memo)
            rec = P.worklist(W, H)
            r.setup(rec)
            out, stats = [], []
            for i in range(8):
                if i == 3:
                    r.init_nif_weights(B, 12, META["max"], mean)                                   # hot swap
                if i == 5:
                    r.init_render_settings(samples_per_step=9, env_rotation_degrees=120.0)          # azimuth
                if i == 6:
                    r.init_render_settings(samples_per_step=9, env_rotation_degrees=120.0, fov_degrees=60.0, seed=7)
                if i == 7:
                    rec = P.worklist(W, H)
                    r.setup(rec)                                                                    # a new worklist
                r.path_trace()
                stats.append(r.nif_memo_stats())
                r.read_results(rec)
                out.append(rec.tobytes())
                r.film_accumulate()
            out.append(r.gather_hdr(W * H, P.HDR_FILM).tobytes())
            return out, stats
        finally:
            r.close()

    ref, _ = sequence(0)
    got, stats = sequence(GIB)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a == b, "part %d differs" % i
    g0 = stats[0]["generation"]
    gens = [s["generation"] - g0 for s in stats]
    assert gens == [0, 0, 0, 1, 1, 1, 1, 1], gens
    assert stats[3]["served"] == 0 and stats[1]["served"] > 0 and stats[2]["served"] > 0 and stats[4]["served"] > 0
    assert stats[7]["served"] > 0   # pt_setup keeps the memo


def test_tiny_memo_overflows_and_retains_exactly(ptmi_lib):
    """A 256-slot memo (test build hook): keys overflow, occupancy passes 1/2 and retain passes run; the film does not change."""
    P, layers = ptmi_lib, nif_assets.synthetic_nif()
    kw = dict(depth=8, spp=16, steps=4, ipb=8)
    off_rec, off_film, _, _ = _render(P, 64, 48, layers, **kw)
    rec, film, mstats, _ = _render(P, 64, 48, layers, memo=GIB, slots=256, **kw)
    assert rec == off_rec and film == off_film
    assert all(m["slots"] == 256 and m["occupied"] <= 256 for m in mstats)
    assert sum(m["overflowed"] for m in mstats) > 0 and mstats[-1]["retains"] > 0
    assert all(m["evaluations"] <= m["escaped"] for m in mstats)


def test_failed_step_starts_a_new_generation(ptmi_lib):
    P = ptmi_lib
    W, H = 96, 64
    layers = nif_assets.synthetic_nif()

    def sequence(memo):
        r = P.Renderer(W, H, max_path_length=7, iterations_per_batch=3, diag=True)
        diag = P.load_library(diag=True)
        try:
            r.init_nif_weights(layers, 12, META["max"], nif_assets.folded_mean())
            r.init_render_settings(samples_per_step=9)
            if memo:
                r.set_nif_memo(memo)
            rec = P.worklist(W, H)
            r.setup(rec)
            out = []
            for _ in range(2):
                r.path_trace()
                r.read_results(rec)
                out.append(rec.tobytes())
            before = r.nif_memo_stats()
            assert diag.pt_diag_inject_fault(r.handle, 1) == 0   # 3 batches: batch 1 fails
            with pytest.raises(P.PtError) as e:
                r.path_trace()
            assert e.value.code == -3 and "injected fault" in str(e.value)
            assert diag.pt_diag_inject_fault(r.handle, -1) == 0
            after = r.nif_memo_stats()
            r.synchronize()
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            nxt = r.nif_memo_stats()
            r.read_results(rec)
            out.append(rec.tobytes())
            return out, before, after, nxt
        finally:
            r.close()

    ref, _, _, _ = sequence(0)
    got, before, after, nxt = sequence(GIB)
    assert got == ref
    assert before["served"] > 0 and after["generation"] == before["generation"] + 1
    assert nxt["generation"] == after["generation"] and nxt["served"] == 0


def test_calibrate_after_a_memo_step_leaves_the_next_step_alone(ptmi_lib):
    """pt_calibrate_nif after a step with the memo replays the distinct queue of the step's largest batch out of the step store:
    it reports that queue's length and a time, and the step after it equals the one of a handle that never calibrated --
    records and memo statistics (all but memo_ms, a device time).  6 iterations at 2 per batch are dealt 1 + 2 + 2 + 1, so the
    replayed batch is the third, in store region 2.  The forced memo (test build hook) has 2^16 slots: more than twice the
    13,824 paths of a step, so no key overflows and every count is decided by the keys alone."""
    P, layers = ptmi_lib, nif_assets.synthetic_nif()
    W = H = 48

    def two_steps(calibrate):
        r = P.Renderer(W, H, max_path_length=6, iterations_per_batch=2, diag=True)
        try:
            r.init_nif_weights(layers, 12, META["max"], nif_assets.folded_mean())
            r.init_render_settings(samples_per_step=6)
            assert P.load_library(diag=True).pt_diag_set_nif_memo_slots(r.handle, 1 << 16) == 0
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            first = r.nif_memo_stats()
            if calibrate:
                ms, evals = r.calibrate_nif(2)
                assert 0 < evals <= first["evaluations"] and ms > 0
            r.path_trace()
            second = r.nif_memo_stats()
            r.read_results(rec)
            return rec.tobytes(), [{k: v for k, v in m.items() if k != "memo_ms"} for m in (first, second)]
        finally:
            r.close()

    rec, stats = two_steps(True)
    ref_rec, ref_stats = two_steps(False)
    assert rec == ref_rec and stats == ref_stats
    assert stats[0]["enabled"] and stats[0]["slots"] == 1 << 16 and stats[0]["evaluations"] > 0 and stats[1]["served"] > 0


def test_memo_with_each_sharing_mode(ptmi_lib):
    P, layers = ptmi_lib, nif_assets.synthetic_nif()
    off_rec, off_film, _, _ = _render(P, 160, 120, layers, steps=3)
    runs = {mode: _render(P, 160, 120, layers, memo=GIB, mode=mode, steps=3) for mode in ("off", "batch", "step")}
    for mode, (rec, film, mstats, sstats) in runs.items():
        assert rec == off_rec and film == off_film, mode
        assert [s["mode"] for s in sstats] == [mode] * 3
        assert [m["evaluations"] for m in mstats] == [s["evaluations"] for s in sstats]
    # the memo decides the rows whatever the sharing mode says
    assert [m["evaluations"] for m in runs["off"][2]] == [m["evaluations"] for m in runs["step"][2]] == \
        [m["evaluations"] for m in runs["batch"][2]]


def test_set_and_clear_on_a_handle(ptmi_lib):
    P = ptmi_lib
    r = P.Renderer(64, 48, max_path_length=6)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=8)
        with pytest.raises(P.PtError) as e:
            r.set_nif_memo(1000)              # below one 48 KiB minimum
        assert e.value.code == -1 and not r.nif_memo_stats()["enabled"]
        r.set_nif_memo(48 * 1024)
        assert r.nif_memo_stats()["slots"] == 1024
        r.set_nif_memo(GIB)
        assert r.nif_memo_stats()["slots"] == 1 << 24
        rec = P.worklist(64, 48)
        r.setup(rec)
        r.path_trace()
        r.path_trace()
        s = r.nif_memo_stats()
        assert s["served"] > 0 and s["occupied"] > 0
        r.set_nif_memo(GIB)                   # same capacity: the entries stay
        assert r.nif_memo_stats()["occupied"] == s["occupied"]
        r.clear_nif_memo()
        c = r.nif_memo_stats()
        assert c["generation"] == s["generation"] + 1 and c["occupied"] == 0
        r.path_trace()
        assert r.nif_memo_stats()["served"] == 0
        r.set_nif_memo(0)
        r.path_trace()
        s = r.nif_memo_stats()
        assert not s["enabled"] and s["slots"] == 0 and s["evaluations"] == s["escaped"] and s["memo_ms"] == 0.0
    finally:
        r.close()


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
def test_cli_nif_memo_writes_the_same_exr(tmp_path, devices):
    plain, log = _run_cli(tmp_path, "plain", devices)
    memo, mlog = _run_cli(tmp_path, "memo", devices + ["--nif-memo-gib", "2"])
    assert memo == plain
    lines = re.findall(r"NIF memo: served (\d+) of (\d+) escaped, (\d+) rows executed", mlog)
    assert len(lines) == 2, mlog[-2000:]                         # save intervals at steps 2 and 3
    for x, y, z in lines:
        assert 0 < int(x) < int(y) and 0 < int(z) < int(y)
    assert "NIF memo:" not in log
