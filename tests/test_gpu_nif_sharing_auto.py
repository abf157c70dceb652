"""The automatic default of NIF sharing: a handle on which pt_set_nif_sharing was never called shares at step scope when the
environment is a NIF and the memo is off, and renders the same bytes as an explicit off.  64 x 48 pixels, 64 samples per
step in two batches of 32 iterations, depth 8 throughout."""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
W, H, SPP, IPB, DEPTH = 64, 48, 64, 32, 8
DEFAULT = None   # `mode` of a handle that never calls set_nif_sharing
# AA noise scale (pixels) at which this small image shares: at the default 0.3 a 64-pixel-wide image jitters every camera ray
# over hundreds of binary16 values, and 99.7 % of a step's keys are distinct; at 0.01 the samples of a pixel share their ray.
FINE_AA = 0.01


def _render(P, mode, steps=3, env="nif", memo=0, capacity=None, aa_scales=None):
    """`steps` steps with the film resident; returns (records of every step, resident film, sharing stats and memo stats of
    every step).  aa_scales: the AA noise scale of every step (same seed, so the sample sequence continues)."""
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB, diag=capacity is not None)
    try:
        if env == "const":
            r.set_constant_env((0.5, 1.0, 2.0))
        elif env == "map":
            r.set_env_map(np.random.default_rng(7).random((8, 16, 3), dtype=np.float32) + np.float32(0.25))
        else:
            r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=SPP)
        if capacity is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_share_capacity(r.handle, capacity) == 0
        if memo:
            r.set_nif_memo(memo)
        if mode is not DEFAULT:
            r.set_nif_sharing(mode)
        rec = P.worklist(W, H)
        r.setup(rec)
        records, stats, memos = [], [], []
        for i in range(steps):
            if aa_scales is not None:
                r.init_render_settings(aa_noise_scale=aa_scales[i], samples_per_step=SPP)
            r.path_trace()
            stats.append(r.nif_sharing_stats())
            memos.append(r.nif_memo_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)
        return records, film.tobytes(), stats, memos
    finally:
        r.close()


@pytest.fixture(scope="module")
def off(ptmi_lib):
    return _render(ptmi_lib, "off")


@pytest.fixture(scope="module")
def default(ptmi_lib):
    return _render(ptmi_lib, DEFAULT)


@pytest.fixture(scope="module")
def off_fine(ptmi_lib):
    return _render(ptmi_lib, "off", aa_scales=[FINE_AA] * 3)


@pytest.fixture(scope="module")
def default_fine(ptmi_lib):
    return _render(ptmi_lib, DEFAULT, aa_scales=[FINE_AA] * 3)


@pytest.mark.parametrize("aa", ["default_aa", "fine_aa"])
def test_default_handle_renders_the_bytes_of_explicit_off(request, aa):
    off = request.getfixturevalue("off" if aa == "default_aa" else "off_fine")
    default = request.getfixturevalue("default" if aa == "default_aa" else "default_fine")
    assert len(default[0]) == 3
    for i, (a, b) in enumerate(zip(default[0], off[0])):
        assert a == b, "records of step %d differ" % i
    assert default[1] == off[1], "resident film differs"
    for s, o in zip(default[2], off[2]):
        assert s["mode"] == "step" and s["escaped"] == o["escaped"] and 0 < s["evaluations"] < s["escaped"], s
        assert s["table_slots"] > 0 and s["share_ms"] > 0.0 and s["overflowed"] == 0, s


def test_explicit_off_runs_no_sharing_pass(off):
    for s in off[2]:
        assert s["mode"] == "off" and s["evaluations"] == s["escaped"] > 0, s
        assert s["table_slots"] == 0 and s["share_ms"] == 0.0 and s["overflowed"] == 0, s


@pytest.mark.parametrize("aa", ["default_aa", "fine_aa"])
def test_default_evaluations_are_the_distinct_uv_bit_pairs(ptmi_lib, request, aa):
    """As tests/test_gpu_nif_sharing.py::test_evaluation_counts_are_the_distinct_uv_bit_pairs counts them: pt_trace_paths
    traces every (pixel, sample) of a step, numpy counts the distinct (u, v) bit pairs of its escaped paths -- for all three
    steps."""
    P = ptmi_lib
    default = request.getfixturevalue("default" if aa == "default_aa" else "default_fine")
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(aa_noise_scale=0.3 if aa == "default_aa" else FINE_AA, samples_per_step=SPP)
        px = np.arange(W * H)
        for step, st in enumerate(default[2]):
            s = np.repeat(np.arange(step * SPP, (step + 1) * SPP, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, SPP), np.tile(px // W, SPP), s)
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).view(np.uint32).reshape(-1, 2).astype(np.uint64)
            distinct = np.unique((uv[:, 0] << np.uint64(32)) | uv[:, 1]).size
            print("step %d: escaped %d, distinct %d, stats %r" % (step, int(esc.sum()), distinct, st))
            assert st["mode"] == "step" and st["escaped"] == int(esc.sum()) and st["overflowed"] == 0
            assert st["evaluations"] == distinct, (step, st, distinct)
    finally:
        r.close()


@pytest.mark.parametrize("env", ["const", "map"])
def test_constant_environment_and_environment_map_run_off(ptmi_lib, env):
    rec, film, stats, _ = _render(ptmi_lib, DEFAULT, steps=2, env=env)
    ref_rec, ref_film, ref_stats, _ = _render(ptmi_lib, "off", steps=2, env=env)
    assert rec == ref_rec and film == ref_film
    for s, o in zip(stats, ref_stats):
        assert s == o, (s, o)
        assert s["mode"] == "off" and s["table_slots"] == 0 and s["share_ms"] == 0.0 and s["escaped"] > 0
        assert s["evaluations"] == (0 if env == "const" else s["escaped"])


def test_memo_behaves_as_with_sharing_off(ptmi_lib, off):
    """With the memo on the automatic default stays out of the way: the sharing mode reads off, the memo's own passes run,
    and every count equals the one of a handle with an explicit off."""
    memo_bytes = 192 << 20   # 4 M slots for half a million keys: no key of the three steps overflows the memo
    rec, film, stats, memos = _render(ptmi_lib, DEFAULT, memo=memo_bytes)
    ref_rec, ref_film, ref_stats, ref_memos = _render(ptmi_lib, "off", memo=memo_bytes)
    assert rec == ref_rec == off[0] and film == ref_film == off[1]
    for s, o, m, n in zip(stats, ref_stats, memos, ref_memos):
        assert s["mode"] == "off" and s["table_slots"] == 0 and s["share_ms"] == 0.0
        for k in ("escaped", "evaluations", "overflowed"):
            assert s[k] == o[k], (k, s, o)
        for k in ("enabled", "slots", "occupied", "escaped", "served", "evaluations", "inserted", "overflowed", "generation",
                  "retains"):
            assert m[k] == n[k], (k, m, n)
        assert m["enabled"] and m["memo_ms"] > 0.0


def test_automatic_mode_stays_exact_with_a_16_slot_table(ptmi_lib, off):
    """The test build's forced capacity: nearly every key finds no slot and is evaluated alone; the film does not change."""
    rec, film, stats, _ = _render(ptmi_lib, DEFAULT, capacity=16)
    assert rec == off[0] and film == off[1]
    for s, o in zip(stats, off[2]):
        assert s["mode"] == "step" and s["table_slots"] == 16 and s["overflowed"] > 0
        assert s["escaped"] == o["escaped"] and s["evaluations"] <= s["escaped"]


def test_a_memo_call_ends_the_automatic_choice(ptmi_lib):
    """A handle whose caller has switched the memo on and off again runs the unshared step, as it did before the default
    became automatic (tests/test_gpu_nif_memo.py::test_set_and_clear_on_a_handle); pt_set_nif_sharing still switches it."""
    P = ptmi_lib
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(aa_noise_scale=FINE_AA, samples_per_step=SPP)
        r.setup(P.worklist(W, H))
        r.path_trace()
        first = r.nif_sharing_stats()
        assert first["mode"] == "step" and first["evaluations"] < first["escaped"]
        r.set_nif_memo(0)
        r.path_trace()
        s = r.nif_sharing_stats()
        assert s["mode"] == "off" and s["evaluations"] == s["escaped"] and s["table_slots"] == 0 and s["share_ms"] == 0.0
        r.set_nif_sharing("step")
        r.path_trace()
        s = r.nif_sharing_stats()
        assert s["mode"] == "step" and s["evaluations"] < s["escaped"]
    finally:
        r.close()
