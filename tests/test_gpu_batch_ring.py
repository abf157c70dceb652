"""The ring of batch-buffer sets on the GPU: a step whose batches wrap the ring more than twice renders the bytes of the same
samples rendered one batch per step, in every mode that touches a set's buffers, owner map or store region.

64 x 48 pixels, the built-in scene, depth 8, the synthetic 6 x 320 NIF.  2 iterations per batch and 17 samples per step: a
NIF or map step is 1 + 8 batches (a short first one), a constant-environment step 8 + 1, so three sets are each used three
times and two sets more than four.  The expected values never come from the ring: the reference renders the same 17 samples
as nine steps of at most 2 samples -- one batch each, every one drained by the host's wait, no set used twice -- with sharing
off.  Per-pixel fp32 sums are in iteration order whatever the split, so records and the resident film are equal byte for
byte.  Two such steps, so the ring also starts over on sets the previous step has used."""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
W, H, DEPTH, IPB, SPP, STEPS = 64, 48, 8, 2, 17, 2
DEAL = (1, 2, 2, 2, 2, 2, 2, 2, 2)       # iterations of a NIF step's batches (ptmi_step_plan.h: batch_iterations)
CHUNKS = (2, 2, 2, 2, 2, 2, 2, 2, 1)     # the reference's single-batch steps
DEFAULT = None                           # `mode` of a handle that never calls set_nif_sharing
COARSE_AA, FINE_AA = 0.3, 0.01           # at 0.01 the samples of a pixel share their camera ray: many shared keys
MEMO_BYTES = 48 << 20                    # a million slots for 10^5 keys: nothing overflows, no retain pass


def _environment(r, env):
    if env == "const":
        r.set_constant_env((0.5, 1.0, 2.0))
    elif env == "map":
        r.set_env_map(np.random.default_rng(7).random((8, 16, 3), dtype=np.float32) + np.float32(0.25))
    else:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())


def _render(P, env, aa, mode, memo=0, capacity=None, chunks=(SPP,), diag=False):
    """STEPS times SPP samples, each SPP rendered as the steps `chunks`; returns (records after every SPP samples, resident
    film, per SPP samples: escaped summed over the chunks, sharing stats and memo stats of the last chunk, batches of every
    chunk)."""
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB, diag=diag or capacity is not None)
    try:
        _environment(r, env)
        r.init_render_settings(aa_noise_scale=aa, samples_per_step=chunks[0])
        if capacity is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_share_capacity(r.handle, capacity) == 0
        if memo:
            r.set_nif_memo(memo)
        if mode is not DEFAULT:
            r.set_nif_sharing(mode)
        rec = P.worklist(W, H)
        r.setup(rec)
        records, escaped, share, memos, launches = [], [], [], [], []
        for _ in range(STEPS):
            esc = 0
            for c in chunks:
                r.init_render_settings(aa_noise_scale=aa, samples_per_step=c)   # same seed: the sample sequence continues
                r.path_trace()
                esc += r.nif_sharing_stats()["escaped"]
                launches.append(r.stats().trace_launches)
            escaped.append(esc)
            share.append(r.nif_sharing_stats())
            memos.append(r.nif_memo_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM).tobytes()
        return records, film, escaped, share, memos, launches
    finally:
        r.close()


_references = {}


def _reference(P, env, aa):
    """One batch per step, sharing off: computed once per environment and AA scale, shared by the cases, never changed."""
    if (env, aa) not in _references:
        records, film, escaped, share, _, launches = _render(P, env, aa, "off", chunks=CHUNKS)
        assert launches == [1] * (STEPS * len(CHUNKS)), launches   # no step of the reference uses a set twice
        assert share[-1]["mode"] == "off"
        _references[(env, aa)] = (records, film, escaped)
    return _references[(env, aa)]


_keys = {}


def _iteration_keys(P, aa):
    """Per sample iteration of both steps: the (u, v) bit pairs of its escaped paths, from pt_trace_paths -- what a sharing
    table must find, counted with numpy."""
    if aa not in _keys:
        r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB)
        try:
            _environment(r, "nif")
            r.init_render_settings(aa_noise_scale=aa, samples_per_step=SPP)
            px = np.arange(W * H)
            out = []
            for s in range(STEPS * SPP):
                paths = r.trace_paths(px % W, px // W, np.full(W * H, s, dtype=np.uint32))
                esc = paths["escaped"] != 0
                uv = np.ascontiguousarray(paths["uv"][esc]).view(np.uint32).reshape(-1, 2).astype(np.uint64)
                out.append((uv[:, 0] << np.uint64(32)) | uv[:, 1])
            _keys[aa] = out
        finally:
            r.close()
    return _keys[aa]


def _distinct(keys):
    return np.unique(np.concatenate(keys)).size


def _per_batch_distinct(keys):
    total, first = 0, 0
    for n in DEAL:
        total += _distinct(keys[first:first + n])
        first += n
    return total


def _check_bytes(P, env, aa, got):
    ref_records, ref_film, ref_escaped = _reference(P, env, aa)
    records, film, escaped, share, memos, launches = got
    assert launches == [len(DEAL)] * STEPS, launches   # 1 + 8 batches (8 + 1 for a constant environment): the ring wraps
    for i, (a, b) in enumerate(zip(records, ref_records)):
        assert a == b, "records of step %d differ from the one-batch-per-step render" % i
    assert film == ref_film, "resident film differs from the one-batch-per-step render"
    assert escaped == ref_escaped
    return share, memos


CASES = {
    #                 env     aa         mode     expected mode
    "default":       ("nif", COARSE_AA, DEFAULT, "step"),
    "off":           ("nif", COARSE_AA, "off", "off"),
    "batch":         ("nif", COARSE_AA, "batch", "batch"),
    "step":          ("nif", COARSE_AA, "step", "step"),
    "default_fine":  ("nif", FINE_AA, DEFAULT, "step"),
    "batch_fine":    ("nif", FINE_AA, "batch", "batch"),
    "const":         ("const", COARSE_AA, DEFAULT, "off"),
    "map":           ("map", COARSE_AA, DEFAULT, "off"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_wrapping_step_renders_the_bytes_of_single_batch_steps(ptmi_lib, case):
    P = ptmi_lib
    env, aa, mode, ran = CASES[case]
    share, _ = _check_bytes(P, env, aa, _render(P, env, aa, mode))
    keys = _iteration_keys(P, aa) if env == "nif" else None
    for step, s in enumerate(share):
        assert s["mode"] == ran and s["overflowed"] == 0, s
        if env == "const":
            assert s["evaluations"] == 0 and s["escaped"] > 0 and s["share_ms"] == 0.0
            continue
        if ran == "off":
            assert s["evaluations"] == s["escaped"] > 0 and s["table_slots"] == 0 and s["share_ms"] == 0.0
            if env != "nif":
                continue
        mine = keys[step * SPP:(step + 1) * SPP]
        assert s["escaped"] == sum(k.size for k in mine)
        if ran == "step":     # the distinct (u, v) bit pairs of the step's escaped paths
            assert s["evaluations"] == _distinct(mine), (s, _distinct(mine))
        elif ran == "batch":  # ... of every batch
            assert s["evaluations"] == _per_batch_distinct(mine), (s, _per_batch_distinct(mine))
        if ran != "off":
            assert s["table_slots"] > 0 and s["share_ms"] > 0.0 and s["evaluations"] <= s["escaped"]
            if aa == FINE_AA:
                assert s["evaluations"] < s["escaped"], s   # this image shares


@pytest.mark.parametrize("aa", [COARSE_AA, FINE_AA], ids=["coarse", "fine"])
def test_wrapping_step_with_the_memo(ptmi_lib, aa):
    """The memo's lookup, expand and publish over the ring: an empty memo is step-scope sharing, and the second step evaluates
    exactly the keys the first has not left in the memo."""
    P = ptmi_lib
    share, memos = _check_bytes(P, "nif", aa, _render(P, "nif", aa, "off", memo=MEMO_BYTES))
    keys = _iteration_keys(P, aa)
    first, second = keys[:SPP], keys[SPP:]
    new_in_second = np.setdiff1d(np.concatenate(second), np.concatenate(first)).size
    for m, s, expect in zip(memos, share, (_distinct(first), new_in_second)):
        assert m["enabled"] and m["overflowed"] == 0 and m["retains"] == 0 and s["mode"] == "off" and s["share_ms"] == 0.0
        assert m["escaped"] == s["escaped"] and m["evaluations"] == s["evaluations"] == m["inserted"] == expect, (m, s, expect)
    assert memos[0]["served"] == 0 and memos[1]["occupied"] == _distinct(keys)
    if aa == FINE_AA:
        assert memos[1]["served"] > 0


@pytest.mark.parametrize("mode", ["batch", "step"])
def test_wrapping_step_with_a_16_slot_table(ptmi_lib, mode):
    """The test build's forced capacity: nearly every key finds no slot and is evaluated alone (the overflow path writes the
    set's owner map and its store region all the same); the bytes do not change."""
    P = ptmi_lib
    share, _ = _check_bytes(P, "nif", FINE_AA, _render(P, "nif", FINE_AA, mode, capacity=16))
    keys = _iteration_keys(P, FINE_AA)
    for step, s in enumerate(share):
        mine = keys[step * SPP:(step + 1) * SPP]
        floor = _distinct(mine) if mode == "step" else _per_batch_distinct(mine)
        assert s["mode"] == mode and s["table_slots"] == 16 and s["overflowed"] > 0
        assert floor <= s["evaluations"] <= s["escaped"] == sum(k.size for k in mine), (s, floor)


@pytest.mark.parametrize("mode", ["batch", "step"])
def test_profiling_build_with_two_sets_renders_the_same_bytes(ptmi_lib, mode, monkeypatch):
    """PTMI_BATCH_SETS=2, read once per handle by the profiling build: the ring of depth 2 -- sets, owner maps and batch-scope
    store regions alternate -- against the same reference."""
    P = ptmi_lib
    monkeypatch.setenv("PTMI_BATCH_SETS", "2")
    got = _render(P, "nif", FINE_AA, mode, diag=True)
    monkeypatch.delenv("PTMI_BATCH_SETS")
    share, _ = _check_bytes(P, "nif", FINE_AA, got)
    keys = _iteration_keys(P, FINE_AA)
    for step, s in enumerate(share):
        mine = keys[step * SPP:(step + 1) * SPP]
        assert s["mode"] == mode and s["overflowed"] == 0
        assert s["evaluations"] == (_distinct(mine) if mode == "step" else _per_batch_distinct(mine)), s
