"""The step-scope sharing table from one step to the next: whatever a step leaves in the table -- after a reallocation, a
batch-scope step, a step with sharing off or a constant environment, a forced capacity or a failed step -- the next step-scope
step must not see it.  A key left by an earlier step would show twice: its paths would take the radiance of a store entry of
the wrong step (records differ from explicit off), and the step would evaluate fewer rows than it has distinct (u, v) pairs.
Today every step-scope step clears the table at its start; a clear moved to the end of the step before (tried in round 23 and
not kept) has to pass these sequences too.  64 x 48 pixels, 64 samples per step in two batches of 32
iterations, depth 8, AA scale 0.01 (tests/test_gpu_nif_sharing_auto.py), three good steps or more per sequence."""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
W, H, SPP, IPB, DEPTH, AA = 64, 48, 64, 32, 8, 0.01

# a sequence: one dict per pt_path_trace; mode: what set_nif_sharing gets ahead of it (None: no call), env: "nif" / "const" set
# ahead of it, spp: samples per step from here on, capacity: the test build's forced table capacity set ahead of it,
# fault: the batch whose NIF launch fails (the step raises; a fresh setup follows, as after any failed step)
SEQUENCES = {
    "default_throughout": [dict(), dict(), dict(), dict()],
    "step_batch_step": [dict(mode="step"), dict(mode="batch"), dict(mode="step"), dict()],
    "step_off_step": [dict(mode="step"), dict(mode="off"), dict(mode="step"), dict()],
    "step_const_nif": [dict(mode="step"), dict(env="const"), dict(env="nif"), dict()],
    "scope_grows": [dict(mode="step"), dict(spp=160), dict(), dict(spp=SPP)],
    "forced_capacity": [dict(mode="step"), dict(capacity=1 << 20), dict(), dict(capacity=0), dict()],
    "failed_step": [dict(mode="step"), dict(), dict(fault=1), dict(), dict()],
}
DIAG = {"forced_capacity", "failed_step"}


def _nif(r):
    r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())


def _run(P, seq, subject, diag=False):
    """The sequence on one handle: as written (subject) or with sharing explicitly off and neither capacity nor fault (the
    reference, which sets up afresh where the subject has to).  Returns the records after every good step, the resident film,
    and per good step (first sample, samples, sharing stats)."""
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB, diag=diag and subject)
    lib = P.load_library(diag=True) if diag and subject else None
    try:
        _nif(r)
        spp, cursor = SPP, 0
        r.init_render_settings(aa_noise_scale=AA, samples_per_step=spp)
        if not subject:
            r.set_nif_sharing("off")
        rec = P.worklist(W, H)
        r.setup(rec)
        records, steps = [], []
        for op in seq:
            if op.get("env") == "const":
                r.set_constant_env((0.5, 1.0, 2.0))
            elif op.get("env") == "nif":
                _nif(r)
            if "spp" in op:
                spp = op["spp"]
                r.init_render_settings(aa_noise_scale=AA, samples_per_step=spp)   # same seed: the sample sequence continues
            if subject and op.get("mode"):
                r.set_nif_sharing(op["mode"])
            if subject and "capacity" in op:
                assert lib.pt_diag_set_nif_share_capacity(r.handle, op["capacity"]) == 0
            if "fault" in op:
                if subject:
                    assert lib.pt_diag_inject_fault(r.handle, op["fault"]) == 0
                    with pytest.raises(P.PtError) as e:
                        r.path_trace()
                    assert "injected fault" in str(e.value)
                    assert lib.pt_diag_inject_fault(r.handle, -1) == 0
                    r.synchronize()
                rec = P.worklist(W, H)   # accumulators are undefined after a failure; the sample sequence has not advanced
                r.setup(rec)
                continue
            r.path_trace()
            steps.append((cursor, spp, r.nif_sharing_stats()))
            cursor += spp
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        return records, r.gather_hdr(W * H, P.HDR_FILM).tobytes(), steps
    finally:
        r.close()


@pytest.fixture(scope="module")
def distinct_pairs(ptmi_lib):
    """distinct(first, n): the distinct (u, v) bit pairs among the escaped paths of samples first .. first + n - 1 of every
    pixel, counted with numpy from pt_trace_paths (tests/test_gpu_nif_sharing_auto.py); every range is traced once."""
    P = ptmi_lib
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB)
    _nif(r)
    r.init_render_settings(aa_noise_scale=AA, samples_per_step=SPP)
    px = np.arange(W * H)
    known = {}

    def distinct(first, n):
        if (first, n) not in known:
            s = np.repeat(np.arange(first, first + n, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, n), np.tile(px // W, n), s)
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).view(np.uint32).reshape(-1, 2).astype(np.uint64)
            known[(first, n)] = (int(esc.sum()), np.unique((uv[:, 0] << np.uint64(32)) | uv[:, 1]).size)
        return known[(first, n)]

    yield distinct
    r.close()


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_sequence_equals_explicit_off_and_evaluates_the_distinct_pairs(ptmi_lib, distinct_pairs, name):
    seq = SEQUENCES[name]
    ref_records, ref_film, ref_steps = _run(ptmi_lib, seq, subject=False)
    records, film, steps = _run(ptmi_lib, seq, subject=True, diag=name in DIAG)
    assert len(records) == len(ref_records) >= 3
    for i, (a, b) in enumerate(zip(records, ref_records)):
        assert a == b, "records after good step %d differ from explicit off" % i
    assert film == ref_film, "resident film differs from explicit off"
    step_scope = 0
    for (first, n, st), (_, _, off) in zip(steps, ref_steps):
        print("%s: samples %d..%d %r" % (name, first, first + n - 1, st))
        assert off["mode"] == "off" and st["escaped"] == off["escaped"]
        if st["mode"] != "step":
            continue
        step_scope += 1
        escaped, distinct = distinct_pairs(first, n)
        assert st["escaped"] == escaped and st["overflowed"] == 0, st
        assert st["evaluations"] == distinct, (st, distinct)
    # what the sequence is there for really happened
    modes = [st["mode"] for _, _, st in steps]
    slots = [st["table_slots"] for _, _, st in steps]
    expect = {
        "default_throughout": ["step"] * 4,
        "step_batch_step": ["step", "batch", "step", "step"],
        "step_off_step": ["step", "off", "step", "step"],
        "step_const_nif": ["step", "off", "step", "step"],
        "scope_grows": ["step"] * 4,
        "forced_capacity": ["step"] * 5,
        "failed_step": ["step"] * 4,
    }[name]
    assert modes == expect and step_scope >= 3
    if name == "scope_grows":
        assert slots[1] > slots[0] and slots[2] == slots[3] == slots[1], slots   # reallocated once, kept afterwards
    if name == "forced_capacity":
        assert slots[1] == slots[2] == 1 << 20 and slots[0] != 1 << 20 and slots[3] == slots[4] != 1 << 20, slots
