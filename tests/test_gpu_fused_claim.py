"""The fused step on the GPU (csrc/pt_nif_group.h: ShareClassTable, share_class_claim / share_class_resolve / share_class_expand):
the class is claimed inside S(b), the owner words are class-store indices and E(b) gathers from the class store.

1. pt_diag_share_class_claim over hand-built queues, with numpy as the judge: every final owner is the row of a class-queue
   entry of its own class, the raw appends are the distinct raw pairs (plus the overflows), the class queue is as long as the
   classes are many (plus the rows alone), both queues are dense and no class-queue index lies beyond its length.
2. Renders at the sizes of tests/test_gpu_nif_classes.py: records and resident film are the bytes of explicit off, `evaluations`
   stays the distinct raw pairs and `mlp_rows` the classes, in the modes that run the fused step (step scope, chosen or automatic)
   and in batch scope (which keeps the level's own passes), with forced tiny tables, new weights, pt_calibrate_nif, the memo and
   an environment map in between."""
import ctypes as C

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests.class_key_model import class_key

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
TAGGED = 0x80000000
TILE = 2048
LENGTHS = (1, 2047, 2048, 2049, 3 * 2048 + 5)
BIG = 1 << 14
TABLES = {"big": (BIG, BIG), "raw16": (16, BIG), "class4": (BIG, 4), "tiny": (16, 4)}


def _f(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _ulps(x, d):
    return (np.asarray(x, dtype=np.float32).view(np.int32) + np.int32(d)).view(np.float32)


def _raw(u, v):
    return (u.view(np.uint32).astype(np.uint64) << np.uint64(32)) | v.view(np.uint32)


def _queue(content, n):
    """n entries: `equal`, `distinct` (every entry a class of its own) or `mixed` (each raw pair several times, several raw pairs
    per class, a coordinate equal to 1.0 -- a raw-bits class -- and the tables' empty marker as a key)."""
    i = np.arange(n)
    if content == "equal":
        return np.full(n, 0.3, np.float32), np.full(n, 0.7, np.float32)
    if content == "distinct":    # a grid of step 1/256: x moves by 1/128 from entry to entry, far more than a half's ulp
        return (0.25 + (i % 96) / 256.0).astype(np.float32), (0.25 + (i // 96) / 256.0).astype(np.float32)
    rng = np.random.default_rng(5)
    m = max(1, n // 6)           # classes
    cu, cv = rng.random(m, dtype=np.float32) * 0.9 + 0.05, rng.random(m, dtype=np.float32) * 0.9 + 0.05
    pick, moved = rng.integers(0, m, n), rng.integers(0, 3, n)
    u, v = _ulps(cu[pick], moved), _ulps(cv[pick], -moved)
    same = class_key(u, v) == class_key(cu[pick], cv[pick])
    u, v = np.where(same, u, cu[pick]), np.where(same, v, cv[pick])
    if n > 64:
        u[5:n:97] = 1.0                                    # x = 0: the class is the coordinate's own bits
        u[7:n:193], v[7:n:193] = 1.0, 1.0
        u[11:n:389], v[11:n:389] = _f(0xFFFFFFFF), _f(0xFFFFFFFF)   # the empty marker: alone at both levels
    if n > TILE:
        u[TILE - 1:TILE + 1] = [0.4, _ulps(0.4, 3)]        # one class, two raw pairs, two claim tiles
        v[TILE - 1:TILE + 1] = [0.2, _ulps(0.2, -3)]
    return np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)


@pytest.fixture(scope="module")
def diag(ptmi_lib):
    r = ptmi_lib.Renderer(64, 64, max_path_length=4, diag=True)
    yield ptmi_lib.load_library(diag=True), r
    r.close()


def _fused(diag, u, v, counts, region_cap, raw_slots, class_slots):
    lib, r = diag
    counts = np.ascontiguousarray(counts, np.uint32)
    n = counts.size * region_cap
    assert u.size == v.size == n
    owner = np.zeros(n, np.uint32)
    d_u, d_v, c_u, c_v = (np.zeros(n, np.float32) for _ in range(4))
    ctr = np.zeros(4, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.pt_diag_share_class_claim(r.handle, ptr(u), ptr(v), ptr(counts), counts.size, region_cap, raw_slots, class_slots,
                                       ptr(owner), ptr(d_u), ptr(d_v), ptr(c_u), ptr(c_v), ptr(ctr))
    assert rc == 0, rc
    return owner, d_u, d_v, c_u, c_v, [int(x) for x in ctr]


def _check(diag, content, length, tables, empty_first):
    raw_slots, class_slots = TABLES[tables]
    cap = length + 3                                       # (slots above the count hold rubbish the passes must not read as live)
    lu, lv = _queue(content, length)
    u, v = np.full(2 * cap, np.float32(0.123)), np.full(2 * cap, np.float32(0.456))
    at = cap if empty_first else 0
    u[at:at + length], v[at:at + length] = lu, lv
    counts = [0, length] if empty_first else [length, 0]
    owner, d_u, d_v, c_u, c_v, (n_d, over, n_c, alone) = _fused(diag, u, v, counts, cap, raw_slots, class_slots)
    owner = owner[at:at + length]
    raw, keys = _raw(lu, lv), class_key(lu, lv)
    pairs, classes = np.unique(raw), np.unique(keys)
    print(content, length, tables, "pairs", pairs.size, "classes", classes.size, "distinct", n_d, "over", over, "rows", n_c, "alone", alone)
    assert 0 < n_c <= n_d <= length
    # every final owner is the row of a class-queue entry with the same class_key; no index beyond the length, none unused
    assert not (owner & TAGGED).any(), "an owner word is not a class-store index after resolve"
    assert int(owner.max()) < n_c
    q_keys = class_key(c_u[:n_c], c_v[:n_c])
    assert np.array_equal(q_keys[owner], keys), "an owner word points at a row of another class"
    assert np.array_equal(np.unique(owner), np.arange(n_c)), "a class-queue index is unused"
    # both queues are dense: rows of the queue itself, bit for bit; every pair and every class is there
    d_raw, c_raw = _raw(d_u[:n_d], d_v[:n_d]), _raw(c_u[:n_c], c_v[:n_c])
    assert np.isin(d_raw, raw).all() and np.isin(c_raw, d_raw).all()
    assert np.array_equal(np.unique(d_raw), pairs) and np.array_equal(np.unique(q_keys), classes)
    # the raw appends: a row per distinct pair, and the overflows; the class queue: a row per class, and the rows alone
    n_marker = int((raw == EMPTY).sum())
    assert n_d - np.unique(d_raw[d_raw != EMPTY]).size - n_marker <= over - n_marker and over >= n_marker
    assert alone >= int((class_key(d_u[:n_d], d_v[:n_d]) == EMPTY).sum())
    assert n_c - classes.size <= alone
    if raw_slots == BIG:
        assert over == n_marker and n_d == pairs.size - int(n_marker > 0) + n_marker      # the distinct raw pairs
    elif pairs.size > raw_slots:
        assert over > n_marker
    if class_slots == BIG:
        assert alone == int((class_key(d_u[:n_d], d_v[:n_d]) == EMPTY).sum())
        assert n_c == classes.size - int(EMPTY in classes) + alone                        # the distinct classes, plus the rows alone
    elif classes.size > class_slots:
        assert alone > 0
    if content == "equal":
        assert n_d == n_c == 1
    if content == "distinct":
        assert n_c == classes.size == length or class_slots != BIG
    if content == "mixed" and length > TILE and tables == "big":
        assert classes.size < pairs.size < length and n_marker > 0 and alone == n_marker


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("content", ("mixed", "equal", "distinct"))
def test_fused_claim_and_resolve_against_numpy(diag, content, length):
    _check(diag, content, length, "big", empty_first=length % 2 == 0)


@pytest.mark.parametrize("tables", ("raw16", "class4", "tiny"))
@pytest.mark.parametrize("content", ("mixed", "distinct"))
def test_fused_claim_with_tiny_tables(diag, content, tables):
    _check(diag, content, LENGTHS[-1], tables, empty_first=False)
    _check(diag, content, TILE + 1, tables, empty_first=True)


# ---- renders
W, H, DEPTH, STEPS, SPP = 64, 48, 8, 3, 17
AA_SCALES = {"aa_0.3": 0.3, "aa_0.01": 0.01}
MEMO_BYTES = 192 << 20
MODES = {"default": (None, "step"), "step": ("step", "step"), "batch": ("batch", "batch")}


def _nif(r, seed=2024):
    r.init_nif_weights(nif_assets.synthetic_nif(seed=seed), 12, META["max"], nif_assets.folded_mean())


def _env_map():
    rng = np.random.default_rng(3)
    return (rng.random((16, 32, 3), dtype=np.float32) * 2.0).astype(np.float32)


def _render(P, aa, plan, ipb=2, raw_slots=None, class_slots=None):
    """One step per entry of `plan` with the film resident.  An entry is a sharing mode (None: the handle's own choice, set once,
    ahead of the first step) or "off"/"step"/"batch" ahead of that step, with an optional suffix: "+memo" (the memo on for that
    step alone), "+map" (an environment map for that step alone), "+weights" (another model from that step on), "+calibrate"
    (pt_calibrate_nif behind that step).  Returns (records per step, film, sharing stats, class stats, calibrations)."""
    diag = raw_slots is not None or class_slots is not None
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=ipb, diag=diag)
    try:
        _nif(r)
        r.init_render_settings(aa_noise_scale=aa, samples_per_step=SPP)
        lib = P.load_library(diag=True) if diag else None
        if raw_slots is not None:
            assert lib.pt_diag_set_nif_share_capacity(r.handle, raw_slots) == 0
        if class_slots is not None:
            assert lib.pt_diag_set_nif_class_capacity(r.handle, class_slots) == 0
        rec = P.worklist(W, H)
        r.setup(rec)
        records, stats, classes, calibrated = [], [], [], []
        memo_on = map_on = False
        for i, entry in enumerate(plan):
            mode, _, extra = (entry or "").partition("+")
            if mode:
                r.set_nif_sharing(mode)
            if (extra == "memo") != memo_on:
                memo_on = extra == "memo"
                r.set_nif_memo(MEMO_BYTES if memo_on else 0)
            if extra == "map":
                r.set_env_map(_env_map())
                map_on = True
            elif map_on:
                _nif(r)
                map_on = False
            if extra == "weights":
                _nif(r, seed=77)
            r.path_trace()
            stats.append(r.nif_sharing_stats())
            classes.append(r.nif_class_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
            if extra == "calibrate":
                calibrated.append(r.calibrate_nif(2)[1])
        return records, r.gather_hdr(W * H, P.HDR_FILM).tobytes(), stats, classes, calibrated
    finally:
        r.close()


@pytest.fixture(scope="module")
def off(ptmi_lib):
    """off(aa, plan, ipb): the same plan with sharing explicitly off in every step, rendered once per case and left unchanged."""
    known = {}

    def get(aa, plan=(None,) * STEPS, ipb=2):
        plan_off = tuple("off" + ("+" + (e or "").partition("+")[2] if "+" in (e or "") else "") for e in plan)
        plan_off = tuple(e.replace("+memo", "").replace("+calibrate", "") for e in plan_off)
        if (aa, plan_off, ipb) not in known:
            known[(aa, plan_off, ipb)] = _render(ptmi_lib, AA_SCALES[aa], plan_off, ipb=ipb)
        return known[(aa, plan_off, ipb)]

    return get


@pytest.fixture(scope="module")
def counted(ptmi_lib):
    """counted(aa, step): (escaped paths, distinct raw pairs, distinct class keys) of a step, with numpy from pt_trace_paths.
    counted.new_pairs(aa, step, first, n): the distinct raw pairs of the step's iterations [first, first + n) that none of its
    iterations [0, first) has -- the distinct queue of a step-scope batch of those iterations."""
    P = ptmi_lib
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=32)
    _nif(r)
    px = np.arange(W * H)
    known, samples = {}, {}

    def get(aa, step):
        if (aa, step) not in known:
            r.init_render_settings(aa_noise_scale=AA_SCALES[aa], samples_per_step=SPP)
            s = np.repeat(np.arange(step * SPP, (step + 1) * SPP, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, SPP), np.tile(px // W, SPP), s)   # iteration-major: SPP runs of W x H pixels
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).reshape(-1, 2)
            raw = _raw(uv[:, 0].copy(), uv[:, 1].copy())
            ends = np.cumsum(esc.reshape(SPP, W * H).sum(axis=1))
            keys = class_key(uv[:, 0].copy(), uv[:, 1].copy())
            samples[(aa, step)] = (np.split(raw, ends[:-1]), np.split(keys, ends[:-1]))
            known[(aa, step)] = (int(esc.sum()), np.unique(raw).size, np.unique(keys).size)
        return known[(aa, step)]

    def new_in(per, first, n):
        batch = np.unique(np.concatenate(per[first:first + n]))
        return int(batch.size - np.isin(batch, np.concatenate(per[:first])).sum()) if first else int(batch.size)

    def new_pairs(aa, step, first, n):
        get(aa, step)
        return new_in(samples[(aa, step)][0], first, n)

    def new_classes(aa, step, first, n):   # ... and the same of the class keys: the batch's class queue
        get(aa, step)
        return new_in(samples[(aa, step)][1], first, n)

    get.new_pairs, get.new_classes = new_pairs, new_classes
    yield get
    r.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("aa", sorted(AA_SCALES))
def test_fused_step_renders_the_bytes_of_explicit_off(ptmi_lib, off, counted, aa, mode):
    """Nine batches a step: the ring of three buffer sets wraps."""
    sharing, reported = MODES[mode]
    ref_records, ref_film, _, _, _ = off(aa)
    records, film, stats, classes, _ = _render(ptmi_lib, AA_SCALES[aa], (sharing,) + (None,) * (STEPS - 1))
    assert records == ref_records, "records differ from explicit off"
    assert film == ref_film, "resident film differs from explicit off"
    for i, (st, cl) in enumerate(zip(stats, classes)):
        escaped, distinct, n_classes = counted(aa, i)
        print("%s %s step %d: %r %r; numpy: escaped %d distinct %d classes %d" % (aa, mode, i, st, cl, escaped, distinct, n_classes))
        assert st["mode"] == reported and st["escaped"] == escaped and st["share_ms"] > 0.0
        assert st["overflowed"] == 0 and cl["ran"] and cl["alone"] == 0
        assert (cl["class_ms"] == 0.0) == (reported == "step"), "step scope claims the class in its sharing passes; batch scope does not"
        assert cl["mlp_rows"] == n_classes
        if reported == "step":
            assert st["evaluations"] == distinct
        else:
            assert distinct <= st["evaluations"] <= escaped


def test_two_batches_a_step(ptmi_lib, off, counted):
    """17 iterations in batches of 9 and 8.  pt_calibrate_nif behind the second step replays the larger batch, the first: its
    distinct queue is the step's first batch's, so it holds the distinct raw pairs of the step's first nine iterations -- not
    the batch's classes, over which the fused N(b) ran, and not the step's pairs."""
    plan = (None, "+calibrate", None)
    ref_records, ref_film, _, _, _ = off("aa_0.3", plan, ipb=9)
    records, film, stats, classes, calibrated = _render(ptmi_lib, AA_SCALES["aa_0.3"], plan, ipb=9)
    assert records == ref_records and film == ref_film
    for i, (st, cl) in enumerate(zip(stats, classes)):
        _, distinct, n_classes = counted("aa_0.3", i)
        assert st["mode"] == "step" and st["evaluations"] == distinct and cl["mlp_rows"] == n_classes
    first_batch, its_classes = counted.new_pairs("aa_0.3", 1, 0, 9), counted.new_classes("aa_0.3", 1, 0, 9)
    print("calibrated", calibrated, "first batch", first_batch, "its classes", its_classes, "step", stats[1]["evaluations"])
    assert its_classes < first_batch < stats[1]["evaluations"]   # (the counts a replay could report instead differ from it)
    assert calibrated == [first_batch]


@pytest.mark.parametrize("tables", ("raw16", "class16"))
def test_forced_tiny_tables_stay_exact(ptmi_lib, off, tables):
    ref_records, ref_film, ref_stats, _, _ = off("aa_0.3")
    kw = dict(raw_slots=16) if tables == "raw16" else dict(class_slots=16)
    records, film, stats, classes, _ = _render(ptmi_lib, AA_SCALES["aa_0.3"], ("step",) + (None,) * (STEPS - 1), **kw)
    assert records == ref_records and film == ref_film
    for st, cl, o in zip(stats, classes, ref_stats):
        print(st, cl)
        assert st["mode"] == "step" and cl["ran"] and st["escaped"] == o["escaped"]
        if tables == "raw16":
            assert st["table_slots"] == 16 and st["overflowed"] > 0
        else:
            assert cl["table_slots"] == 16 and cl["alone"] > 0


def test_new_weights_calibration_memo_and_map_between_fused_steps(ptmi_lib, off, counted):
    """One handle: a fused step, pt_calibrate_nif behind it, another model, a memo step, a fused step, a memo step (over a raw
    table whose values the fused step filled with class-store indices), a step with an environment map (the raw-only path: no
    class level), a fused step."""
    plan = (None, "+calibrate", "+weights", "+memo", "step", "+memo", "+map", None)   # (pt_set_nif_memo ends the handle's own choice: off)
    ref_records, ref_film, _, _, _ = off("aa_0.3", plan)
    records, film, stats, classes, calibrated = _render(ptmi_lib, AA_SCALES["aa_0.3"], plan)
    for i, (a, b) in enumerate(zip(records, ref_records)):
        assert a == b, "records of step %d differ from explicit off" % i
    assert film == ref_film
    print(stats, classes, calibrated)
    assert [st["mode"] for st in stats] == ["step", "step", "step", "off", "step", "step", "step", "step"]
    assert [bool(cl["ran"]) for cl in classes] == [True, True, True, True, True, True, False, True]
    assert [cl["class_ms"] == 0.0 for cl in classes] == [True, True, True, False, True, False, True, True], \
        "the memo's steps run the level's own passes, the fused steps and the step without the level none"
    assert classes[6]["mlp_rows"] == stats[6]["evaluations"] and stats[6]["table_slots"] > 0
    _, distinct, n_classes = counted("aa_0.3", 1)
    assert stats[1]["evaluations"] == distinct and classes[1]["mlp_rows"] == n_classes
    # pt_calibrate_nif replays the distinct queue of the largest batch, the earliest buffer set among equals.  17 iterations in
    # batches of IPB = 2 are dealt 1, 2, 2, 2, 2, 2, 2, 2, 2 (ptmi_step_plan.h: batch_iterations) over three sets, which hold
    # batches 6, 7 and 8 when the step ends: batch 6, iterations 11 and 12.  Its step-scope distinct queue is the raw pairs of
    # those two that no earlier iteration of the step has.
    replayed = counted.new_pairs("aa_0.3", 1, 11, 2)
    print("calibrated", calibrated, "batch 6", replayed)
    assert calibrated == [replayed]
