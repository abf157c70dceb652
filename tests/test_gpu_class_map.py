"""The mapped step on the GPU (csrc/pt_nif_group.h: ClassMap, class_map_claim / share_raw_claim / class_map_expand /
class_map_release; csrc/ptmi_share_plan.h: the class map): a step-scope step indexes its classes directly in a map of one word
per class, runs no resolve pass, counts raw pairs in a pass nothing waits for, and releases the words it took at its end.

1. pt_diag_class_map_claim over hand-built queues, with numpy as the judge: every entry ends at the row of its class, the class
   queue is as long as the classes are many plus the rows alone, a word is taken per class and none is left after the release;
   a second launch finds rows, and a launch behind a release gives the first launch's counts.
2. The raw-pair pass alone (pt_diag_claim_resolve, memo = 2) over the queues of tests/test_gpu_claim_tile.py: the distinct queue
   and the counts are share_claim_kernel's, and the owner map keeps its fill.
3. Renders at the sizes of tests/test_gpu_share_expand.py with 2, 4 and 9 batches a step: records and film are the bytes of
   explicit off and the counts are numpy's in three consecutive steps; with the map declined by a forced class capacity; across
   pt_upload_nif."""
import ctypes as C

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import test_gpu_claim_tile as tile
from tests.class_key_model import class_coord, class_key

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
TAGGED, PENDING, SLOT_BITS = 0x80000000, 0xC0000000, 0x3FFFFFFF
MIN_MAG, MAX_MAG = 0x38800000, 0x40000000
AXIS = ((MAX_MAG - MIN_MAG) >> 13) + 1
MAP_WORDS = AXIS * AXIS
COUNTS = np.array([1, 0, 2047, 2048, 0, 2049], dtype=np.uint32)   # an empty region between live ones, twice
CAP = 2049 + 3                                                    # no multiple of the tile
BIG_TAIL = 1 << 12


def _f(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _axis(coord):
    """numpy's class_axis_index: the axis index of a regular coordinate, -1 of an irregular one."""
    c = class_coord(coord).astype(np.int64)
    mag = c & 0x7FFFFFFF
    regular = ((c >> 31) == 1) & ((c & 0x1FFF) == 0) & (mag >= MIN_MAG) & (mag <= MAX_MAG)
    return np.where(regular, (mag - MIN_MAG) >> 13, -1)


def _map_index(u, v):
    iu, iv = _axis(u), _axis(v)
    return np.where((iu < 0) | (iv < 0), -1, iu * AXIS + iv)


def test_the_numpy_model_of_the_index():
    assert AXIS == 15361 and MAP_WORDS == 235960321
    u = np.array([0.0, 1.0 - 2.0 ** -15, 1.0, 1.5, np.nan, 0.5, -0.0], np.float32)
    assert list(_axis(u)) == [15360, 0, -1, -1, -1, (0x3F800000 - MIN_MAG) >> 13, 15360]


def _queue(content, n):
    """n live entries.  `equal`: one class; `distinct`: every entry a class of its own; `mixed`: each class several times over,
    as several floats, with u = 1, NaN, a coordinate above 1 and the tables' empty marker mixed in; `irregular`: 12 irregular
    classes, each as many times as the others (with a 4-slot tail: 4 find a slot, whichever they are)."""
    i = np.arange(n)
    if content == "equal":
        return np.full(n, 0.3, np.float32), np.full(n, 0.7, np.float32)
    if content == "distinct":
        return (0.25 + (i % 96) / 256.0).astype(np.float32), (0.25 + (i // 96) / 256.0).astype(np.float32)
    if content == "irregular":
        j = (i % 12).astype(np.float32)
        return np.full(n, 1.0, np.float32), (0.1 + j / 16.0).astype(np.float32)
    rng = np.random.default_rng(11)
    m = max(1, n // 6)
    cu, cv = rng.random(m, dtype=np.float32) * 0.9 + 0.05, rng.random(m, dtype=np.float32) * 0.9 + 0.05
    pick, moved = rng.integers(0, m, n), rng.integers(0, 3, n)
    u = (cu[pick].view(np.int32) + moved.astype(np.int32)).view(np.float32)
    v = (cv[pick].view(np.int32) - moved.astype(np.int32)).view(np.float32)
    same = class_key(u, v) == class_key(cu[pick], cv[pick])
    u, v = np.where(same, u, cu[pick]), np.where(same, v, cv[pick])
    if n > 64:
        u[5:n:97] = 1.0                                    # x = 0
        u[7:n:193], v[7:n:193] = 1.0, 1.0
        v[9:n:211] = np.nan
        u[10:n:223] = 1.25                                 # x > 0
        u[11:n:389], v[11:n:389] = _f(0xFFFFFFFF), _f(0xFFFFFFFF)   # the empty marker: alone
        v[13:n:401] = np.float32(1.0 - 2.0 ** -17)         # |x| < 2^-14
    return np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)


@pytest.fixture(scope="module")
def diag(ptmi_lib):
    r = ptmi_lib.Renderer(64, 64, max_path_length=4, diag=True)
    yield ptmi_lib.load_library(diag=True), r
    r.close()


def _claim(diag, u, v, counts, cap, tail_slots, launches=1, release_between=0):
    lib, r = diag
    counts = np.ascontiguousarray(counts, np.uint32)
    n = counts.size * cap
    assert u.size == v.size == n
    owner, rows = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    c_u, c_v = np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32)
    ctr = np.zeros(4, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.pt_diag_class_map_claim(r.handle, ptr(u), ptr(v), ptr(counts), counts.size, cap, tail_slots, launches, release_between,
                                     ptr(owner), ptr(rows), ptr(c_u), ptr(c_v), ptr(ctr))
    assert rc == 0, rc
    return owner, rows, c_u, c_v, [int(x) for x in ctr]


def _laid_out(content, counts=COUNTS, cap=CAP):
    """The queue of `content` dealt over the regions; the slots above a region's count hold a class no live entry has."""
    lu, lv = _queue(content, int(counts.sum()))
    u, v = np.full(counts.size * cap, np.float32(0.9123)), np.full(counts.size * cap, np.float32(0.0456))
    live = (np.arange(counts.size * cap) % cap) < np.repeat(counts, cap)
    u[live], v[live] = lu, lv
    return u, v, live


def _check(u, v, live, tail_slots, owner, rows, c_u, c_v, n_c, alone, taken, left, earlier_alone=0):
    """What C and E's hop leave; earlier_alone: rows an earlier launch over the same queue appended for its entries alone."""
    lu, lv, o, r = u[live], v[live], owner[live], rows[live]
    keys, index = class_key(lu, lv), _map_index(lu, lv)
    classes = np.unique(keys)
    print("entries", keys.size, "classes", classes.size, "irregular", int((index < 0).sum()), "rows", n_c, "alone", alone, "taken", taken, "left", left)
    assert not (r & TAGGED).any() and int(r.max()) < n_c, "an entry does not end at a row"
    q_keys = class_key(c_u[:n_c], c_v[:n_c])
    assert np.array_equal(q_keys[r], keys), "an entry ends at a row of another class"
    assert np.array_equal(np.unique(q_keys), classes)
    # an owner word is the row itself or a pending class word that names the entry's slot
    pending = (o & TAGGED) != 0
    assert np.array_equal(o[~pending], r[~pending]) and not ((o[pending] & PENDING) == PENDING).any()
    slot = (o[pending] & SLOT_BITS).astype(np.int64)
    regular = index[pending] >= 0
    assert np.array_equal(slot[regular], index[pending][regular])
    assert ((slot[~regular] >= MAP_WORDS) & (slot[~regular] < MAP_WORDS + tail_slots)).all()
    # rows: a row per class that holds a word, and a row per entry evaluated alone; the empty marker is always alone
    n_marker = int((keys == EMPTY).sum())
    assert alone >= n_marker and taken == n_c - alone and left == 0
    assert np.array_equal(np.unique(r).size, n_c - earlier_alone)
    irregular = np.unique(keys[(index < 0) & (keys != EMPTY)])
    if irregular.size <= tail_slots // 2:
        assert alone - earlier_alone == n_marker and taken == classes.size - int(n_marker > 0)
    return classes.size, n_marker


@pytest.mark.parametrize("content", ("mixed", "equal", "distinct"))
def test_class_claim_against_numpy(diag, content):
    u, v, live = _laid_out(content)
    owner, rows, c_u, c_v, (n_c, alone, taken, left) = _claim(diag, u, v, COUNTS, CAP, BIG_TAIL)
    n_classes, n_marker = _check(u, v, live, BIG_TAIL, owner, rows, c_u, c_v, n_c, alone, taken, left)
    assert n_c == n_classes - int(n_marker > 0) + n_marker
    if content == "equal":
        assert n_c == 1 and taken == 1
    if content == "distinct":
        assert n_c == int(COUNTS.sum())
    if content == "mixed":
        assert n_marker > 0 and n_classes < int(COUNTS.sum()) // 4


def test_all_regions_empty(diag):
    u, v, _ = _laid_out("mixed")
    _, _, _, _, ctr = _claim(diag, u, v, np.zeros_like(COUNTS), CAP, BIG_TAIL)
    assert ctr == [0, 0, 0, 0]


def test_a_four_slot_tail_fills(diag):
    """12 irregular classes of equally many entries each: 4 find a slot, the entries of the other 8 are evaluated alone."""
    counts = np.array([2048 * 3, 0, 12 * 100], dtype=np.uint32)
    u, v, live = _laid_out("irregular", counts, 2048 * 3 + 1)
    per_class = int(counts.sum()) // 12
    owner, rows, c_u, c_v, (n_c, alone, taken, left) = _claim(diag, u, v, counts, 2048 * 3 + 1, 4)
    _check(u, v, live, 4, owner, rows, c_u, c_v, n_c, alone, taken, left)
    assert alone == 8 * per_class and taken == 4 and n_c == 4 + alone
    # ... and mixed into regular entries
    u, v, live = _laid_out("mixed")
    owner, rows, c_u, c_v, (n_c, alone, taken, left) = _claim(diag, u, v, COUNTS, CAP, 4)
    _check(u, v, live, 4, owner, rows, c_u, c_v, n_c, alone, taken, left)
    keys, index = class_key(u[live], v[live]), _map_index(u[live], v[live])
    n_irregular = np.unique(keys[(index < 0) & (keys != EMPTY)]).size
    assert n_irregular > 4 and taken == np.unique(keys[index >= 0]).size + 4


@pytest.mark.parametrize("content", ("mixed", "equal"))
def test_a_second_launch_finds_rows(diag, content):
    u, v, live = _laid_out(content)
    _, rows1, _, _, (n_c1, alone1, taken1, _) = _claim(diag, u, v, COUNTS, CAP, BIG_TAIL)
    owner, rows, c_u, c_v, (n_c, alone, taken, left) = _claim(diag, u, v, COUNTS, CAP, BIG_TAIL, launches=2)
    _check(u, v, live, BIG_TAIL, owner, rows, c_u, c_v, n_c, alone, taken, left, earlier_alone=alone1)
    assert not (owner[live] & TAGGED).any(), "the second launch left a pending word: it saw no row"
    assert (n_c, alone, taken) == (n_c1 + alone1, 2 * alone1, taken1)   # nothing new but the rows alone, once more


@pytest.mark.parametrize("content", ("mixed", "irregular"))
def test_release_then_the_same_queue_again(diag, content):
    """`irregular` with a 4-slot tail: whichever 4 of the 12 classes find a slot, the counts are the same (each class has as
    many entries as the others); which 4 of `mixed`'s irregular classes would is the hardware's choice, so it takes a tail
    with room."""
    counts, cap, tail = (COUNTS, CAP, BIG_TAIL) if content == "mixed" else (np.array([2048 * 3, 0, 12 * 100], dtype=np.uint32), 2048 * 3 + 1, 4)
    u, v, live = _laid_out(content, counts, cap)
    _, _, _, _, first = _claim(diag, u, v, counts, cap, tail)
    owner, rows, c_u, c_v, again = _claim(diag, u, v, counts, cap, tail, launches=2, release_between=1)
    _check(u, v, live, tail, owner, rows, c_u, c_v, *again)
    assert again == first and first[3] == 0 and first[2] > 0


# ---- R alone: the raw-pair pass against share_claim_kernel
@pytest.mark.parametrize("case", tile.CASES)
def test_raw_pair_pass_counts_as_the_claim_pass(ptmi_lib, case):
    keys, live, slots = tile._queue(case)
    _, d_keys, length, over, _, table = tile._run(ptmi_lib, keys, slots)
    owner, r_keys, r_length, r_over, _, r_table = tile._run(ptmi_lib, keys, slots, memo=2)
    assert (owner == 0xFFFFFFFF).all(), "the raw-pair pass wrote an owner word"
    k_live = keys[live]
    assert np.array_equal(np.unique(r_keys[:r_length]), np.unique(k_live))
    assert int((r_table != tile.EMPTY).sum()) == int((table != tile.EMPTY).sum())
    if case == "four_slots":                               # which 4 keys find a slot is the hardware's choice
        uniq, per_key = np.unique(k_live, return_counts=True)
        q_uniq, q_per_key = np.unique(r_keys[:r_length], return_counts=True)
        slotted = q_per_key == 1
        assert int(slotted.sum()) == 4 and np.array_equal(q_per_key[~slotted], per_key[~slotted])
        assert r_over == int(per_key[~slotted].sum()) and r_length == 4 + r_over
    else:
        assert (r_length, r_over) == (length, over)
        assert np.array_equal(np.sort(r_keys[:r_length]), np.sort(d_keys[:length]))


# ---- renders
W, H, DEPTH, STEPS = 64, 48, 8, 3
CONFIGS = {"two_batches": dict(ipb=32, spp=64), "four_batches": dict(ipb=6, spp=17), "nine_batches": dict(ipb=2, spp=17)}
AA_SCALES = {"aa_0.3": 0.3, "aa_0.01": 0.01}
MODES = {"default": None, "step": "step"}


def _nif(r, seed=2024):
    r.init_nif_weights(nif_assets.synthetic_nif(seed=seed), 12, META["max"], nif_assets.folded_mean())


def _render(P, cfg, aa, sharing, class_slots=None, weights_at=None):
    """STEPS steps with the film resident; sharing: None (the handle's own choice) or a mode set ahead of the first step;
    class_slots: a class capacity forced by the test build (which declines the map); weights_at: another model from that step
    on.  Returns (records per step, film, sharing stats, class stats)."""
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=cfg["ipb"], diag=class_slots is not None)
    try:
        _nif(r)
        r.init_render_settings(aa_noise_scale=aa, samples_per_step=cfg["spp"])
        if class_slots is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_class_capacity(r.handle, class_slots) == 0
        if sharing:
            r.set_nif_sharing(sharing)
        rec = P.worklist(W, H)
        r.setup(rec)
        records, stats, classes = [], [], []
        for i in range(STEPS):
            if weights_at == i:
                _nif(r, seed=77)
            r.path_trace()
            stats.append(r.nif_sharing_stats())
            classes.append(r.nif_class_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        return records, r.gather_hdr(W * H, P.HDR_FILM).tobytes(), stats, classes
    finally:
        r.close()


@pytest.fixture(scope="module")
def off(ptmi_lib):
    """off(config, aa, weights_at): the same steps with sharing explicitly off, rendered once per case and left unchanged."""
    known = {}

    def get(config, aa, weights_at=None):
        if (config, aa, weights_at) not in known:
            known[(config, aa, weights_at)] = _render(ptmi_lib, CONFIGS[config], AA_SCALES[aa], "off", weights_at=weights_at)
        return known[(config, aa, weights_at)]

    return get


@pytest.fixture(scope="module")
def counted(ptmi_lib):
    """counted(spp, aa, step): (escaped paths, distinct raw pairs, distinct classes) of a step, with numpy from pt_trace_paths."""
    P = ptmi_lib
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=32)
    _nif(r)
    px = np.arange(W * H)
    known = {}

    def get(spp, aa, step):
        if (spp, aa, step) not in known:
            r.init_render_settings(aa_noise_scale=AA_SCALES[aa], samples_per_step=spp)
            s = np.repeat(np.arange(step * spp, (step + 1) * spp, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, spp), np.tile(px // W, spp), s)
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).reshape(-1, 2)
            bits = uv.view(np.uint32).astype(np.uint64)
            raw = (bits[:, 0] << np.uint64(32)) | bits[:, 1]
            known[(spp, aa, step)] = (int(esc.sum()), np.unique(raw).size, np.unique(class_key(uv[:, 0].copy(), uv[:, 1].copy())).size)
        return known[(spp, aa, step)]

    yield get
    r.close()


def _check_steps(cfg, aa, stats, classes, counted, mapped=True):
    for i, (st, cl) in enumerate(zip(stats, classes)):
        escaped, distinct, n_classes = counted(cfg["spp"], aa, i)
        print("step %d: %r %r; numpy: escaped %d distinct %d classes %d" % (i, st, cl, escaped, distinct, n_classes))
        assert st["mode"] == "step" and st["escaped"] == escaped and st["share_ms"] > 0.0 and st["overflowed"] == 0
        assert st["evaluations"] == distinct, "the raw-pair pass counts the distinct raw pairs"
        assert cl["ran"] and cl["alone"] == 0 and cl["class_ms"] == 0.0
        assert cl["mlp_rows"] == n_classes, "a row per class, in every step: the release left nothing behind"
        assert (cl["table_slots"] == MAP_WORDS + (1 << 16)) == mapped


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("aa", sorted(AA_SCALES))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_mapped_step_renders_the_bytes_of_explicit_off(ptmi_lib, off, counted, config, aa, mode):
    cfg = CONFIGS[config]
    ref_records, ref_film, _, _ = off(config, aa)
    records, film, stats, classes = _render(ptmi_lib, cfg, AA_SCALES[aa], MODES[mode])
    assert records == ref_records, "records differ from explicit off"
    assert film == ref_film, "resident film differs from explicit off"
    _check_steps(cfg, aa, stats, classes, counted)


def test_map_declined_runs_the_hashed_path(ptmi_lib, off, counted):
    """A forced class capacity selects the hashed class table: the fused step as it was, the same bytes and counts."""
    cfg = CONFIGS["nine_batches"]
    ref_records, ref_film, _, _ = off("nine_batches", "aa_0.3")
    records, film, stats, classes = _render(ptmi_lib, cfg, 0.3, None, class_slots=1 << 20)   # (room for every class: none alone)
    assert records == ref_records and film == ref_film
    _check_steps(cfg, "aa_0.3", stats, classes, counted, mapped=False)
    assert all(cl["table_slots"] == 1 << 20 for cl in classes)


def test_new_weights_between_mapped_steps(ptmi_lib, off):
    """pt_upload_nif ahead of the second step: the map holds nothing of the first model's rows."""
    ref_records, ref_film, _, _ = off("four_batches", "aa_0.3", weights_at=1)
    records, film, stats, classes = _render(ptmi_lib, CONFIGS["four_batches"], 0.3, None, weights_at=1)
    assert records == ref_records and film == ref_film
    assert records[1] != off("four_batches", "aa_0.3")[0][1], "the second model renders what the first does"
    assert all(st["mode"] == "step" for st in stats) and all(cl["table_slots"] == MAP_WORDS + (1 << 16) for cl in classes)
