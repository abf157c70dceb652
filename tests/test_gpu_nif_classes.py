"""The class level of the NIF stage on the GPU (csrc/pt_nif_group.h: ClassTable, class_claim / class_resolve / class_spread;
key and sizes: csrc/ptmi_share_plan.h).

1. pt_diag_class_claim over hand-built distinct queues of 4096 rows, against numpy: the class queue is as long as the classes
   are many (plus the rows evaluated alone), every owner word points at a row of its own class, no index of the class queue is
   unused or used twice.
2. The kernels' property: pt_nif_infer of a row equals pt_nif_infer of its class owner, as bytes, for every kernel family.
3. Renders: every sharing mode with the level gives the bytes of explicit off; `evaluations` stays the distinct raw pairs and the
   new `mlp_rows` is the number of classes, counted with numpy from pt_trace_paths.

The class key is restated in numpy (tests/class_key_model.py: numpy's own binary16 conversion)."""
import ctypes as C

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests.class_key_model import class_coord, class_key

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
N = 4096
TILE = 2048                      # kClaimBlock x kClaimK of ptmi_share_plan.h: rows 2047 and 2048 lie in different claim tiles
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
TAGGED = 0x80000000
CASES = ("mixed", "equal", "distinct", "four_slots")


def _f(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _ulps(x, d):
    return (np.asarray(x, dtype=np.float32).view(np.int32) + np.int32(d)).view(np.float32)


def _queue(case):
    """(u, v, table slots): one region of N live rows."""
    slots = 1 << 14
    if case == "equal":
        return np.full(N, 0.3, np.float32), np.full(N, 0.7, np.float32), slots
    i = np.arange(N)
    if case == "distinct":       # a 64 x 64 grid of step 1/128: x moves by 1/64 from row to row, far more than a half's ulp
        return (0.25 + (i % 64) / 128.0).astype(np.float32), (0.25 + (i // 64) / 128.0).astype(np.float32), slots
    if case == "four_slots":     # 16 classes, each many times over and in several fp32 versions: 4 find a slot
        u = _ulps(np.float32(0.1) + (i % 16).astype(np.float32) / np.float32(32), (i // 16) % 3)
        return u, np.full(N, 0.6, np.float32), 4
    rng = np.random.default_rng(11)
    u, v = rng.random(N, dtype=np.float32), rng.random(N, dtype=np.float32)
    # rows that differ in fp32 and share a class: each row of the second quarter is a row of the first, moved by an ulp or two
    # where that stays in the class; one such pair straddles two claim tiles
    for lo in (0, TILE):
        src, dst = slice(lo, lo + 512), slice(lo + 512, lo + 1024)
        for arr in (u, v):
            moved = _ulps(arr[src], 2)
            arr[dst] = np.where(class_coord(moved) == class_coord(arr[src]), moved, arr[src])
    u[TILE - 1], v[TILE - 1] = 0.4, 0.2
    u[TILE], v[TILE] = _ulps(0.4, 3), _ulps(0.2, -3)
    assert class_key(u[TILE - 1:TILE], v[TILE - 1:TILE]) == class_key(u[TILE:TILE + 1], v[TILE:TILE + 1]) and u[TILE] != u[TILE - 1]
    # one ulp of x on either side of a rounding boundary: x = -(1 + 2^-11) is the midpoint of two halves, coord = 1 + x / 2
    # (two ulps of the coordinate are one of x)
    mid = np.float32(1.0 - (1.0 + 2.0 ** -11) / 2.0)
    u[3000:3003] = [_ulps(mid, -2), mid, _ulps(mid, 2)]
    v[3000:3003] = 0.5
    x = (u[3000:3003] - np.float32(1.0)) * np.float32(2.0)
    assert np.array_equal(x.view(np.int32) - x.view(np.int32)[1], [1, 0, -1]) and x[1] == -(1.0 + 2.0 ** -11)
    assert class_coord(u[3000:3001]) != class_coord(u[3002:3003])
    # tiny |x| (its own bits), 1.0, greater than 1 (in range and not), below 0, NaN and the tables' empty marker
    u[3010:3014] = [1.0, _ulps(1.0, -1), _ulps(1.0, -2), np.float32(1.0 - 2.0 ** -16)]
    u[3014:3018] = [1.25, _ulps(1.25, 1), 2.5, -0.5]
    u[3018:3020] = np.nan
    v[3018:3020] = [0.5, np.nan]
    u[3020:3023] = _f([0xFFFFFFFF] * 3)
    v[3020:3023] = _f([0xFFFFFFFF] * 3)
    u[3030:3034] = 1.0
    v[3030:3034] = 1.0
    return u, v, slots


def _claim(P, u, v, slots):
    lib = P.load_library(diag=True)
    r = P.Renderer(64, 64, max_path_length=4, diag=True)
    try:
        u, v = np.ascontiguousarray(u, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
        owner = np.zeros(N, np.uint32)
        c_u, c_v = np.zeros(N, np.float32), np.zeros(N, np.float32)
        length, alone = C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.pt_diag_class_claim(r.handle, ptr(u), ptr(v), N, slots, ptr(owner), ptr(c_u), ptr(c_v),
                                     C.cast(C.byref(length), C.c_void_p), C.cast(C.byref(alone), C.c_void_p))
        assert rc == 0, rc
        return owner, c_u, c_v, int(length.value), int(alone.value)
    finally:
        r.close()


@pytest.fixture(scope="module")
def claimed(ptmi_lib):
    """claimed(case): the queue of a case and what pt_diag_class_claim made of it, run once per case and left unchanged."""
    known = {}

    def get(case):
        if case not in known:
            u, v, slots = _queue(case)
            known[case] = (u, v, slots) + _claim(ptmi_lib, u, v, slots)
        return known[case]

    return get


@pytest.mark.parametrize("case", CASES)
def test_class_claim_against_numpy(claimed, case):
    u, v, slots, owner, c_u, c_v, length, alone = claimed(case)
    keys = class_key(u, v)
    uniq, per_key = np.unique(keys, return_counts=True)
    print(case, "rows", N, "classes", uniq.size, "class queue", length, "alone", alone)
    assert 0 < length <= N
    assert not (owner & TAGGED).any(), "an owner word is not a class-store index after resolve"
    assert np.array_equal(np.unique(owner), np.arange(length)), "a class-queue index is unused, used twice or beyond the length"
    q_keys = class_key(c_u[:length], c_v[:length])
    assert np.array_equal(q_keys[owner], keys), "an owner word points at a row of another class"
    # the class queue holds rows of the queue itself, bit for bit: each owner's (u, v) is one of its class's rows
    raw = (u.view(np.uint32).astype(np.uint64) << np.uint64(32)) | v.view(np.uint32)
    q_raw = (c_u[:length].view(np.uint32).astype(np.uint64) << np.uint64(32)) | c_v[:length].view(np.uint32)
    assert np.isin(q_raw, raw).all()
    q_uniq, q_per_key = np.unique(q_keys, return_counts=True)
    assert np.array_equal(q_uniq, uniq)
    if case == "four_slots":
        is_alone = q_per_key > 1
        assert int((~is_alone).sum()) == 4 and alone > 0 and per_key.min() > 1
    else:
        is_alone = uniq == EMPTY
        assert alone == int((keys == EMPTY).sum())
        assert length == uniq.size - int(EMPTY in uniq) + alone     # np.unique of class_key, plus the rows evaluated alone
    assert np.array_equal(q_per_key[~is_alone], np.ones(int((~is_alone).sum()), q_per_key.dtype))
    assert np.array_equal(q_per_key[is_alone], per_key[is_alone])
    assert alone == int(per_key[is_alone].sum()) and length == int((~is_alone).sum()) + alone
    if case == "equal":
        assert length == 1
    if case == "distinct":
        assert length == N
    if case == "mixed":
        assert alone == 3 and uniq.size < np.unique(raw).size - 900, "the queue was built to hold far fewer classes than raw pairs"


MODELS = {
    "fused_e12": dict(hidden=320, layer_count=6, embedding_dim=12),
    "fused_e16": dict(hidden=320, layer_count=6, embedding_dim=16),
    "layerwise_352": dict(hidden=352, layer_count=2, embedding_dim=12),
    "float32_32": dict(hidden=32, layer_count=2, embedding_dim=12, dtype=np.float32),
}


@pytest.mark.parametrize("model", sorted(MODELS))
def test_a_row_and_its_class_owner_infer_the_same_bytes(ptmi_lib, claimed, model):
    """Rows with a NaN coordinate are compared too: as bytes.  u = 0 is in the queue at E = 16 (row 0), where its last feature
    overflows to infinity."""
    P = ptmi_lib
    u, v, _, owner, c_u, c_v, length, _ = claimed("mixed")
    u, v = u.copy(), v.copy()
    r = P.Renderer(64, 64, max_path_length=4)
    try:
        kw = MODELS[model]
        r.init_nif_weights(nif_assets.synthetic_nif(**kw), kw["embedding_dim"], META["max"], nif_assets.folded_mean())
        u0 = np.concatenate([[np.float32(0.0), np.float32(2.0 ** -30)], u])     # x = -2 and a float that shares its class
        v0 = np.concatenate([[np.float32(0.25), np.float32(0.25)], v])
        rows = r.nif_infer(u0, v0)
        owners = r.nif_infer(c_u[:length], c_v[:length])
        name = r.nif_kernel_name()
    finally:
        r.close()
    print(model, name)
    assert ("nif32" in name) == (model == "float32_32") and ("nifg16" in name) == (model == "layerwise_352")
    assert rows[0].tobytes() == rows[1].tobytes()
    assert rows[2:].tobytes() == owners[owner].tobytes()
    moved = (u.view(np.uint32) != c_u[owner].view(np.uint32)) | (v.view(np.uint32) != c_v[owner].view(np.uint32))
    assert moved.sum() > 500, "the comparison must cover rows whose owner has other fp32 coordinates"


# ---- renders
W, H, DEPTH, STEPS, IPB, SPP = 64, 48, 8, 3, 2, 17       # nine batches a step: the ring of three buffer sets wraps
AA_SCALES = {"aa_0.3": 0.3, "aa_0.01": 0.01}
MEMO_BYTES = 192 << 20
MODES = {"default": (None, 0, "step"), "step": ("step", 0, "step"), "batch": ("batch", 0, "batch"), "memo": (None, MEMO_BYTES, "off")}


def _nif(r, seed=2024):
    r.init_nif_weights(nif_assets.synthetic_nif(seed=seed), 12, META["max"], nif_assets.folded_mean())


def _render(P, aa, sharing, memo=0, class_slots=None, swap_weights=False):
    """STEPS steps with the film resident: (records of every step, resident film, sharing stats, class stats of every step)."""
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=IPB, diag=class_slots is not None)
    try:
        _nif(r)
        r.init_render_settings(aa_noise_scale=aa, samples_per_step=SPP)
        if class_slots is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_class_capacity(r.handle, class_slots) == 0
        if memo:
            r.set_nif_memo(memo)
        if sharing is not None:
            r.set_nif_sharing(sharing)
        rec = P.worklist(W, H)
        r.setup(rec)
        records, stats, classes = [], [], []
        for i in range(STEPS):
            if swap_weights and i == 1:
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
    """off(aa, swap): the run with sharing explicitly off, rendered once per case and left unchanged."""
    known = {}

    def get(aa, swap=False):
        if (aa, swap) not in known:
            known[(aa, swap)] = _render(ptmi_lib, AA_SCALES[aa], "off", swap_weights=swap)
        return known[(aa, swap)]

    return get


@pytest.fixture(scope="module")
def counted(ptmi_lib):
    """counted(aa, step): (escaped paths, distinct raw (u, v) pairs, distinct class keys) of a step, with numpy from pt_trace_paths."""
    P = ptmi_lib
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=32)
    _nif(r)
    px = np.arange(W * H)
    known = {}

    def get(aa, step):
        if (aa, step) not in known:
            r.init_render_settings(aa_noise_scale=AA_SCALES[aa], samples_per_step=SPP)
            s = np.repeat(np.arange(step * SPP, (step + 1) * SPP, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, SPP), np.tile(px // W, SPP), s)
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).reshape(-1, 2)
            bits = uv.view(np.uint32).astype(np.uint64)
            known[(aa, step)] = (int(esc.sum()), np.unique((bits[:, 0] << np.uint64(32)) | bits[:, 1]).size,
                                 np.unique(class_key(uv[:, 0].copy(), uv[:, 1].copy())).size)
        return known[(aa, step)]

    yield get
    r.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("aa", sorted(AA_SCALES))
def test_every_mode_renders_the_bytes_of_explicit_off(ptmi_lib, off, counted, aa, mode):
    sharing, memo, reported = MODES[mode]
    ref_records, ref_film, ref_stats, ref_classes = off(aa)
    records, film, stats, classes = _render(ptmi_lib, AA_SCALES[aa], sharing, memo=memo)
    for i, (a, b) in enumerate(zip(records, ref_records)):
        assert a == b, "records of step %d differ from explicit off" % i
    assert film == ref_film, "resident film differs from explicit off"
    for i, (st, cl, o, ocl) in enumerate(zip(stats, classes, ref_stats, ref_classes)):
        escaped, distinct, n_classes = counted(aa, i)
        print("%s %s step %d: %r %r; numpy: escaped %d distinct %d classes %d" % (aa, mode, i, st, cl, escaped, distinct, n_classes))
        # explicit off: the level did not run, and the network ran a row per escaped path
        assert o["mode"] == "off" and not ocl["ran"] and ocl["alone"] == 0 and ocl["table_slots"] == 0
        assert ocl["mlp_rows"] == o["evaluations"] == o["escaped"] == escaped
        assert st["mode"] == reported and st["escaped"] == escaped and st["overflowed"] == 0
        assert cl["ran"] and cl["alone"] == 0 and cl["table_slots"] >= 2 * cl["mlp_rows"]
        assert cl["mlp_rows"] <= st["evaluations"] <= escaped
        if reported == "step":
            assert st["evaluations"] == distinct         # as today: the distinct raw pairs
        if not memo or i == 0:                           # the class table lives for the step whatever the sharing mode
            assert cl["mlp_rows"] == n_classes
        if aa == "aa_0.3":
            assert cl["mlp_rows"] < st["evaluations"]


def test_a_16_slot_class_table_evaluates_rows_alone_and_stays_exact(ptmi_lib, off):
    ref_records, ref_film, ref_stats, _ = off("aa_0.3")
    records, film, stats, classes = _render(ptmi_lib, AA_SCALES["aa_0.3"], "step", class_slots=16)
    assert records == ref_records and film == ref_film
    for st, cl, o in zip(stats, classes, ref_stats):
        print(st, cl)
        assert cl["ran"] and cl["table_slots"] == 16 and cl["alone"] > 0
        assert st["mode"] == "step" and st["escaped"] == o["escaped"] and cl["mlp_rows"] <= st["evaluations"]


def test_new_weights_between_steps(ptmi_lib, off):
    """pt_upload_nif of another model ahead of the second step: no class of the first step's model serves it."""
    ref_records, ref_film, _, _ = off("aa_0.3", swap=True)
    plain_records, _, _, _ = off("aa_0.3")
    assert ref_records[0] == plain_records[0] and ref_records[1] != plain_records[1]
    for sharing, memo in ((None, 0), (None, MEMO_BYTES)):
        records, film, _, classes = _render(ptmi_lib, AA_SCALES["aa_0.3"], sharing, memo=memo, swap_weights=True)
        assert all(cl["ran"] for cl in classes)
        assert records == ref_records and film == ref_film
