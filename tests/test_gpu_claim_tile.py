"""The claim pass's workgroup tiles on the GPU (group_claim in csrc/pt_nif_group.h: kClaimK entries per thread, one reservation
in the distinct queue per tile).  The profiling build's pt_diag_claim_resolve runs claim + resolve over a queue built here, for
the sharing table and for the memo's, and numpy says what must come out: how long the distinct queue is, that it holds every
key once (a key without a slot once per entry), that every entry's owner holds the entry's own (u, v) bit for bit and that no
owner word stays pending.  Then one render whose trace regions span more than one tile, against sharing off."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = nif_assets.URBAN_ALLEY_META
_PLAN = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "ptmi_share_plan.h")).read()
K = int(re.search(r"constexpr uint32_t kClaimK = (\d+);", _PLAN).group(1))
TILE = 256 * K
COUNTS = np.array([0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 65], dtype=np.uint32)   # one launch, a region each
CAP = 2 * TILE + 100                                                                  # no multiple of the tile
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
TAGGED, PENDING, SLOT_BITS = 0x80000000, 0xC0000000, 0x3FFFFFFF
CASES = ("equal", "distinct", "pair_across_tiles", "empty_marker", "four_slots")


def _queue(case):
    """(keys [regions x CAP] uint64, live mask, table slots).  The dead slots of a region hold keys no live entry has: a pass
    that took one would lengthen the distinct queue."""
    n = COUNTS.size * CAP
    idx = np.arange(n, dtype=np.uint64)
    keys = ((np.uint64(0x3F000000) + idx) << np.uint64(32)) | (np.uint64(0x3E000000) + np.uint64(7) * idx)
    local = np.arange(n) % CAP
    live = local < np.repeat(COUNTS, CAP)
    slots = 1 << 16
    if case == "equal":
        keys[live] = (np.uint64(0x3D000000) << np.uint64(32)) | np.uint64(5)
    elif case == "pair_across_tiles":
        base = 5 * CAP                       # the last region: entries TILE - 1 (tile 0) and TILE (tile 1)
        keys[base + TILE] = keys[base + TILE - 1]
    elif case == "empty_marker":
        keys[3 * CAP + 77] = EMPTY
    elif case == "four_slots":
        j = np.arange(16, dtype=np.uint64)
        some = ((np.uint64(0x3D000000) + j) << np.uint64(32)) | j      # 16 keys, each many times over: 4 find a slot
        keys[live] = some[np.arange(int(live.sum())) % 16]
        slots = 4
    return keys.reshape(COUNTS.size, CAP), live.reshape(COUNTS.size, CAP), slots


def _run(P, keys, slots, memo=0, passes=1):
    lib = P.load_library(diag=True)
    r = P.Renderer(64, 64, max_path_length=4, diag=True)
    try:
        n = keys.size
        u = np.ascontiguousarray((keys >> np.uint64(32)).astype(np.uint32))
        v = np.ascontiguousarray((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        owner = np.zeros(n, np.uint32)
        d_u, d_v = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        d_count, over = C.c_uint32(0), C.c_uint64(0)
        ctr, table = np.zeros(4, np.uint64), np.zeros(slots, np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.pt_diag_claim_resolve(r.handle, memo, passes, ptr(u), ptr(v), ptr(COUNTS), COUNTS.size, CAP, slots, ptr(owner),
                                       ptr(d_u), ptr(d_v), C.cast(C.byref(d_count), C.c_void_p), C.cast(C.byref(over), C.c_void_p),
                                       ptr(ctr), ptr(table))
        assert rc == 0, rc
        d_keys = (d_u.astype(np.uint64) << np.uint64(32)) | d_v.astype(np.uint64)
        return owner.reshape(keys.shape), d_keys, int(d_count.value), int(over.value), ctr, table
    finally:
        r.close()


def _check_first_pass(case, keys, live, owner, d_keys, length, over):
    """What claim + resolve leave over an empty table; returns the number of keys that hold a slot."""
    k_live, o_live = keys[live], owner[live]
    uniq, per_key = np.unique(k_live, return_counts=True)
    if case == "four_slots":
        expect_over = None                                   # which 4 keys find a slot is the hardware's choice
    else:
        expect_over = int((k_live == EMPTY).sum())
        assert over == expect_over
        assert length == uniq.size - int(EMPTY in uniq) + over      # distinct keys, plus the entries evaluated alone
    assert 0 < length <= k_live.size
    assert not (o_live & TAGGED).any(), "an owner word is not a store index after resolve"
    assert np.array_equal(np.unique(o_live), np.arange(length)), "a distinct-queue index is unused, used twice or beyond the length"
    assert np.array_equal(d_keys[o_live], k_live), "an owner holds another (u, v) than its entry"
    # every key once in the distinct queue, or -- without a slot -- once per entry
    q_uniq, q_per_key = np.unique(d_keys[:length], return_counts=True)
    assert np.array_equal(q_uniq, uniq)
    alone = q_per_key > 1 if case == "four_slots" else uniq == EMPTY
    assert np.array_equal(q_per_key[~alone], np.ones(int((~alone).sum()), q_per_key.dtype))
    assert np.array_equal(q_per_key[alone], per_key[alone])
    assert over == int(per_key[alone].sum())
    slotted = int((~alone).sum())
    assert length == slotted + over
    if case == "four_slots":
        assert slotted == 4 and per_key.min() > 1
    if case == "equal":
        assert length == 1
    if case == "distinct":
        assert length == k_live.size
    return slotted


@pytest.mark.parametrize("case", CASES)
def test_share_table(ptmi_lib, case):
    keys, live, slots = _queue(case)
    owner, d_keys, length, over, _, table = _run(ptmi_lib, keys, slots)
    slotted = _check_first_pass(case, keys, live, owner, d_keys, length, over)
    assert int((table != EMPTY).sum()) == slotted


@pytest.mark.parametrize("case", CASES)
def test_memo_table_first_and_second_launch(ptmi_lib, case):
    keys, live, slots = _queue(case)
    owner, d_keys, length, over, ctr, table = _run(ptmi_lib, keys, slots, memo=1, passes=1)
    slotted = _check_first_pass(case, keys, live, owner, d_keys, length, over)
    occupied, served, inserted = int(ctr[0]), int(ctr[1]), int(ctr[2])
    assert (occupied, served, inserted) == (slotted, 0, slotted)
    assert int((table != EMPTY).sum()) == slotted
    # the same keys again after a publish: whatever holds a slot is served from it, the rest is evaluated alone again
    owner, d_keys, length, over, ctr, table = _run(ptmi_lib, keys, slots, memo=1, passes=2)
    k_live, o_live = keys[live], owner[live]
    is_served = (o_live & PENDING) == TAGGED
    assert not ((o_live & PENDING) == PENDING).any(), "an owner word is left pending"
    assert np.array_equal(table[o_live[is_served] & SLOT_BITS], k_live[is_served]), "served from another key's slot"
    assert np.array_equal(d_keys[o_live[~is_served]], k_live[~is_served])
    assert np.array_equal(np.sort(o_live[~is_served]), np.arange(length))
    n_slotted = int((table != EMPTY).sum())
    assert n_slotted == slotted
    in_table = np.isin(k_live, table[table != EMPTY]) & (k_live != EMPTY)
    assert np.array_equal(is_served, in_table)
    assert length == over == int((~in_table).sum())
    assert (int(ctr[0]), int(ctr[1]), int(ctr[2])) == (slotted, int(in_table.sum()), 0)


def _render(P, mode, memo=0, steps=2, W=256, H=256, spp=64):
    r = P.Renderer(W, H, max_path_length=8)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=spp)
        r.set_nif_sharing(mode)
        if memo:
            r.set_nif_memo(memo)
        rec = P.worklist(W, H)
        r.setup(rec)
        share, memo_stats = [], []
        for _ in range(steps):
            r.path_trace()
            share.append(r.nif_sharing_stats())
            memo_stats.append(r.nif_memo_stats())
            r.film_accumulate()
        return r.gather_hdr(W * H, P.HDR_FILM).tobytes(), share, memo_stats
    finally:
        r.close()


def _distinct_in_first_step(P, W=256, H=256, spp=64):
    """The distinct (u, v) bit pairs of the first step's escaped paths, from pt_trace_paths and numpy alone."""
    r = P.Renderer(W, H, max_path_length=8)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(samples_per_step=spp)
        px = np.arange(W * H)
        found, escaped = [], 0
        for s0 in range(0, spp, 16):
            s = np.repeat(np.arange(s0, s0 + 16, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, 16), np.tile(px // W, 16), s)
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).view(np.uint32).reshape(-1, 2).astype(np.uint64)
            found.append(np.unique((uv[:, 0] << np.uint64(32)) | uv[:, 1]))
            escaped += int(esc.sum())
        return np.unique(np.concatenate(found)).size, escaped
    finally:
        r.close()


def test_render_with_regions_of_more_than_one_tile(ptmi_lib):
    """256 x 256, 64 spp, depth 8, synthetic 6 x 320 NIF: a trace region holds 2816 entries, more than a tile of 256 x 8."""
    P = ptmi_lib
    film_off, _, _ = _render(P, "off")
    film_step, share, _ = _render(P, "step")
    assert film_step == film_off
    distinct, escaped = _distinct_in_first_step(P)
    assert share[0]["mode"] == "step" and share[0]["overflowed"] == 0
    assert share[0]["escaped"] == escaped and share[0]["evaluations"] == distinct < escaped
    film_memo, _, memo = _render(P, "off", memo=1 << 30)
    assert film_memo == film_off
    assert memo[0]["served"] == 0 and memo[0]["evaluations"] == distinct
    assert memo[1]["served"] > 0
