"""The expand pass (reads ahead of its stores, with either table) and the table's clear handed from step to step: every
sharing mode renders the bytes of explicit off, on the records of every step and on the resident film.  An entry that E(b)
does not expand, or expands from the wrong owner, reads the radiance its buffer set held three batches earlier or another
key's, so the first configuration wraps the ring of three sets: 17 samples per step in batches of 2 iterations are 9
batches.  The second has two batches (64 samples, 32 iterations each).  Both at AA scale 0.3, where nearly every owner lies
in the entry's own batch, and at 0.01, where the samples of a pixel share their camera ray and most owners lie in earlier
batches of the step (or, with the memo, in earlier steps).  64 x 48 pixels, depth 8, three steps per run, so that two steps
of each step-scope run start on a table the step before cleared; in every step-scope step the evaluations are the distinct
(u, v) bit pairs of the step, counted as tests/test_gpu_nif_sharing_auto.py counts them.  (A split of E(b) into an early
and a late pass was measured slower and is not in the tree; these cases are what it had to pass.)"""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

META = nif_assets.URBAN_ALLEY_META
W, H, DEPTH, STEPS = 64, 48, 8, 3
CONFIGS = {"nine_batches": dict(ipb=2, spp=17), "two_batches": dict(ipb=32, spp=64)}
AA_SCALES = {"aa_0.3": 0.3, "aa_0.01": 0.01}
MEMO_BYTES = 192 << 20
# mode -> (set_nif_sharing argument or None for a handle that never calls it, memo bytes, what nif_sharing_stats reports)
MODES = {"default": (None, 0, "step"), "step": ("step", 0, "step"), "batch": ("batch", 0, "batch"), "memo": (None, MEMO_BYTES, "off")}


def _nif(r):
    r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())


def _render(P, cfg, aa, sharing, memo=0, capacity=None):
    """STEPS steps with the film resident: (records of every step, resident film, sharing stats, memo stats of every step)."""
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=cfg["ipb"], diag=capacity is not None)
    try:
        _nif(r)
        r.init_render_settings(aa_noise_scale=aa, samples_per_step=cfg["spp"])
        if capacity is not None:
            assert P.load_library(diag=True).pt_diag_set_nif_share_capacity(r.handle, capacity) == 0
        if memo:
            r.set_nif_memo(memo)
        if sharing is not None:
            r.set_nif_sharing(sharing)
        rec = P.worklist(W, H)
        r.setup(rec)
        records, stats, memos = [], [], []
        for _ in range(STEPS):
            r.path_trace()
            stats.append(r.nif_sharing_stats())
            memos.append(r.nif_memo_stats())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        return records, r.gather_hdr(W * H, P.HDR_FILM).tobytes(), stats, memos
    finally:
        r.close()


@pytest.fixture(scope="module")
def off(ptmi_lib):
    """off(config, aa): the run with sharing explicitly off, rendered once per (config, aa) and left unchanged."""
    known = {}

    def get(config, aa):
        if (config, aa) not in known:
            known[(config, aa)] = _render(ptmi_lib, CONFIGS[config], AA_SCALES[aa], "off")
        return known[(config, aa)]

    return get


@pytest.fixture(scope="module")
def distinct_pairs(ptmi_lib):
    """distinct(aa, first, n): (escaped paths, distinct (u, v) bit pairs among them) of samples first .. first + n - 1 of every
    pixel, counted with numpy from pt_trace_paths; every range is traced once."""
    P = ptmi_lib
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=32)
    _nif(r)
    px = np.arange(W * H)
    known = {}

    def distinct(aa, first, n):
        if (aa, first, n) not in known:
            r.init_render_settings(aa_noise_scale=AA_SCALES[aa], samples_per_step=n)
            s = np.repeat(np.arange(first, first + n, dtype=np.uint32), W * H)
            paths = r.trace_paths(np.tile(px % W, n), np.tile(px // W, n), s)
            esc = paths["escaped"] != 0
            uv = np.ascontiguousarray(paths["uv"][esc]).view(np.uint32).reshape(-1, 2).astype(np.uint64)
            known[(aa, first, n)] = (int(esc.sum()), np.unique((uv[:, 0] << np.uint64(32)) | uv[:, 1]).size)
        return known[(aa, first, n)]

    yield distinct
    r.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("aa", sorted(AA_SCALES))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_mode_renders_the_bytes_of_explicit_off(ptmi_lib, off, distinct_pairs, config, aa, mode):
    sharing, memo, reported = MODES[mode]
    spp = CONFIGS[config]["spp"]
    ref_records, ref_film, ref_stats, _ = off(config, aa)
    records, film, stats, memos = _render(ptmi_lib, CONFIGS[config], AA_SCALES[aa], sharing, memo=memo)
    assert len(records) == len(ref_records) == STEPS
    for i, (a, b) in enumerate(zip(records, ref_records)):
        assert a == b, "records of step %d differ from explicit off" % i
    assert film == ref_film, "resident film differs from explicit off"
    for i, (st, o, m) in enumerate(zip(stats, ref_stats, memos)):
        print("%s %s %s step %d: %r %r" % (config, aa, mode, i, st, m if memo else ""))
        assert o["mode"] == "off" and st["mode"] == reported and st["escaped"] == o["escaped"] > 0, (st, o)
        assert st["overflowed"] == 0, st
        if st["mode"] == "step":
            escaped, distinct = distinct_pairs(aa, i * spp, spp)
            assert st["escaped"] == escaped
            assert st["evaluations"] == distinct, (st, distinct)
        elif mode == "batch":
            assert distinct_pairs(aa, i * spp, spp)[1] <= st["evaluations"] <= st["escaped"], st
        if memo:
            assert m["enabled"] and m["overflowed"] == 0 and m["evaluations"] + m["served"] <= m["escaped"], m
            if i == 0:
                assert m["served"] == 0 and m["evaluations"] == distinct_pairs(aa, 0, spp)[1], m
    if aa == "aa_0.01":   # the samples of a pixel share their camera ray: keys repeat from batch to batch and from step to step
        for st in stats:
            if st["mode"] != "off":
                assert st["evaluations"] < st["escaped"], st
        if memo:
            assert memos[1]["served"] > 0 and memos[2]["served"] > 0, memos


def test_a_16_slot_table_overflows_and_stays_exact(ptmi_lib, off):
    """The test build's forced capacity over nine batches per step: nearly every key finds no slot, is evaluated alone and
    owns an entry of its own batch; the few that share are expanded from an earlier batch's.  The film does not change."""
    records, film, stats, _ = _render(ptmi_lib, CONFIGS["nine_batches"], AA_SCALES["aa_0.01"], None, capacity=16)
    ref_records, ref_film, ref_stats, _ = off("nine_batches", "aa_0.01")
    assert records == ref_records and film == ref_film
    for st, o in zip(stats, ref_stats):
        print(st)
        assert st["mode"] == "step" and st["table_slots"] == 16 and st["overflowed"] > 0, st
        assert st["escaped"] == o["escaped"] and st["evaluations"] <= st["escaped"], st
