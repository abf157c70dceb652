"""Expand inside the accumulate pass of a mapped step (csrc/pt_nif_group.h: accumulate_mapped_kernel; csrc/pt_trace.h:
emit_escaped / emit_emitted with TraceParams::q_inverse; csrc/ptmi_share_plan.h: kNoQueueSlot), and the step's end: the tail's
clears inside class_map_release_kernel.

Every case renders three consecutive steps at 64 x 48 (or smaller), depth 8, with the film resident, and compares records and
film with explicit off byte for byte; the counts (evaluations, mlp_rows, escaped, overflowed) are numpy's, by
tests/test_gpu_class_map.py's _check_steps.  A worklist whose size is no multiple of four (63 x 47) keeps E(b) + A(b): it is
here to pin that the choice is made per worklist and that both paths give the same bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_class_map as cm

pytestmark = pytest.mark.gpu

off = cm.off            # off(config, aa, weights_at): the explicit-off renders of tests/test_gpu_class_map.py, once per case
counted = cm.counted    # counted(spp, aa, step): numpy's counts from pt_trace_paths

W, H, DEPTH, STEPS = cm.W, cm.H, cm.DEPTH, cm.STEPS
CONFIGS, AA_SCALES = cm.CONFIGS, cm.AA_SCALES
MAP_SLOTS = cm.MAP_WORDS + (1 << 16)


def _lamp_scene(P):
    """The built-in scene with its first sphere a lamp: camera rays and bounces both reach it."""
    scene = P.builtin_scene()
    k = int(np.flatnonzero(scene["shape"] == P.SHAPES["sphere"])[0])
    scene[k]["material"] = P.MATERIALS["emissive"]
    scene[k]["colour"] = (3.0, 2.0, 1.5)
    return scene


def _render(P, ipb, spp, aa, sharing, w=W, h=H, padding=0, scene=None, diag=False, weights_at=None, steps=STEPS):
    """`steps` steps with the film resident.  padding: worklist items with u = v = 65535 spread through the worklist.  Returns
    (records per step, film, sharing stats, class stats, pt_stats per step)."""
    n = w * h + padding
    r = P.Renderer(w, h, max_work_items=n, max_path_length=DEPTH, iterations_per_batch=ipb, diag=diag)
    try:
        cm._nif(r)
        r.init_render_settings(aa_noise_scale=aa, samples_per_step=spp)
        if scene is not None:
            r.set_scene(scene)
        if sharing:
            r.set_nif_sharing(sharing)
        rec = P.worklist(w, h)
        if padding:
            pad = np.zeros(padding, dtype=rec.dtype)
            pad["u"], pad["v"] = 65535, 65535
            at = np.linspace(5, rec.size - 5, padding).astype(np.int64)   # inside the worklist, not only behind it
            rec = np.insert(rec, at, pad)
        r.setup(rec)
        records, sharing_stats, classes, stats = [], [], [], []
        for i in range(steps):
            if weights_at == i:
                cm._nif(r, seed=77)
            r.path_trace()
            sharing_stats.append(r.nif_sharing_stats())
            classes.append(r.nif_class_stats())
            stats.append(r.stats().as_dict())
            r.read_results(rec)
            records.append(rec.tobytes())
            r.film_accumulate()
        return records, r.gather_hdr(n, P.HDR_FILM).tobytes(), sharing_stats, classes, stats
    finally:
        r.close()


def _same_as_off(P, mapped=True, **kw):
    ref = _render(P, sharing="off", **kw)
    got = _render(P, sharing=None, **kw)
    assert got[0] == ref[0], "records differ from explicit off"
    assert got[1] == ref[1], "resident film differs from explicit off"
    for st, cl, s, s_ref in zip(got[2], got[3], got[4], ref[4]):
        print(st, cl)
        assert st["mode"] == "step" and st["overflowed"] == 0 and st["escaped"] == s_ref["escaped"]
        assert (cl["table_slots"] == MAP_SLOTS) == mapped and cl["alone"] == 0
    return ref, got


@pytest.mark.parametrize("mode", sorted(cm.MODES))
@pytest.mark.parametrize("aa", sorted(AA_SCALES))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_expanding_accumulate_renders_the_bytes_of_explicit_off(ptmi_lib, off, counted, config, aa, mode):
    """17 spp over 6 or 2 iterations a batch: batches of 1, 2, 4 and 6 iterations, odd and even against the two in flight."""
    cfg = CONFIGS[config]
    ref_records, ref_film, _, _ = off(config, aa)
    records, film, stats, classes, _ = _render(ptmi_lib, cfg["ipb"], cfg["spp"], AA_SCALES[aa], cm.MODES[mode])
    assert records == ref_records, "records differ from explicit off"
    assert film == ref_film, "resident film differs from explicit off"
    cm._check_steps(cfg, aa, stats, classes, counted)


def test_worklist_no_multiple_of_four(ptmi_lib):
    """63 x 47 = 2961 items: the mapped step keeps its expand pass and the one-item accumulate kernel."""
    _same_as_off(ptmi_lib, ipb=2, spp=17, aa=0.3, w=63, h=47)


def test_worklist_with_padding_items(ptmi_lib):
    """3072 pixels and 8 padding items among them: a multiple of four, records of length 0 that own no path and no slot."""
    ref, got = _same_as_off(ptmi_lib, ipb=6, spp=17, aa=0.3, padding=8)
    rec = np.frombuffer(got[0][-1], dtype=ptmi_lib.TRACE_DTYPE)
    pad = rec["u"] == 65535
    assert int(pad.sum()) == 8 and not rec["pathLength"][pad].any()


def test_emitted_and_escaped_paths_in_one_batch(ptmi_lib):
    P = ptmi_lib
    scene = _lamp_scene(P)
    ref, got = _same_as_off(P, ipb=6, spp=17, aa=0.3, scene=scene)
    # numpy's count of the first step's escapes, and the paths that end on the lamp at depth 0 and deeper
    r = P.Renderer(W, H, max_path_length=DEPTH)
    try:
        cm._nif(r)
        r.init_render_settings(aa_noise_scale=0.3, samples_per_step=17)
        r.set_scene(scene)
        px = np.arange(W * H)
        paths = r.trace_paths(np.tile(px % W, 17), np.tile(px // W, 17), np.repeat(np.arange(17, dtype=np.uint32), W * H))
    finally:
        r.close()
    esc, lamp = paths["escaped"] == 1, paths["escaped"] == 2   # (pt_trace_paths: 2 = ended on an emitter)
    seen, reached = int((lamp & (paths["length"] == 1)).sum()), int((lamp & (paths["length"] > 1)).sum())
    print("escaped", int(esc.sum()), "camera rays on the lamp", seen, "bounces that reach it", reached)
    assert seen > 100 and reached > 100 and got[4][0]["escaped"] == int(esc.sum())
    plain = _render(P, 6, 17, 0.3, "off")
    assert plain[1] != ref[1], "the lamp lights nothing"


@pytest.mark.parametrize("spp, ipb", ((1, 4), (2, 1)), ids=("one_spp", "two_batches_of_one"))
def test_one_iteration_per_batch(ptmi_lib, counted, spp, ipb):
    ref, got = _same_as_off(ptmi_lib, ipb=ipb, spp=spp, aa=0.3)
    cm._check_steps(dict(spp=spp), "aa_0.3", got[2], got[3], counted)


def test_step_kinds_in_turn_on_one_handle(ptmi_lib):
    """Default (mapped), batch scope, off, step scope (mapped), a constant environment, the NIF and the mapped step again: the
    q_path buffers hold the inverse map in some steps and the forward one in others, and no step reads the other's."""
    P = ptmi_lib
    turns = (None, "batch", "off", "step", "constant", "nif")

    def run(all_off):
        r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=2)
        try:
            cm._nif(r)
            r.init_render_settings(aa_noise_scale=0.3, samples_per_step=17)
            if all_off:
                r.set_nif_sharing("off")
            rec = P.worklist(W, H)
            r.setup(rec)
            records, modes = [], []
            for turn in turns:
                if turn == "constant":
                    r.set_constant_env((0.5, 0.75, 1.0))
                elif turn == "nif":
                    cm._nif(r)
                elif turn is not None and not all_off:
                    r.set_nif_sharing(turn)
                r.path_trace()
                modes.append((r.nif_sharing_stats()["mode"], r.nif_class_stats()["table_slots"]))
                r.read_results(rec)
                records.append(rec.tobytes())
                r.film_accumulate()
            return records, r.gather_hdr(W * H, P.HDR_FILM).tobytes(), modes
        finally:
            r.close()

    ref_records, ref_film, _ = run(True)
    records, film, modes = run(False)
    print(modes)
    assert [m for m, _ in modes] == ["step", "batch", "off", "step", "off", "step"]
    assert [s == MAP_SLOTS for _, s in modes] == [True, False, False, True, False, True]
    for i, (a, b) in enumerate(zip(records, ref_records)):
        assert a == b, "step %d (%s) differs from the all-off handle" % (i, turns[i])
    assert film == ref_film


def test_new_weights_between_expanding_steps(ptmi_lib, off):
    ref_records, ref_film, _, _ = off("four_batches", "aa_0.3", weights_at=1)
    cfg = CONFIGS["four_batches"]
    records, film, stats, classes, _ = _render(ptmi_lib, cfg["ipb"], cfg["spp"], 0.3, None, weights_at=1)
    assert records == ref_records and film == ref_film
    assert all(cl["table_slots"] == MAP_SLOTS for cl in classes)


def _expand_launches(P, w, h, ipb, spp):
    """E(b) launches and batches of one default step on the profiling build (pt_diag_expand_launches)."""
    r = P.Renderer(w, h, max_path_length=DEPTH, iterations_per_batch=ipb, diag=True)
    try:
        cm._nif(r)
        r.init_render_settings(aa_noise_scale=0.3, samples_per_step=spp)
        r.setup(P.worklist(w, h))
        r.path_trace()
        n = C.c_uint32(12345)
        assert P.load_library(diag=True).pt_diag_expand_launches(r.handle, C.byref(n)) == 0
        assert r.nif_class_stats()["table_slots"] == MAP_SLOTS
        return n.value, r.stats().accumulate_launches
    finally:
        r.close()


def test_the_expanding_pass_runs_and_no_expand_pass(ptmi_lib, monkeypatch):
    """A mapped step over 64 x 48 launches no E(b): its accumulate passes expand.  Over 63 x 47, and with the profiling build's
    switch, it launches one per batch: no quiet fall-back either way."""
    assert _expand_launches(ptmi_lib, W, H, 2, 17) == (0, 9)
    assert _expand_launches(ptmi_lib, 63, 47, 2, 17) == (9, 9)
    monkeypatch.setenv("PTMI_EXPAND_PASS", "1")
    assert _expand_launches(ptmi_lib, W, H, 2, 17) == (9, 9)


@pytest.mark.parametrize("switch", ("PTMI_EXPAND_PASS",))
@pytest.mark.parametrize("config", ("two_batches", "nine_batches"))
def test_profiling_build_switches_render_the_same(ptmi_lib, off, counted, monkeypatch, switch, config):
    """The A/B switch of the profiling build (E(b) + A(b) as before): the same bytes and counts."""
    cfg = CONFIGS[config]
    ref_records, ref_film, _, _ = off(config, "aa_0.3")
    plain = _render(ptmi_lib, cfg["ipb"], cfg["spp"], 0.3, None, diag=True)
    monkeypatch.setenv(switch, "1")
    switched = _render(ptmi_lib, cfg["ipb"], cfg["spp"], 0.3, None, diag=True)
    monkeypatch.delenv(switch)
    for records, film, stats, classes, _ in (plain, switched):
        assert records == ref_records and film == ref_film
        cm._check_steps(cfg, "aa_0.3", stats, classes, counted)
