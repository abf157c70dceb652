"""The accumulate pass in the shape that fits beside two NIF waves per SIMD: accumulate4_kernel keeps
its four consecutive items per thread with 32-bit path indices, accumulate_kernel its one item per thread, and both reduce
the step counters per wave.  Every pixel's fp32 adds are the adds of before in iteration
order, so a constant-sky render equals the oracle's in every TraceRecord field and in the step counters, as in
tests/test_gpu_parity.py::test_render_constant_sky_bit_exact_config_c1 -- here over every remainder of the unroll."""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

ENV = (1.0, 0.9, 0.8)
DEPTH = 4


def _steps_equal_the_oracle(O, P, W, H, spp, ipb, steps=1):
    cfg = O.make_config(width=W, height=H, max_path_length=DEPTH, env_rgb=ENV, fold=O.FOLD_FORWARD)
    ref = O.worklist(W, H)
    r = P.Renderer(W, H, max_path_length=DEPTH, iterations_per_batch=ipb)
    try:
        r.set_constant_env(ENV)
        r.init_render_settings(seed=1, samples_per_step=spp)
        got = P.worklist(W, H)
        r.setup(got)
        for step in range(steps):
            st = O.render(cfg, None, ref, step * spp, spp)
            r.path_trace()
            gst = r.read_results(got)
            assert got.tobytes() == ref.tobytes(), "TraceRecords of step %d differ from the oracle's" % step
            assert (gst.paths, gst.segments, gst.escaped) == (st.paths, st.segments, st.escaped), step
            assert r.stats().accumulate_launches == (spp + ipb - 1) // ipb
    finally:
        r.close()


@pytest.mark.parametrize("k", range(1, 10))
def test_one_batch_of_k_iterations_four_item_kernel(oracle, ptmi_lib, k):
    """64 x 48 = 3072 items (a multiple of four: accumulate4_kernel), one batch of k iterations for k = 1 .. 9: every
    remainder of the unroll, whatever its depth up to four, and a ragged last group."""
    _steps_equal_the_oracle(oracle, ptmi_lib, 64, 48, k, k)


def test_several_batches_and_a_second_step_four_item_kernel(oracle, ptmi_lib):
    """16 spp at 5 iterations per batch, and a second step on top: sums, count and length continue over batches and steps."""
    _steps_equal_the_oracle(oracle, ptmi_lib, 64, 48, 16, 5, steps=2)


def test_odd_worklist_one_item_kernel(oracle, ptmi_lib):
    """203 x 77 = 15631 items, not a multiple of four: accumulate_kernel, 62 workgroups with a ragged last one; 7 spp at 3 per batch."""
    _steps_equal_the_oracle(oracle, ptmi_lib, 203, 77, 7, 3)


def test_nif_lit_default_handle_equals_explicit_off(ptmi_lib):
    """NIF-lit, 64 x 48, 64 spp in two batches of 32, AA scale 0.01 (tests/test_gpu_nif_sharing_auto.py): the default handle
    (step-scope sharing: E(b) ahead of A(b)) and explicit off give the same records and the same resident film, byte for byte."""
    P = ptmi_lib
    meta = nif_assets.URBAN_ALLEY_META

    def render(mode):
        r = P.Renderer(64, 48, max_path_length=8, iterations_per_batch=32)
        try:
            r.init_nif_weights(nif_assets.synthetic_nif(), 12, meta["max"], nif_assets.folded_mean())
            r.init_render_settings(aa_noise_scale=0.01, samples_per_step=64)
            if mode is not None:
                r.set_nif_sharing(mode)
            rec = P.worklist(64, 48)
            r.setup(rec)
            out = []
            for _ in range(2):
                r.path_trace()
                st = r.read_results(rec)
                out.append((rec.tobytes(), st.paths, st.segments, st.escaped))
                r.film_accumulate()
            return out, r.gather_hdr(64 * 48, P.HDR_FILM).tobytes(), r.nif_sharing_stats()
        finally:
            r.close()

    off, off_film, off_stats = render("off")
    got, got_film, got_stats = render(None)
    assert off_stats["mode"] == "off" and got_stats["mode"] == "step" and 0 < got_stats["evaluations"] < got_stats["escaped"]
    assert got == off and got_film == off_film
    assert np.frombuffer(off[-1][0], dtype=P.TRACE_DTYPE)["sampleCount"].min() == 64   # (film_accumulate starts the records afresh)
