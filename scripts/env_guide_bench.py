#!/usr/bin/env python3
"""Environment-guided diffuse sampling (pt_set_env_guide) measured on the C2 shape: 1104x1000, 300 spp, depth 8, built-in scene,
lit by a procedural 512 x 256 sun map (tests/env_guide_model.py::procedural_sun_map, bilinear), unguided against guided by that
same image (default grid 256 x 512, alpha 0.5).

usage: python scripts/env_guide_bench.py [steps-per-window] [repeats] [reference-steps]

Time.  One renderer; a window is `steps-per-window` pt_path_trace calls between two host clock readings (the call blocks until
the step is done); unguided and guided windows are taken in turn, the figure is the median over `repeats` windows after a
warm-up window of each.  pt_stats' trace / map stage times of the last step of each kind are printed beside it.
Error.  The film's mean squared error (all pixels, all channels) against a long unguided reference render of `reference-steps`
steps under another seed: one unguided step, one guided step (equal samples), and one guided step with 300 x t_off / t_on
samples (equal time).  The reference's own noise, about MSE_unguided / reference-steps, is inside every figure.  A relative
form, mean((x - ref)^2 / (ref^2 + 0.01)), is printed too: the plain MSE is dominated by the few pixels a sun sample lands in.
Depends on tests/env_guide_model.py (imported as the package `tests` from the repository root) for the map.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipu_path_trace_amd import ptmi  # noqa: E402
from tests import env_guide_model as G  # noqa: E402

W, H, SPP, DEPTH = 1104, 1000, 300, 8


def film(r, rec):
    for k in ("r", "g", "b", "sampleCount", "pathLength"):
        rec[k] = 0                      # pt_setup takes the records' accumulators as they stand: start every film at zero
    r.setup(rec)
    r.path_trace()
    r.read_results(rec)
    n = rec["sampleCount"].astype(np.float64)[:, None]
    return np.stack([rec["b"], rec["g"], rec["r"]], -1).astype(np.float64) / n


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ref_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    img = G.procedural_sun_map()
    rows, cols = ptmi.default_env_guide_grid(img.shape[1], img.shape[0])
    r = ptmi.Renderer(W, H, max_path_length=DEPTH)
    try:
        r.set_env_map(img, "bilinear")
        r.init_render_settings(seed=1, samples_per_step=SPP)
        rec = ptmi.worklist(W, H)
        r.setup(rec)
        ms = {"off": [], "on": []}
        stage = {}
        for rep in range(repeats + 1):
            for name in ("off", "on"):
                r.set_env_guide(img if name == "on" else None)
                t0 = time.perf_counter()
                for _ in range(steps):
                    r.path_trace()
                dt = (time.perf_counter() - t0) * 1e3 / steps
                if rep:   # window 0 warms up
                    ms[name].append(dt)
                st = r.stats()
                stage[name] = (st.path_trace_ms, st.nif_ms, st.accumulate_ms, st.total_ms, st.escaped, st.paths, st.segments)
        t = {k: float(np.median(v)) for k, v in ms.items()}
        print("map %d x %d, guide %d x %d cells, alpha 0.5; image %d x %d, %d spp, depth %d; median of %d windows of %d steps" % (
            img.shape[1], img.shape[0], rows, cols, W, H, SPP, DEPTH, repeats, steps))
        for name, label in (("off", "unguided"), ("on", "guided")):
            s = stage[name]
            print("%-9s step ms %8.3f (windows %s)  last step: trace ms %.3f  map ms %.3f  accumulate ms %.3f  total ms %.3f  "
                  "escaped %d of %d paths, %d segments" % ((label, t[name], " ".join("%.3f" % x for x in ms[name])) + s))
        print("guided / unguided step time %.3f" % (t["on"] / t["off"]))

        # error against a long unguided reference under another seed
        r.set_env_guide(None)
        r.init_render_settings(seed=77, samples_per_step=SPP)
        ref = np.zeros((W * H, 3))
        for _ in range(ref_steps):
            ref += film(r, rec)
        ref /= ref_steps
        spp_eq = max(1, int(round(SPP * t["off"] / t["on"])))
        runs = [("unguided, %d spp" % SPP, None, SPP), ("guided, %d spp (equal samples)" % SPP, img, SPP),
                ("guided, %d spp (equal time)" % spp_eq, img, spp_eq)]
        base = None
        for label, guide, spp in runs:
            r.set_env_guide(guide)
            r.init_render_settings(seed=1, samples_per_step=spp)
            x = film(r, rec)
            mse = float(np.mean((x - ref) ** 2))
            rel = float(np.mean((x - ref) ** 2 / (ref * ref + 0.01)))
            base = base or (mse, rel)
            print("%-34s MSE %.6g (%.2fx lower than unguided)  relative MSE %.6g (%.2fx lower)  film mean %.5f (reference %.5f)" % (
                label, mse, base[0] / mse, rel, base[1] / rel, x.mean(), ref.mean()))
        print("reference: %d unguided steps of %d spp, seed 77; its own noise is about MSE_unguided / %d" % (ref_steps, SPP, ref_steps))
    finally:
        r.close()


if __name__ == "__main__":
    main()
