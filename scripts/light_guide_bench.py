#!/usr/bin/env python3
"""Emitter-guided diffuse sampling (pt_set_light_guide) measured on the C2 shape: 1104x1000, 300 spp, depth 8, the built-in
objects plus one small sphere lamp (radius 0.15, radiance 400) above them, under a dim constant sky (0.02), unguided against
guided at beta 0.5.

usage: python scripts/light_guide_bench.py [steps-per-window] [repeats] [reference-steps]

Time.  One renderer; a window is `steps-per-window` pt_path_trace calls between two host clock readings (the call blocks until
the step is done); unguided and guided windows are taken in turn, the figure is the median over `repeats` windows after a
warm-up window of each.  pt_stats' trace stage time of the last step of each kind is printed beside it.
The grid.  The light-guided instances are held to 80 VGPRs so that all six workgroups per CU of the grid are resident (DESIGN.md
section 4.12; left alone they took 83-84 and the last sixth of the grid ran late).  The profiling build can size the grid
(PTMI_TRACE_BLOCKS): the guided step is timed there at 6 and at 5 workgroups per CU as a check that six is no slower.
Error.  The film's mean squared error (all pixels, all channels) against a long unguided reference render of `reference-steps`
steps under another seed: one unguided step, one guided step (equal samples), and one guided step with 300 x t_off / t_on
samples (equal time).  The reference's own noise, about MSE_unguided / reference-steps, is inside every figure.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipu_path_trace_amd import ptmi  # noqa: E402

W, H, SPP, DEPTH = 1104, 1000, 300, 8
SKY, BETA = 0.02, 0.5
LAMP = dict(shape="sphere", material="emissive", centre=(0.5, 1.6, -3.5), radius=0.15, colour=(400.0, 400.0, 400.0))


def scene():
    return [dict(shape=int(o["shape"]), material=int(o["material"]), centre=tuple(o["centre"]), radius=float(o["radius"]),
                 normal=tuple(o["normal"]), colour=tuple(o["colour"])) for o in ptmi.builtin_scene()] + [LAMP]


def film(r, rec):
    for k in ("r", "g", "b", "sampleCount", "pathLength"):
        rec[k] = 0                      # pt_setup takes the records' accumulators as they stand: start every film at zero
    r.setup(rec)
    r.path_trace()
    r.read_results(rec)
    n = rec["sampleCount"].astype(np.float64)[:, None]
    return np.stack([rec["b"], rec["g"], rec["r"]], -1).astype(np.float64) / n


def renderer(diag=False):
    r = ptmi.Renderer(W, H, max_path_length=DEPTH, diag=diag)
    r.set_constant_env((SKY, SKY, SKY))
    r.init_render_settings(seed=1, samples_per_step=SPP)
    r.set_scene(scene())
    return r


def windows(r, rec, steps, repeats, kinds):
    ms = {name: [] for name, _ in kinds}
    stage = {}
    r.setup(rec)
    for rep in range(repeats + 1):
        for name, beta in kinds:
            r.set_light_guide(beta)
            t0 = time.perf_counter()
            for _ in range(steps):
                r.path_trace()
            dt = (time.perf_counter() - t0) * 1e3 / steps
            if rep:   # window 0 warms up
                ms[name].append(dt)
            st = r.stats()
            stage[name] = (st.path_trace_ms, st.total_ms, st.escaped, st.paths, st.segments)
    return {k: float(np.median(v)) for k, v in ms.items()}, ms, stage


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ref_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    rec = ptmi.worklist(W, H)
    r = renderer()
    try:
        t, ms, stage = windows(r, rec, steps, repeats, (("off", None), ("on", BETA)))
        r.set_light_guide(BETA)
        info = r.light_guide_info()
        print("built-in objects + a sphere lamp r %.2f, sky %.2f, beta %.2f (%d emitter, active %s); image %d x %d, %d spp, depth %d; "
              "median of %d windows of %d steps" % (LAMP["radius"], SKY, BETA, info["n_lights"], info["active"], W, H, SPP, DEPTH, repeats, steps))
        for name, label in (("off", "unguided"), ("on", "guided")):
            print("%-9s step ms %8.3f (windows %s)  last step: trace ms %.3f  total ms %.3f  escaped %d of %d paths, %d segments" % (
                (label, t[name], " ".join("%.3f" % x for x in ms[name])) + stage[name]))
        print("guided / unguided step time %.3f" % (t["on"] / t["off"]))

        # error against a long unguided reference under another seed
        r.set_light_guide(None)
        r.init_render_settings(seed=77, samples_per_step=SPP)
        ref = np.zeros((W * H, 3))
        for _ in range(ref_steps):
            ref += film(r, rec)
        ref /= ref_steps
        spp_eq = max(1, int(round(SPP * t["off"] / t["on"])))
        runs = [("unguided, %d spp" % SPP, None, SPP), ("guided, %d spp (equal samples)" % SPP, BETA, SPP),
                ("guided, %d spp (equal time)" % spp_eq, BETA, spp_eq)]
        base = None
        for label, beta, spp in runs:
            r.set_light_guide(beta)
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

    # the light-guided grid at 6 and 5 workgroups per CU, on the profiling build (the only one that reads PTMI_TRACE_BLOCKS)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for per_cu in (6, 5):
            os.environ["PTMI_TRACE_BLOCKS"] = str(per_cu * cus)
            r = renderer(diag=True)
            try:
                t, ms, stage = windows(r, rec, steps, repeats, (("on", BETA),))
                print("profiling build, %d workgroups per CU (%d): guided step ms %8.3f (windows %s), trace ms %.3f" % (
                    per_cu, per_cu * cus, t["on"], " ".join("%.3f" % x for x in ms["on"]), stage["on"][0]))
            finally:
                r.close()
    finally:
        os.environ.pop("PTMI_TRACE_BLOCKS", None)


if __name__ == "__main__":
    main()
