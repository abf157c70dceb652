#!/usr/bin/env python3
"""Polygon lamps in the emitter guide (pt_set_light_guide_ex, PT_LIGHT_GUIDE_POLYGONS): the resource rows of the six new kernel
instances, what a Cornell box gains from them, and what they cost a user who never sets the flag.

usage: python scripts/light_guide_polygon_bench.py resources [--remarks FILE] [--baseline-remarks FILE] [--out FILE]   (no GPU)
       python scripts/light_guide_polygon_bench.py time [--baseline-tree DIR] [--runs N] [--out FILE]                  (GPU)
       python scripts/light_guide_polygon_bench.py measure LEG                                                         (one run, one JSON line)

resources  the compiler's resource row (-Rpass-analysis=kernel-resource-usage) of every light-guided kernel; --remarks takes the
           compiler's stderr of an earlier compilation of this tree instead of compiling again.  With --baseline-remarks (the same
           of the parent commit) it says whether every kernel of the parent kept its row.
time       cornell (tests/scene_poly_model.py's box, its only lamp the ceiling parallelogram) at 1104 x 1000 x 64 spp, depth 8,
           constant sky, guide off and on (beta 0.5): milliseconds per step, the per-pixel variance of a step mean over STEPS
           steps (its mean over the pixels and the median pixel's), the variance ratio off / on and ratio / time ratio as the
           efficiency gain; the same again under a dim sky (0.05), where the lamp is the main light.  Then the built-in scene's step
           with this tree and, with --baseline-tree (a checkout of the parent with its library built), with the parent's library,
           the legs taking turns to go first: information, the gate being that the parent's kernels keep their instructions.
Every figure goes to stdout and, with --out, is appended to that file.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, REPEATS, STEPS = 1104, 1000, 64, 8, 5, 6
BETA = 0.5
DIM_SKY = 0.05          # the second pair of legs: the box under a sky that leaves the lamp the main light
KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]")


def rows_of(text):
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.rsplit(":", 1)
            rows[cur][k.strip()] = v.strip()
    return rows


def resources(args, emit):
    if args.remarks:
        new = rows_of(open(args.remarks, errors="replace").read())
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
               "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"),
               "-o", "OUT", os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "ptmi.hip"), "-Rpass-analysis=kernel-resource-usage"]
        with tempfile.TemporaryDirectory() as tmp:             # the library itself is not wanted, only the compiler's remarks
            cmd[cmd.index("OUT")] = os.path.join(tmp, "libptmi_remarks.so")
            new = rows_of(subprocess.run(cmd, capture_output=True, text=True, check=True).stderr)
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.split("(")[0].strip()   # noqa: E731
    emit("kernel resource rows (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): SGPR VGPR AGPR scratch occupancy spillS spillV LDS")
    for name, r in new.items():
        short = demangle(name)
        if "lights" in short or "light_guide" in short:
            emit("  %-44s %s" % (short.replace("ptd::", ""), " ".join("%4s" % r.get(k, "?") for k in KEYS)))
    if args.baseline_remarks:
        old = rows_of(open(args.baseline_remarks, errors="replace").read())
        moved = [demangle(k) for k in old if new.get(k) != old[k]]
        emit("kernels of the parent: %d; of this tree: %d; new: %s" % (len(old), len(new), ", ".join(
            demangle(k).replace("ptd::", "") for k in new if k not in old)))
        emit("parent kernels whose row changed: %s" % (", ".join(moved) if moved else "none"))
        return 1 if moved else 0
    return 0


def measure(leg):
    """One process, one renderer.  builtin: a warm-up step and REPEATS timed ones.  cornell_off / cornell_on: the same, then
    STEPS steps read back for the per-pixel variance of a step mean."""
    import numpy as np
    from ipu_path_trace_amd import ptmi
    r = ptmi.Renderer(W, H, max_path_length=DEPTH)
    try:
        sky = DIM_SKY if "dim" in leg else 1.0
        r.set_constant_env((sky, sky, sky))
        r.init_render_settings(samples_per_step=SPP)
        if leg != "builtin":
            from tests import scene_poly_model as PM
            r.set_scene(PM.world_scene("cornell", "none"))
            if leg.endswith("_on"):
                r.set_light_guide(BETA, polygons=True)
        rec = ptmi.worklist(W, H)
        r.setup(rec)
        trace, total = [], []
        for rep in range(REPEATS + 1):
            r.path_trace()
            st = r.stats()
            if rep:
                trace.append(st.path_trace_ms)
                total.append(st.total_ms)
        out = {"leg": leg, "trace_ms": float(np.median(trace)), "step_ms": float(np.median(total)), "paths": int(st.paths),
               "segments_per_path": st.segments / st.paths}
        if leg != "builtin":
            s1, s2 = np.zeros((len(rec), 3)), np.zeros((len(rec), 3))
            for _ in range(STEPS):
                r.setup(rec)
                r.path_trace()
                r.read_results(rec)
                m = np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64) / SPP
                s1 += m
                s2 += m * m
            var = (s2 - s1 * s1 / STEPS) / (STEPS - 1)
            out["pixel_variance"] = float(var.mean())
            out["pixel_variance_median"] = float(np.median(var.mean(axis=1)))   # the mean is a few pixels' (glass paths that grow by 1.15 rr a bounce)
            out["mean"] = [float(x) for x in (s1 / STEPS).mean(axis=0)]
            out["emitters"] = int(r.light_guide_info()["n_lights"])
        print(json.dumps(out))
    finally:
        r.close()


def run_child(tree, leg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", leg, "--tree", tree], capture_output=True,
                         text=True, timeout=600, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def compare(emit, off, on):
    if "dim" in off["leg"]:
        emit("the same under a constant sky of %.2f" % DIM_SKY)
    for x in (off, on):
        emit("  %-15s step ms %.3f  trace ms %.3f  segments / path %.3f  per-pixel variance: mean %.6g median %.6g  film mean %s  emitters listed %d" % (
            x["leg"], x["step_ms"], x["trace_ms"], x["segments_per_path"], x["pixel_variance"], x["pixel_variance_median"],
            " ".join("%.5f" % m for m in x["mean"]), x["emitters"]))
    cost = on["step_ms"] / off["step_ms"]
    for what, key in (("mean over the pixels", "pixel_variance"), ("median pixel", "pixel_variance_median")):
        ratio = off[key] / on[key]
        emit("  %s: variance off / on %.3f, step time on / off %.3f, efficiency gain (variance ratio / time ratio) %.3f" % (what, ratio, cost, ratio / cost))


def time_(args, emit):
    import numpy as np
    emit("cornell, %d x %d x %d spp, depth %d, constant sky of 1, beta %.2f; each figure the median of %d steps, variance over %d steps" % (
        W, H, SPP, DEPTH, BETA, REPEATS, STEPS))
    for pair in (("cornell_off", "cornell_on"), ("cornell_dim_off", "cornell_dim_on")):
        compare(emit, run_child(ROOT, pair[0]), run_child(ROOT, pair[1]))
    legs = [("this", ROOT)] + ([("parent", os.path.abspath(args.baseline_tree))] if args.baseline_tree else [])
    got = {who: [] for who, _ in legs}
    for k in range(args.runs):
        for who, tree in (legs if k % 2 == 0 else legs[::-1]):
            got[who].append(run_child(tree, "builtin"))
    emit("the built-in scene, same shape, %d processes per leg taking turns to go first (information; the gate is instruction identity)" % args.runs)
    for who, runs in got.items():
        emit("  %-6s trace ms %s  step ms %s  (median step %.3f)" % (who, " ".join("%.3f" % x["trace_ms"] for x in runs),
                                                                  " ".join("%.3f" % x["step_ms"] for x in runs), np.median([x["step_ms"] for x in runs])))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["resources", "time", "measure"])
    ap.add_argument("leg", nargs="?", default="builtin", choices=["builtin", "cornell_off", "cornell_on", "cornell_dim_off", "cornell_dim_on"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline-tree")
    ap.add_argument("--remarks")
    ap.add_argument("--baseline-remarks")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.mode == "measure":
        sys.path.insert(0, os.path.abspath(args.tree))
        measure(args.leg)
        return 0

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return resources(args, emit) if args.mode == "resources" else time_(args, emit)


if __name__ == "__main__":
    sys.exit(main())
