#!/usr/bin/env python3
"""Cost of polygons in runtime scenes (pt_set_scene_ex): resource rows of the kernel instances, the trace-stage and step time of
a Cornell box against the built-in scene, and the gate -- what the change costs a user who never calls pt_set_scene_ex.

usage: python scripts/polygon_bench.py resources [--baseline-remarks FILE] [--out FILE]     (no GPU: compiles with remarks)
       python scripts/polygon_bench.py time [--baseline-tree DIR] [--runs N] [--out FILE]    (GPU)
       python scripts/polygon_bench.py measure SCENE                                         (one run, one JSON line; used by `time`)

resources  compiles csrc/ptmi.hip with -Rpass-analysis=kernel-resource-usage and prints the rows of every trace, trace-paths and
           feature kernel.  With --baseline-remarks (the compiler's stderr of the same compilation of the parent commit) it also
           says whether every kernel the parent has kept its row.
time       one step of 1104 x 1000 x 64 spp at depth 8 under a constant sky (the C2 shape), in a fresh process per run:
           `builtin` and `cornell` (tests/scene_poly_model.py's box, eleven objects) with this tree, and with --baseline-tree (a
           checkout of the parent commit with its library built) `builtin` with that tree, the two built-in legs interleaved and taking turns to go first.  The gate: the
           median of this tree's built-in trace-stage time is not above the parent's by more than the parent's own spread
           (max - min of its runs).  Same box, same session: boxes differ by 5-7 %.
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
W, H, SPP, DEPTH, REPEATS = 1104, 1000, 64, 8, 5
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
        if any(s in short for s in ("trace_kernel", "trace_paths", "features_kernel")):
            emit("  %-44s %s" % (short.replace("ptd::", ""), " ".join("%4s" % r.get(k, "?") for k in KEYS)))
    if args.baseline_remarks:
        old = rows_of(open(args.baseline_remarks, errors="replace").read())
        moved = [demangle(k) for k in old if new.get(k) != old[k]]
        emit("kernels of the parent: %d; of this tree: %d; parent kernels whose row changed: %s" % (
            len(old), len(new), ", ".join(moved) if moved else "none"))
        return 1 if moved else 0
    return 0


def measure(scene):
    """One process, one renderer: a warm-up step and REPEATS timed ones; the medians as one JSON line."""
    import numpy as np
    from ipu_path_trace_amd import ptmi
    r = ptmi.Renderer(W, H, max_path_length=DEPTH)
    try:
        r.set_constant_env((1, 1, 1))
        r.init_render_settings(samples_per_step=SPP)
        if scene == "cornell":
            from tests import scene_poly_model as PM
            r.set_scene(PM.world_scene("cornell", "none"))
        rec = ptmi.worklist(W, H)
        r.setup(rec)
        trace, total = [], []
        for rep in range(REPEATS + 1):
            r.path_trace()
            st = r.stats()
            if rep:
                trace.append(st.path_trace_ms)
                total.append(st.total_ms)
        print(json.dumps({"scene": scene, "trace_ms": float(np.median(trace)), "step_ms": float(np.median(total)),
                          "paths": int(st.paths), "segments_per_path": st.segments / st.paths, "escaped": int(st.escaped)}))
    finally:
        r.close()


def run_child(tree, scene):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", scene, "--tree", tree], capture_output=True,
                         text=True, timeout=300, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def time_(args, emit):
    import numpy as np
    legs = [("this", ROOT, "builtin"), ("this", ROOT, "cornell")]
    if args.baseline_tree:
        legs.insert(1, ("parent", os.path.abspath(args.baseline_tree), "builtin"))
    got = {(who, scene): [] for who, _, scene in legs}
    gate = [leg for leg in legs if leg[2] == "builtin"]
    for k in range(args.runs):
        # the two built-in legs interleaved, and who goes first alternates: the device's drift, and whatever the process before
        # left behind, weigh on both alike (the box's ten-times-longer steps run afterwards, not in between)
        for who, tree, scene in (gate if k % 2 == 0 else gate[::-1]):
            got[(who, scene)].append(run_child(tree, scene))
    for _ in range(args.runs):
        got[("this", "cornell")].append(run_child(ROOT, "cornell"))
    emit("one step of %d x %d x %d spp, depth %d, constant sky; %d processes per leg, each the median of %d steps" % (
        W, H, SPP, DEPTH, args.runs, REPEATS))
    for (who, scene), runs in got.items():
        emit("  %-6s %-8s trace ms %s  step ms %s  segments / path %.3f" % (
            who, scene, " ".join("%.3f" % x["trace_ms"] for x in runs), " ".join("%.3f" % x["step_ms"] for x in runs),
            runs[0]["segments_per_path"]))
    b = np.median([x["trace_ms"] for x in got[("this", "builtin")]])
    c = np.median([x["trace_ms"] for x in got[("this", "cornell")]])
    emit("  cornell / builtin trace-stage time: %.2f (the box keeps every path inside: more segments per path, eleven objects per trip)" % (c / b))
    if args.baseline_tree:
        p = [x["trace_ms"] for x in got[("parent", "builtin")]]
        spread = max(p) - min(p)
        ok = b <= np.median(p) + spread
        emit("  gate: this tree's median %.3f ms against the parent's %.3f ms + its spread %.3f ms: %s" % (
            b, np.median(p), spread, "passes" if ok else "FAILS"))
        return 0 if ok else 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["resources", "time", "measure"])
    ap.add_argument("scene", nargs="?", default="builtin", choices=["builtin", "cornell"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline-tree")
    ap.add_argument("--baseline-remarks")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.mode == "measure":
        sys.path.insert(0, os.path.abspath(args.tree))
        measure(args.scene)
        return 0

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return resources(args, emit) if args.mode == "resources" else time_(args, emit)


if __name__ == "__main__":
    sys.exit(main())
