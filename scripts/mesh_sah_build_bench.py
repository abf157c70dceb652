#!/usr/bin/env python3
"""What a SAH tree built on the device costs (pt_set_mesh_device_tree), against the host builder and the device's linear tree.

usage: python scripts/mesh_sah_build_bench.py [--levels 6,7,8] [--poses N] [--width W] [--height H] [--spp N] [--steps K]
                                              [--update-level 8] [--repeats N] [--verify LEVEL] [--out FILE]                 (GPU)
       python scripts/mesh_sah_build_bench.py --one-build LEVEL        (one device SAH build and nothing else: for a kernel trace)
       python scripts/mesh_sah_build_bench.py --split KERNEL_TRACE.csv  (no GPU: that build's kernel times, per kernel and per level)

1. --verify LEVEL: the device SAH tree of the icosphere of tests/mesh_lbvh_main.cpp at that level against the host builder's bytes
   (the program's --dump, its last tree) -- the tests stop at 5120 triangles.
2. Per icosphere level: the build of one mesh by the host (SAH), by the device (linear) and by the device (SAH), as the library
   reports it (pt_mesh_info.build_ms: host clock for the host builder, HIP events for the device paths): the first build, which
   carries the kernels' first launches, and the median of --poses rebuilds after pose changes; last_levels of the SAH builds.
3. The step time of the mesh scene of scripts/mesh_normals_bench.py under the three, their steps taking
   turns, the first step of each is warm-up; median, and the spread (min .. max) of the timed steps of each leg.  Host SAH and
   device SAH trace the same bytes: their medians should agree within that spread.
4. pt_update_mesh_vertices(mode="rebuild") per update at --update-level under device SAH, device linear and the host builder.
No threshold is fixed here or in a test: the numbers are the finding."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ipu_path_trace_amd import ptmi                  # noqa: E402
from scripts import mesh_build_bench as BB            # noqa: E402  (its icosphere and poses)
from scripts import mesh_normals_bench as NB          # noqa: E402  (its scene)
from scripts import mesh_update_bench as UB           # noqa: E402  (its wobble)

LEGS = (("host SAH", "host", "linear"), ("device linear", "device", "linear"), ("device SAH", "device", "sah"))


def renderer(builder, kind, width=64, height=48, spp=1, depth=4, **more):
    r = ptmi.Renderer(width, height, max_path_length=depth, **more)
    r.set_constant_env(BB.SKY)
    r.init_render_settings(seed=3, samples_per_step=spp)
    if builder != "host":
        r.set_mesh_build(builder, "rebuild")
    if kind != "linear":
        r.set_mesh_device_tree(kind)
    return r


def one_mesh(v, t):
    return [{"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": v, "triangles": t}]


def build_times(level, poses):
    v, t = BB.icosphere(level)
    out = {}
    for name, builder, kind in LEGS:
        r = renderer(builder, kind)
        try:
            r.set_scene(one_mesh(v, t))
            first = r.mesh_info(0)["build_ms"]
            again = []
            for k in range(poses):
                r.set_camera(**BB.POSES[k % len(BB.POSES)])
                BB.up_to_date(r)
                again.append(r.mesh_info(0)["build_ms"])
            out[name] = (first, float(np.median(again)), r.mesh_info(0), r.mesh_device_tree_info(), r.mesh_build_info())
        finally:
            r.close()
    return len(t), out


def step_times(a):
    legs = {}
    for name, builder, kind in LEGS:
        r = renderer(builder, kind, a.width, a.height, a.spp, 8, roulette_depth=3)
        r.set_scene(NB.scene(True))
        rec = ptmi.worklist(a.width, a.height)
        r.setup(rec)
        legs[name] = (r, rec, [])
    names = [n for n, _, _ in LEGS]
    for step in range(a.steps):
        for name in names[step % 3:] + names[:step % 3]:      # the legs take turns to go first
            r, rec, total = legs[name]
            r.path_trace()
            st = r.read_results(rec)
            if step:
                total.append(st.total_ms)
    same = {n: legs[n][1].tobytes() == legs["host SAH"][1].tobytes() for n in names}
    trees = {n: [legs[n][0].mesh_tree(k)[0].tobytes() for k in (0, 1)] == [legs["host SAH"][0].mesh_tree(k)[0].tobytes() for k in (0, 1)] for n in names}
    med = {n: (float(np.median(legs[n][2])), float(np.min(legs[n][2])), float(np.max(legs[n][2]))) for n in names}
    for r, _, _ in legs.values():
        r.close()
    return med, same, trees


def update_times(level, repeats):
    v, t = BB.icosphere(level)
    out = {}
    for name, builder, kind in LEGS:
        r = renderer(builder, kind)
        try:
            r.set_scene(one_mesh(v, t))
            BB.up_to_date(r)
            r.update_mesh_vertices(0, v, mode="rebuild")          # (a scene's first update allocates: not timed)
            tree, wall = [], []
            for k in range(repeats):
                vk = UB.wobble(v, 0.3 * (k + 1))
                t0 = time.perf_counter()
                r.update_mesh_vertices(0, vk, mode="rebuild")
                wall.append(1e3 * (time.perf_counter() - t0))
                info = r.mesh_update_info()
                tree.append(info["last_tree_ms"])
            out[name] = (float(np.median(tree)), float(np.median(wall)), info["rebuilds"], info["fallbacks"])
        finally:
            r.close()
    return len(t), out


def verify(level):
    """The device SAH tree of the test program's icosphere(level) in the world frame against the host builder's bytes."""
    with tempfile.TemporaryDirectory() as tmp:
        exe, path = os.path.join(tmp, "mesh_lbvh"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-I" + os.path.join(ROOT, "tests"), "-o", exe,
                               os.path.join(ROOT, "tests", "mesh_lbvh_main.cpp")])
        subprocess.check_call([exe, "--dump", "icosphere%d" % level, path])
        raw = np.fromfile(path, np.uint32)
    nv, nt, nr = int(raw[1]), int(raw[2]), int(raw[3])
    v = raw[4:4 + 3 * nv].view(np.float32).reshape(-1, 3)
    t = raw[4 + 3 * nv:4 + 3 * nv + 3 * nt].reshape(-1, 3)
    at = 4 + 3 * nv + 3 * nt + 8 * nr + 18          # past the rays, their results and the two cameras: eight trees, the SAH world tree last
    for _ in range(7):
        at += 5 + 8 * int(raw[at]) + nt
    n_nodes, depth = int(raw[at]), int(raw[at + 1])
    want_nodes = raw[at + 5:at + 5 + 8 * n_nodes]
    want_orig = raw[at + 5 + 8 * n_nodes:at + 5 + 8 * n_nodes + nt]
    assert at + 5 + 8 * n_nodes + nt == len(raw)
    r = renderer("device", "sah")
    try:
        r.set_scene(one_mesh(v, t))
        nodes, orig = r.mesh_tree(0)
        info, tree = r.mesh_info(0), r.mesh_device_tree_info()
    finally:
        r.close()
    same = len(nodes) == n_nodes and np.array_equal(nodes.view(np.uint32).reshape(-1), want_nodes) and np.array_equal(orig, want_orig) and info["depth"] == depth
    return "verify: icosphere level %d, %d triangles, %d nodes, depth %d, %d levels: the device SAH tree %s the host builder's, byte for byte" % (
        level, nt, n_nodes, depth, tree["last_levels"], "EQUALS" if same else "DIFFERS FROM")


def split(path):
    """A kernel trace (rocprofv3 --kernel-trace, CSV) of --one-build: the builder's kernel times per kernel and per level.  A level
    begins at its first sah_clear / sah_bounds / sah_split dispatch after a partition."""
    import csv
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].split("::")[-1]) for r in csv.DictReader(open(path))]
    rows = sorted(r for r in rows if r[2].startswith("sah_") or r[2].startswith("lbvh_"))
    per_kernel, levels, tail, seen_partition = {}, [], 0.0, True
    for start, end, name in rows:
        us = (end - start) / 1e3
        n, total = per_kernel.get(name, (0, 0.0))
        per_kernel[name] = (n + 1, total + us)
        if name in ("sah_clear_kernel", "sah_bounds_kernel", "sah_bins_kernel", "sah_split_kernel", "sah_flags_kernel", "sah_scan_sums_kernel", "sah_partition_kernel"):
            if seen_partition and name != "sah_partition_kernel":
                levels.append(0.0)
                seen_partition = False
            levels[-1] += us
            seen_partition = seen_partition or name == "sah_partition_kernel"
        elif levels:
            tail += us
    lines = ["kernel time of one device SAH build, %.3f ms in %d dispatches (%.3f ms from the first kernel's start to the last one's end):" % (
        sum(t for _, t in per_kernel.values()) / 1e3, sum(n for n, _ in per_kernel.values()), (rows[-1][1] - rows[0][0]) / 1e6)]
    for name, (n, total) in sorted(per_kernel.items(), key=lambda kv: -kv[1][1]):
        lines.append("  %-24s %4d dispatches %10.1f us" % (name, n, total))
    lines.append("  per level (clear, bounds, bins, split, flags, scan, partition), us: " + " ".join("%.0f" % x for x in levels))
    lines.append("  after the last level (count, emit, slots, the box pass): %.0f us" % tail)
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="6,7,8")
    ap.add_argument("--poses", type=int, default=3)
    ap.add_argument("--width", type=int, default=1104)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--update-level", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--verify", type=int, default=0)
    ap.add_argument("--one-build", type=int, default=0)
    ap.add_argument("--split")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.split:
        print(split(a.split))
        return
    if a.one_build:
        v, t = BB.icosphere(a.one_build)
        r = renderer("device", "sah")
        r.set_scene(one_mesh(v, t))
        print("one build: %d triangles, %.3f ms, %d levels" % (len(t), r.mesh_info(0)["build_ms"], r.mesh_device_tree_info()["last_levels"]))
        r.close()
        return
    lines = ["mesh_sah_build_bench: one icosphere per level; build_ms as the library reports it (host clock / HIP events); rebuilds after a pose change, median of %d" % a.poses]
    if a.verify:
        lines.append(verify(a.verify))
    for level in [int(x) for x in a.levels.split(",") if x]:
        T, out = build_times(level, a.poses)
        tree = out["device SAH"][3]
        lines.append("level %d, %d triangles (device SAH: %d levels, %.1f MiB for its arrays, %.1f bytes per triangle):" % (
            level, T, tree["last_levels"], tree["device_bytes"] / 2.0 ** 20, tree["device_bytes"] / T))
        for name, _, _ in LEGS:
            first, again, m, _, info = out[name]
            lines.append("  %-13s first build %10.3f ms; rebuild %10.3f ms  (%d nodes, depth %d; %d host + %d device builds)" % (
                name, first, again, m["n_nodes"], m["depth"], info["host_builds"], info["device_builds"]))
        lines.append("  host SAH / device SAH: %.1f x; device SAH / device linear: %.1f x (rebuilds)" % (
            out["host SAH"][1] / out["device SAH"][1], out["device SAH"][1] / out["device linear"][1]))
    if a.steps > 1:
        med, same, trees = step_times(a)
        lines.append("step: %d x %d, %d spp, depth 8, constant sky, ball 20480 + field 8192 triangles with normals, %d timed steps per leg" % (
            a.width, a.height, a.spp, a.steps - 1))
        for name, _, _ in LEGS:
            lines.append("  %-13s %8.3f ms/step (min %8.3f, max %8.3f); accumulators %s, trees %s the host's" % (
                name, med[name][0], med[name][1], med[name][2], "bit-identical" if same[name] else "DIFFER", "equal" if trees[name] else "differ from"))
        lines.append("  device SAH / host SAH: %.4f; device linear / host SAH: %.3f" % (
            med["device SAH"][0] / med["host SAH"][0], med["device linear"][0] / med["host SAH"][0]))
    if a.update_level:
        T, out = update_times(a.update_level, a.repeats)
        lines.append("pt_update_mesh_vertices(mode=rebuild), level %d, %d triangles, host memory, median of %d:" % (a.update_level, T, a.repeats))
        for name, _, _ in LEGS:
            tree, wall, rebuilds, fallbacks = out[name]
            lines.append("  %-13s tree pass %10.3f ms, wall clock %10.3f ms  (%d rebuilds, %d fallbacks)" % (name, tree, wall, rebuilds, fallbacks))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
