#!/usr/bin/env python3
"""What a mesh tree costs to build and to refit, on the host and on the device (pt_set_mesh_build), and what the linear tree costs
the trace.

usage: python scripts/mesh_build_bench.py [--levels 6,7,8] [--width W] [--height H] [--spp N] [--steps K] [--out FILE]      (GPU)

1. Per icosphere level: the host (SAH) build, the device (linear BVH) build and the refit of one mesh, as the library reports them
   (pt_mesh_info.build_ms: host clock for the host builder, HIP events for the device paths), and a pose change END TO END -- the
   wall clock from pt_set_camera until the trees are valid again (pt_mesh_tree with nothing to copy) -- for each of the four option
   pairs, the median of --poses changes.
2. The step time of the mesh scene of scripts/mesh_normals_bench.py (a 20480-triangle glass ball with normals over an 8192-triangle
   height field, constant sky) with the SAH tree against the linear tree: two handles, their steps taking turns, the first step
   of each is warm-up.  A slower step under the linear tree is the documented trade, not a failure.
3. --verify LEVEL: the device builder's tree of the icosphere of tests/mesh_lbvh_main.cpp at that level against the CPU reference
   builder's (the program's --dump), byte for byte -- the tests stop at 5120 triangles, this goes where the sort has many tiles.
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

from ipu_path_trace_amd import ptmi                 # noqa: E402
from tests import scene_mesh_model as MM             # noqa: E402
from scripts import mesh_normals_bench as NB         # noqa: E402  (its scene)

SKY = (0.75, 1.5, 3.0)
POSES = [dict(position=(0.3, 0.14, 0.4), look_at=(0.04, -0.06, -0.6), up=(0.1, 1.0, 0.2)),
         dict(position=(-0.25, 0.1, 0.2), look_at=(0.0, -0.05, -0.55), up=(0.3, 1.0, 0.1)),
         dict(position=(0.1, 0.3, -1.3), look_at=(0.0, -0.05, -0.55), up=(0.0, 1.0, 0.0))]


def icosphere(level, radius=0.18, centre=(0.0, 0.0, -0.6)):
    """MM.icosphere's sphere, subdivided with numpy (level 8 has 1.3 M triangles)."""
    v, f = MM.icosphere(0, 1.0, (0.0, 0.0, 0.0))
    f = f.astype(np.int64)
    for _ in range(level):
        n = len(f)
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(e[:, 0] * len(v) + e[:, 1], return_inverse=True)
        mid = len(v) + inv.reshape(-1)
        v = np.concatenate([v, 0.5 * (v[uniq // len(v)] + v[uniq % len(v)])])
        ab, bc, ca = mid[:n], mid[n:2 * n], mid[2 * n:]
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * radius + np.asarray(centre)
    return np.float32(v), np.uint32(f)


def up_to_date(r):
    r._check(r._lib.pt_mesh_tree(r.handle, 0, None, 0, None, 0))


def build_times(level, poses):
    v, t = icosphere(level)
    mesh = [{"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": v, "triangles": t}]
    out = {}
    for builder in ("host", "device"):
        for on_pose in ("rebuild", "refit"):
            r = ptmi.Renderer(64, 48, max_path_length=4)
            try:
                r.set_constant_env(SKY)
                r.init_render_settings(seed=3, samples_per_step=1)
                if (builder, on_pose) != ("host", "rebuild"):
                    r.set_mesh_build(builder, on_pose)
                r.set_scene(mesh)
                first = r.mesh_info(0)["build_ms"]
                wall, reported = [], []
                for k in range(poses):
                    t0 = time.perf_counter()
                    r.set_camera(**POSES[k % len(POSES)])
                    up_to_date(r)
                    wall.append(1e3 * (time.perf_counter() - t0))
                    reported.append(r.mesh_info(0)["build_ms"])
                info = r.mesh_build_info()
                out[(builder, on_pose)] = (first, float(np.median(reported)), float(np.median(wall)), info, r.mesh_info(0))
            finally:
                r.close()
    return len(t), out


def step_times(a):
    legs = {}
    for builder in ("host", "device"):
        r = ptmi.Renderer(a.width, a.height, max_path_length=8, roulette_depth=3)
        r.set_constant_env(SKY)
        r.init_render_settings(seed=3, samples_per_step=a.spp)
        r.set_mesh_build(builder, "rebuild")
        r.set_scene(NB.scene(True))
        rec = ptmi.worklist(a.width, a.height)
        r.setup(rec)
        legs[builder] = (r, rec, [], [])
    for step in range(a.steps):
        for builder in ("host", "device") if step % 2 == 0 else ("device", "host"):      # the legs take turns to go first
            r, rec, total, trace = legs[builder]
            r.path_trace()
            st = r.read_results(rec)
            if step:
                total.append(st.total_ms)
                trace.append(st.path_trace_ms)
    same = legs["host"][1].tobytes() == legs["device"][1].tobytes()
    med = {b: (float(np.median(legs[b][2])), float(np.median(legs[b][3])), [legs[b][0].mesh_info(k)["n_nodes"] for k in (0, 1)]) for b in legs}
    for r, _, _, _ in legs.values():
        r.close()
    return med, same


def verify(level):
    """The device tree of the test program's icosphere(level) in the world frame against the reference builder's bytes."""
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
    at = 4 + 3 * nv + 3 * nt + 8 * nr + 18          # past the rays, their results and the two cameras: the world linear tree
    n_nodes = int(raw[at])
    want_nodes = raw[at + 5:at + 5 + 8 * n_nodes]
    want_orig = raw[at + 5 + 8 * n_nodes:at + 5 + 8 * n_nodes + nt]
    r = ptmi.Renderer(64, 48, max_path_length=4)
    try:
        r.set_constant_env(SKY)
        r.init_render_settings(seed=3, samples_per_step=1)
        r.set_mesh_build("device", "rebuild")
        r.set_scene([{"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": v, "triangles": t}])
        nodes, orig = r.mesh_tree(0)
    finally:
        r.close()
    same = len(nodes) == n_nodes and np.array_equal(nodes.view(np.uint32).reshape(-1), want_nodes) and np.array_equal(orig, want_orig)
    return "verify: icosphere level %d, %d triangles, %d nodes: the device tree %s the CPU reference builder's, byte for byte" % (
        level, nt, n_nodes, "EQUALS" if same else "DIFFERS FROM")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="6,7,8")
    ap.add_argument("--poses", type=int, default=3)
    ap.add_argument("--width", type=int, default=1104)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--verify", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["mesh_build_bench: one icosphere per level; build_ms as the library reports it, pose change = wall clock of pt_set_camera + pt_mesh_tree, median of %d" % a.poses]
    for level in [int(x) for x in a.levels.split(",") if x]:
        T, out = build_times(level, a.poses)
        info = out[("device", "rebuild")][3]
        lines.append("level %d, %d triangles (sort_on_device %d, %.1f MiB held for the device paths):" % (level, T, info["sort_on_device"], info["device_bytes"] / 2.0 ** 20))
        for key in (("host", "rebuild"), ("host", "refit"), ("device", "rebuild"), ("device", "refit")):
            first, again, wall, info, m = out[key]
            lines.append("  %-6s + %-7s first build %9.3f ms; on a pose change %9.3f ms reported, %9.3f ms end to end  (%d nodes, depth %d; %d builds, %d refits)" % (
                key[0], key[1], first, again, wall, m["n_nodes"], m["depth"], info["host_builds"] + info["device_builds"], info["refits"]))
    if a.steps > 1:
        med, same = step_times(a)
        lines.append("step: %d x %d, %d spp, depth 8, constant sky, ball 20480 + field 8192 triangles with normals, %d timed steps per leg; accumulators %s" % (
            a.width, a.height, a.spp, a.steps - 1, "bit-identical" if same else "DIFFER"))
        for b, name in (("host", "SAH"), ("device", "linear")):
            lines.append("  %-6s tree (%d + %d nodes) %8.3f ms/step, trace stage %8.3f ms" % (name, med[b][2][0], med[b][2][1], med[b][0], med[b][1]))
        lines.append("  linear / SAH: step %.3f, trace stage %.3f" % (med["device"][0] / med["host"][0], med["device"][1] / med["host"][1]))
    if a.verify:
        lines.append(verify(a.verify))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
