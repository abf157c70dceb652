#!/usr/bin/env python3
"""What moving a mesh costs (pt_update_mesh_vertices), against setting the scene again, and what successive refits cost the trace.

usage: python scripts/mesh_update_bench.py [--levels 6,8] [--width W] [--height H] [--spp N] [--steps K] [--refits N] [--out FILE]   (GPU)

1. Per icosphere level (8: the 1.3 M triangles of DESIGN.md section 4.20), one smooth mesh: the time of an update, split as the
   library reports it into the frames (copy, check, commit: pt_mesh_update_info.last_frames_ms) and the tree pass (last_tree_ms),
   and its wall clock, for REFIT (host-built topology) and for REBUILD under the device builder, from host memory and from a torch
   tensor on the device; beside it the only other route, pt_set_scene_meshes + pt_set_mesh_normals with the same vertices on the
   same handle, wall clock.  The legs take turns; medians of --repeats.
2. The 28 672-triangle scene of scripts/mesh_normals_bench.py: its glass ball is twisted about its axis a
   little further with every update.  One handle REFITs, one REBUILDs the same vertices (both under the host builder: SAH
   topology); after each update both take --steps steps in turns.  The ratio is the refit's tree quality.
No threshold is fixed here or in a test: the numbers are the finding."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ipu_path_trace_amd import ptmi                  # noqa: E402
from scripts import mesh_build_bench as BB            # noqa: E402  (its icosphere)
from scripts import mesh_normals_bench as NB          # noqa: E402  (its scene)

SKY = (0.75, 1.5, 3.0)


def wobble(v, phase):
    v = np.float32(v)
    return np.ascontiguousarray(v + np.float32(0.01) * np.sin(np.float32(25.0) * v[:, [1, 2, 0]] + np.float32(phase)))


def normals_of(v, centre):
    n = v.astype(np.float64) - np.asarray(centre)
    return np.ascontiguousarray(np.float32(n / np.linalg.norm(n, axis=1)[:, None]))


def update_times(level, repeats):
    import torch
    centre = (0.0, 0.0, -0.6)
    v, t = BB.icosphere(level, centre=centre)
    lines = []
    legs = {}
    for name, builder, mode in (("refit", "host", "refit"), ("device rebuild", "device", "rebuild")):
        r = ptmi.Renderer(64, 48, max_path_length=4)
        r.set_constant_env(SKY)
        r.init_render_settings(seed=3, samples_per_step=1)
        r.set_mesh_build(builder)
        r.set_scene([{"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": v, "triangles": t, "normals": normals_of(v, centre)}])
        BB.up_to_date(r)
        legs[name] = (r, mode, {"frames": [], "tree": [], "wall": [], "wall_device": [], "scene": []})
    for k in range(repeats + 1):
        vk = wobble(v, 0.3 * k)
        nk = normals_of(vk, centre)
        tv, tn = torch.from_numpy(vk).cuda(), torch.from_numpy(nk).cuda()
        torch.cuda.synchronize()
        for name in (list(legs) if k % 2 == 0 else list(legs)[::-1]):
            r, mode, out = legs[name]
            t0 = time.perf_counter()
            r.set_scene([{"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": vk, "triangles": t, "normals": nk}])
            BB.up_to_date(r)
            scene = 1e3 * (time.perf_counter() - t0)
            r.update_mesh_vertices(0, v, mode=mode)          # (a scene's first update allocates: not timed)
            t0 = time.perf_counter()
            r.update_mesh_vertices(0, vk, normals=nk, mode=mode)
            wall = 1e3 * (time.perf_counter() - t0)
            info = r.mesh_update_info()
            t0 = time.perf_counter()
            r.update_mesh_vertices(0, tv, normals=tn, mode=mode)
            wall_device = 1e3 * (time.perf_counter() - t0)
            if k:   # (the first round is warm-up)
                for key, x in (("frames", info["last_frames_ms"]), ("tree", info["last_tree_ms"]), ("wall", wall), ("wall_device", wall_device), ("scene", scene)):
                    out[key].append(x)
    for name, (r, mode, out) in legs.items():
        m = {k: float(np.median(x)) for k, x in out.items()}
        lines.append("  %-14s frames %8.3f ms + tree %8.3f ms; wall clock %9.3f ms from host memory, %9.3f ms from a device tensor; "
                     "set_scene + set_mesh_normals + build %10.3f ms (%.0f x)" % (name, m["frames"], m["tree"], m["wall"], m["wall_device"], m["scene"], m["scene"] / m["wall_device"]))
        r.close()
    return len(t), lines


def twist(v, centre, radius, amount):
    """The ball turned about the vertical axis through its centre by an angle that grows with height: amount = turns end to end."""
    c = np.asarray(centre, np.float64)
    p = v.astype(np.float64) - c
    a = 2.0 * np.pi * amount * p[:, 1] / (2.0 * radius)
    x, z = p[:, 0] * np.cos(a) + p[:, 2] * np.sin(a), -p[:, 0] * np.sin(a) + p[:, 2] * np.cos(a)
    # ... and squeezed at the waist, so that the triangles move relative to their boxes and not only with them
    s = 1.0 - 0.4 * min(amount, 1.0) * np.cos(np.pi * p[:, 1] / (2.0 * radius)) ** 2
    return np.ascontiguousarray(np.float32(np.stack([x * s, p[:, 1], z * s], 1) + c))


def refit_quality(a):
    scene = NB.scene(True)
    v0 = scene[0]["vertices"]
    legs = {}
    for mode in ("refit", "rebuild"):
        r = ptmi.Renderer(a.width, a.height, max_path_length=8, roulette_depth=3)
        r.set_constant_env(SKY)
        r.init_render_settings(seed=3, samples_per_step=a.spp)
        r.set_scene(scene)
        rec = ptmi.worklist(a.width, a.height)
        r.setup(rec)
        r.path_trace()
        r.read_results(rec)      # warm-up; builds the trees
        legs[mode] = (r, rec)
    lines = []
    for k in range(1, a.refits + 1):
        amount = 0.25 * k
        vk = twist(v0, NB.CENTRE, NB.RADIUS, amount)
        times = {m: [] for m in legs}
        for m, (r, rec) in legs.items():
            r.update_mesh_vertices(0, vk, mode=m)
        for step in range(a.steps):
            for m in (("refit", "rebuild") if step % 2 == 0 else ("rebuild", "refit")):
                r, rec = legs[m]
                r.path_trace()
                times[m].append(r.read_results(rec).total_ms)
        same = legs["refit"][1].tobytes() == legs["rebuild"][1].tobytes()
        med = {m: float(np.median(x)) for m, x in times.items()}
        lines.append("  after %d update(s), %.2f turns: refit %8.3f ms/step, rebuild %8.3f ms/step, refit / rebuild %.3f; accumulators %s" % (
            k, amount, med["refit"], med["rebuild"], med["refit"] / med["rebuild"], "bit-identical" if same else "DIFFER"))
    for r, _ in legs.values():
        r.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="6,8")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=1104)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--refits", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["mesh_update_bench: one smooth icosphere per level; an update with new normals, median of %d" % a.repeats]
    for level in [int(x) for x in a.levels.split(",") if x]:
        T, out = update_times(level, a.repeats)
        lines.append("level %d, %d triangles:" % (level, T))
        lines += out
    if a.refits:
        lines.append("refit quality: %d x %d, %d spp, depth 8, constant sky, ball 20480 + field 8192 triangles with normals (the ball keeps its normals), "
                     "%d steps per leg after each update, host builder" % (a.width, a.height, a.spp, a.steps))
        lines += refit_quality(a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
