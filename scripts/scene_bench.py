#!/usr/bin/env python3
"""Trace-kernel time of runtime scenes (pt_set_scene) against the built-in one, constant sky, one step of 1104x1000 x 64 spp.

usage: python scripts/scene_bench.py [depth] [repeats]

Scenes, taken in turn on one renderer: the built-in one (pt_set_scene(NULL, 0)), the built-in table passed through pt_set_scene, the built-in scene plus 26
small spheres inside the mirror sphere (32 objects: every intersection loop runs 32 trips, the image is the built-in one's),
and the built-in scene plus an emissive sphere in view.  Prints one line per scene: trace ms (sum of the step's trace-kernel
launches, the median of `repeats` steps), Mpaths/s over that time, segments per path, escaped paths.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipu_path_trace_amd import ptmi  # noqa: E402

W, H, SPP = 1104, 1000, 64
MIRROR_CENTRE = np.array([0.74795, -0.55, -4.3816])


def scenes():
    table = ptmi.builtin_scene()
    inner = []
    for k in range(26):
        th = 0.15 + 1.2 * (k % 13) / 12.0
        ph = 2 * np.pi * k / 26.0 + (0.3 if k >= 13 else 0.0)
        d = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        inner.append({"shape": "sphere", "centre": tuple(MIRROR_CENTRE + 0.8 * d), "radius": 0.05, "material": "diffuse",
                      "colour": (1.5, 0.2, 0.2)})
    light = ptmi.scene_array([{"shape": "sphere", "centre": (1.2, 1.6, -3.5), "radius": 0.6, "material": "emissive",
                               "emission": (6, 5, 4)}])
    return [("builtin", None), ("builtin_via_set_scene", table),
            ("builtin_plus_26_inside_mirror_32_objects", np.concatenate([table, ptmi.scene_array(inner)])),
            ("builtin_plus_emitter_7_objects", np.concatenate([table, light]))]


def main():
    depth = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    # ONE renderer (the same batch geometry for every scene), the scenes taken in turn within each repeat, so that the
    # device's drift between repeats weighs on all of them alike
    r = ptmi.Renderer(W, H, max_path_length=depth)
    try:
        r.set_constant_env((1, 1, 1))
        r.init_render_settings(samples_per_step=SPP)
        rec = ptmi.worklist(W, H)
        r.setup(rec)
        table = scenes()
        ms = {name: [] for name, _ in table}
        last = {}
        for rep in range(repeats + 1):
            for name, scene in table:
                r.set_scene(scene)
                r.path_trace()
                st = r.stats()
                if rep:   # repeat 0 warms up
                    ms[name].append(st.path_trace_ms)
                last[name] = (st.paths, st.segments, st.escaped)
    finally:
        r.close()
    base = float(np.median(ms["builtin"]))
    for name, _ in table:
        t = float(np.median(ms[name]))
        paths, segs, esc = last[name]
        print("%-44s depth %d  trace ms %.3f (median of %d)  Mpaths/s %.0f  seg/path %.3f  escaped %d  %+.2f %% vs builtin" % (
            name, depth, t, repeats, paths / (t * 1e-3) / 1e6, segs / paths, esc, 100.0 * (t / base - 1.0)))


if __name__ == "__main__":
    main()
