#!/usr/bin/env python3
"""Trace-kernel time of runtime cameras (pt_set_camera) against the built-in one, constant sky, one step of 1104x1000 x 64 spp.

usage: python scripts/camera_bench.py [depth] [repeats]

Cameras, taken in turn on one renderer over the built-in scene: the built-in one (pt_set_camera(NULL)), the same values passed
through pt_set_camera (the same kernel instance: the frame is the identity and no transform is applied), a moved and rotated
pinhole (the pose instance: escapes rotated to world space) and the built-in pose with a thin lens (the lens instance: its own
primary phase).  Prints one line per camera: trace ms (sum of the step's trace-kernel launches, the median of `repeats`
steps), Mpaths/s over that time, segments per path, escaped paths.  The moved camera and the lens see other images (other
path lengths): their lines are not like for like with the built-in one's.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipu_path_trace_amd import ptmi  # noqa: E402

W, H, SPP = 1104, 1000, 64

CAMERAS = [("builtin", None),
           ("builtin_via_set_camera", dict(position=(0, 0, 0), look_at=(0, 0, -1), up=(0, 1, 0))),
           ("moved_rotated_pinhole", dict(position=(1.2, 0.4, 0.8), look_at=(0.0, -0.8, -4.0), up=(0.05, 1.0, 0.0))),
           ("thin_lens_a0.05_F4", dict(lens_radius=0.05, focus_distance=4.0))]


def main():
    depth = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    # ONE renderer (the same batch geometry for every camera), the cameras taken in turn within each repeat, so that the
    # device's drift between repeats weighs on all of them alike
    r = ptmi.Renderer(W, H, max_path_length=depth)
    try:
        r.set_constant_env((1, 1, 1))
        r.init_render_settings(samples_per_step=SPP)
        rec = ptmi.worklist(W, H)
        r.setup(rec)
        ms = {name: [] for name, _ in CAMERAS}
        last = {}
        for rep in range(repeats + 1):
            for name, camera in CAMERAS:
                if camera is None:
                    r.set_camera(None)
                else:
                    r.set_camera(**camera)
                r.path_trace()
                st = r.stats()
                if rep:   # repeat 0 warms up
                    ms[name].append(st.path_trace_ms)
                last[name] = (st.paths, st.segments, st.escaped)
    finally:
        r.close()
    base = float(np.median(ms["builtin"]))
    for name, _ in CAMERAS:
        t = float(np.median(ms[name]))
        paths, segs, esc = last[name]
        print("%-26s depth %d  trace ms %.3f (median of %d)  Mpaths/s %.0f  seg/path %.3f  escaped %d  %+.2f %% vs builtin" % (
            name, depth, t, repeats, paths / (t * 1e-3) / 1e6, segs / paths, esc, 100.0 * (t / base - 1.0)))


if __name__ == "__main__":
    main()
