#!/usr/bin/env python3
"""A first timing of a textured mesh scene against the same scene untextured (pt_set_mesh_texture): the scene of
scripts/mesh_normals_bench.py with its normals -- an icosphere(5) glass ball (20480 triangles) over a 64 x 64 diffuse height field
(8192 triangles) --, under a constant sky and under the synthetic NIF.

usage: python scripts/mesh_texture_bench.py [--width W] [--height H] [--spp N] [--steps K] [--texture N] [--out FILE]      (GPU)

Two handles in one process render the same scene, one untextured -- the smooth-mesh kernels as they were, the baseline -- and one
with an N x N bilinear image on each mesh (the TEX instances); their steps alternate, the first step of each is warm-up.  Printed,
and appended to --out: milliseconds per step and the trace stage's milliseconds (pt_stats.total_ms, path_trace_ms; medians over
the steps), and textured / smooth.  No ratio is fixed in advance: what the textured instances cost beyond the smooth ones is the
finding."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ipu_path_trace_amd import nif_assets, ptmi   # noqa: E402
from tests import scene_mesh_model as MM           # noqa: E402  (the generators of the mesh tests)

CENTRE, RADIUS = (0.0, 0.0, -0.6), 0.18
SKY = (0.75, 1.5, 3.0)


def image(n, seed):
    """(n, n, 3) B,G,R: white noise between 0.2 and 1, so that the throughput stays what the untextured scene's is in magnitude."""
    rng = np.random.default_rng(seed)
    return np.float32(0.2 + 0.8 * rng.random((n, n, 3)))


def scene(textured, n):
    sv, st = MM.icosphere(5, RADIUS, CENTRE)
    fv, ft = MM.height_field(64, 1.4, (0.0, -0.25, -0.7), 0.05)
    sv, fv = np.float32(sv), np.float32(fv)
    ball = {"shape": "mesh", "material": "refractive", "colour": (0.9, 0.95, 0.9), "vertices": sv, "triangles": st}
    field = {"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": fv, "triangles": ft}
    ball["normals"] = np.float32((sv.astype(np.float64) - np.asarray(CENTRE)) / RADIUS)
    field["normals"] = ptmi.vertex_normals(fv, ft)
    if textured:
        p = (sv.astype(np.float64) - np.asarray(CENTRE)) / RADIUS
        ball.update(texture=image(n, 1), texture_filter="bilinear", texture_wrap="repeat",
                    uvs=np.float32(np.stack([np.arctan2(p[:, 2], p[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(p[:, 1], -1, 1)) / np.pi], -1)))
        field.update(texture=image(n, 2), texture_filter="bilinear", texture_wrap="repeat",
                     uvs=np.float32(4.0 * (fv[:, [0, 2]] - fv[:, [0, 2]].min(axis=0)) / np.ptp(fv[:, [0, 2]], axis=0)))
    return [ball, field]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1104)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--texture", type=int, default=256)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["mesh_texture_bench: %d x %d, %d spp per step, %d timed steps per leg, depth 8; ball 20480 + field 8192 triangles, "
             "both smooth; textured: a %d x %d bilinear image on each" % (a.width, a.height, a.spp, a.steps - 1, a.texture, a.texture)]
    for env in ("constant", "nif"):
        legs = {}
        for textured in (False, True):
            r = ptmi.Renderer(a.width, a.height, max_path_length=8, roulette_depth=3)
            if env == "constant":
                r.set_constant_env(SKY)
            else:
                r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
            r.init_render_settings(seed=3, samples_per_step=a.spp)
            r.set_scene(scene(textured, a.texture))
            rec = ptmi.worklist(a.width, a.height)
            r.setup(rec)
            legs[textured] = (r, rec, [], [])
        for step in range(a.steps):
            for textured in (False, True) if step % 2 == 0 else (True, False):     # the legs take turns to go first
                r, rec, total, trace = legs[textured]
                r.path_trace()
                st = r.read_results(rec)
                if step:                                                          # step 0 warms up (and builds the trees)
                    total.append(st.total_ms)
                    trace.append(st.path_trace_ms)
        med = {s: (float(np.median(legs[s][2])), float(np.median(legs[s][3]))) for s in legs}
        for r, _, _, _ in legs.values():
            r.close()
        lines.append("%-8s smooth   %8.3f ms/step, trace stage %8.3f ms" % (env, med[False][0], med[False][1]))
        lines.append("%-8s textured %8.3f ms/step, trace stage %8.3f ms   textured / smooth: step %.3f, trace stage %.3f" % (
            env, med[True][0], med[True][1], med[True][0] / med[False][0], med[True][1] / med[False][1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
