#!/usr/bin/env python3
"""Step time of an HDR environment map (pt_set_env_map) on the C2 shape: 1104x1000, 300 spp, depth 8, built-in scene.

usage: python scripts/envmap_bench.py [repeats] [map_width map_height]

A map of map_width x map_height texels (default 4096 x 2048: 128 MiB of float4 texels on the device) is built in memory.  Both
filters are taken in turn on one renderer, and the constant environment for scale.  Prints one line each: step ms (pt_stats
total_ms, the median of `repeats` steps), nif_ms per launch (the N stage, here the map kernel), escaped paths, the gather rate
in lookups/s over nif_ms, and GB/s of texel bytes the lookups ask for (16 bytes per corner: one corner for nearest, four for
bilinear -- requested bytes, not HBM traffic: neighbouring corners share cache lines and the caches serve repeats).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipu_path_trace_amd import ptmi  # noqa: E402

W, H, SPP, DEPTH = 1104, 1000, 300, 8


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    mw, mh = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (4096, 2048)
    img = np.random.default_rng(1).uniform(0.0, 4.0, (mh, mw, 3)).astype(np.float32)
    envs = [("constant_env", None, 0), ("envmap_nearest", "nearest", 1), ("envmap_bilinear", "bilinear", 4)]
    r = ptmi.Renderer(W, H, max_path_length=DEPTH)
    try:
        r.init_render_settings(samples_per_step=SPP)
        rec = ptmi.worklist(W, H)
        r.setup(rec)
        out = {name: [] for name, _, _ in envs}
        for rep in range(repeats + 1):
            for name, filt, _ in envs:
                if filt is None:
                    r.set_constant_env((1, 1, 1))
                else:
                    r.set_env_map(img, filt)
                r.path_trace()
                st = r.stats()
                if rep:   # repeat 0 warms up
                    out[name].append((st.total_ms, st.nif_ms, st.nif_launches, st.escaped, st.path_trace_ms))
    finally:
        r.close()
    print("map %d x %d (%.0f MiB of texels), image %d x %d, %d spp, depth %d, median of %d steps" % (
        mw, mh, mw * mh * 16 / 2 ** 20, W, H, SPP, DEPTH, repeats))
    for name, filt, corners in envs:
        a = np.array(out[name], dtype=np.float64)
        total, nif, launches, escaped, trace = (float(np.median(a[:, k])) for k in range(5))
        line = "%-16s step ms %8.3f  trace ms %8.3f  escaped %d" % (name, total, trace, int(escaped))
        if corners:
            rate = escaped / (nif * 1e-3)
            line += "  nif_ms %7.3f over %d launches (%.3f per launch)  %.2f G lookups/s  %.1f GB/s of texel bytes" % (
                nif, int(launches), nif / launches, rate / 1e9, rate * 16 * corners / 1e9)
        print(line)


if __name__ == "__main__":
    main()
