#!/usr/bin/env python3
"""Device time of one A-trous iteration of the film denoiser (pt_denoise), per step and kernel variant.

usage: python scripts/denoise_bench.py [launches] [repeats]

For 1104 x 1000 and 3840 x 2160, on the built-in scene's features and a seeded noise image: every iteration i = 0 .. 5 (step 2^i)
of the default filter with its taps read from global memory, and iterations 0 and 1 also with the tile and halo staged in LDS
(the only steps that variant is built for).  Each figure is the median over `repeats` of the average of `launches` launches back
to back between two HIP events (pt_diag_denoise_bench of the profiling build: same kernels as the product), the variants taken
in turn.  Prints ms per iteration and the achieved bytes/s against one read plus one write of the colour frame (32 bytes per
pixel) -- the least traffic an iteration needs; the 25 taps of two 16-byte values it actually asks for are 800 bytes per pixel,
served by the caches or LDS.  Last, a whole pt_denoise call with the defaults from a host image, copies included.
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipu_path_trace_amd import ptmi  # noqa: E402

SHAPES = ((1104, 1000), (3840, 2160))


def main():
    launches = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for W, H in SHAPES:
        r = ptmi.Renderer(W, H, max_work_items=1024, diag=True)
        try:
            r.init_render_settings(samples_per_step=1)
            img = np.random.default_rng(1).uniform(0.0, 4.0, (H, W, 3)).astype(np.float32)
            r.denoise(image=img)                       # allocates the frames, computes the features, warms every kernel up
            variants = [(i, 0) for i in range(6)] + [(0, 1), (1, 1)]
            ms = {v: [] for v in variants}
            for _ in range(repeats):
                for it, tiled in variants:
                    out = C.c_double()
                    r._check(r._lib.pt_diag_denoise_bench(r.handle, tiled, it, launches, C.byref(out)))
                    ms[(it, tiled)].append(out.value)
            t0 = time.perf_counter()
            r.denoise(image=img)
            call_ms = (time.perf_counter() - t0) * 1e3
        finally:
            r.close()
        print("%d x %d, %d launches per figure, median of %d" % (W, H, launches, repeats))
        for it, tiled in variants:
            m = float(np.median(ms[(it, tiled)]))
            print("  iteration %d (step %2d) %-6s %8.4f ms  (min %.4f, max %.4f)  %7.1f GB/s of frame read + write" % (
                it, 2 ** it, "tiled" if tiled else "direct", m, min(ms[(it, tiled)]), max(ms[(it, tiled)]), W * H * 32 / (m * 1e-3) / 1e9))
        print("  pt_denoise, defaults, host image in and out: %.2f ms wall" % call_ms)


if __name__ == "__main__":
    main()
