#!/usr/bin/env python3
"""The environment guide built from the environment in force (pt_set_env_guide_from_environment) measured on one device.

usage: python scripts/env_guide_from_env_bench.py [out-file] [train-steps] [render-steps]

Build time.  info.build_ms (HIP events around the S^2 planes: grid kernel, NIF stage, mass kernel) for the synthetic 6 x 320
fp16 NIF at 256 x 512 and at 1024 x 2048 cells with S = 2, five builds each; the first one carries the one-off costs.
Variance.  A NIF (6 x 320, embedding 12, the trainer's defaults) is trained on tests/env_guide_model.py::procedural_sun_map()
for `train-steps` Adam steps and installed.  The built-in scene, 256 x 192, depth 8, is rendered in `render-steps` steps of 16
spp under three samplers: unguided, guided from the environment (256 x 512, S = 2, alpha 0.5) and guided by the source image
(the same grid and alpha).  Per-sample variance = 16 x the variance of the step means over the steps, per pixel and channel,
averaged over the film; the film mean is printed beside it (the samplers must agree on it).
The lines go to stdout and to `out-file` (default profiles/r16_env_guide_from_env.txt).
Depends on tests/env_guide_model.py (imported as the package `tests` from the repository root) for the map.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ipu_path_trace_amd import nif_assets, ptmi  # noqa: E402
from tests import env_guide_model as G  # noqa: E402

W, H, SPP, DEPTH = 256, 192, 16, 8
ROWS, COLS, S, ALPHA = 256, 512, 2, 0.5


def step_means(r, steps):
    rec = ptmi.worklist(W, H)
    out = np.empty((steps, W * H, 3))
    for k in range(steps):
        for f in ("r", "g", "b", "sampleCount", "pathLength"):
            rec[f] = 0
        r.setup(rec)
        r.path_trace()
        r.read_results(rec)
        out[k] = np.stack([rec["b"], rec["g"], rec["r"]], -1).astype(np.float64) / rec["sampleCount"].astype(np.float64)[:, None]
    return out


def main():
    out_file = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_env_guide_from_env.txt")
    train_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    render_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("== python scripts/env_guide_from_env_bench.py <out> %d %d" % (train_steps, render_steps))
    r = ptmi.Renderer(W, H, max_path_length=DEPTH)
    try:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
        for rows, cols in ((256, 512), (1024, 2048)):
            ms = []
            for _ in range(5):
                r.set_env_guide_from_environment(rows, cols, ALPHA, S, follow=False)
                ms.append(r.env_guide_info()["build_ms"])
            say("build, 6 x 320 fp16 NIF, %4d x %4d cells, S = %d (%d lookups): build_ms %s" % (
                rows, cols, S, rows * cols * S * S, " ".join("%.3f" % x for x in ms)))
        r.set_env_guide(None)

        img = G.procedural_sun_map()
        r.set_env_map(img, "bilinear")
        t = r.train_nif()
        loss = t.steps(train_steps)
        t.install()
        t.close()
        say("NIF trained on procedural_sun_map() %d x %d and installed: %d steps, last loss %.6g" % (img.shape[1], img.shape[0], train_steps, loss))
        samplers = (("unguided", lambda: r.set_env_guide(None)),
                    ("guided from the environment", lambda: r.set_env_guide_from_environment(ROWS, COLS, ALPHA, S, follow=False)),
                    ("guided by the source image", lambda: r.set_env_guide(img, rows=ROWS, cols=COLS, alpha=ALPHA)))
        base = None
        for name, select in samplers:
            select()
            r.init_render_settings(seed=1, samples_per_step=SPP)
            m = step_means(r, render_steps)
            var = float(np.mean(SPP * m.var(axis=0, ddof=1)))
            base = base or var
            info = r.env_guide_info()
            say("%-28s per-sample variance %.6g (%.2fx lower than unguided)  film mean %.5f  [%d x %d, %d spp, depth %d, %d steps; "
                "guide source %s, clamped %d, build_ms %.3f]" % (name, var, base / var, m.mean(), W, H, SPP, DEPTH, render_steps,
                                                                 info["source"] if info["set"] else "none", info["clamped"], info["build_ms"]))
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
