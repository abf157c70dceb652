#!/usr/bin/env python3
"""The NIF trainer (pt_nif_train_*) measured: milliseconds per Adam step and quality of a trained model.

usage: python scripts/nif_train_bench.py [steps-per-window] [repeats] [quality-steps] [--precision mixed]

Speed.  6 x 320, embedding 12, batch 65536 on a procedural 512 x 256 HDR map.  A window is `steps-per-window` steps between two
host clock readings, the second after the call's device synchronise (pt_nif_train_steps blocks); the figure is the median over
`repeats` windows after a warm-up window.  FLOPs per step = 3 x batch x the forward FLOPs of nif_assets.flops_per_sample
(forward, input gradient, weight gradient); the share of peak is against 157 TFLOP/s, the fp32 matrix rate.  This is a
whole-step rate: sampling, encode, loss, reductions and Adam are inside the window.
Yardstick, same box, same run, windows taken in turn with the trainer's: the same stack as torch.nn.Linear layers in float32 with
torch.optim.Adam on a resident batch of random features (its encode and sampling are NOT in its window, which favours it).

Quality.  The same model trained for `quality-steps` steps: the last batch loss, the full-image MSE and PSNR in the normalised
log domain (peak 2: targets span [-1, 1]) from the float64 model of tests/nif_train_model.py on the float32 master weights, and
what the binary16 export loses: the installed NIF through pt_nif_infer against that float64 forward pass, in the same domain.
Depends on tests/nif_train_model.py (imported as the package `tests` from the repository root) for that float64 model.

Precision.  With --precision mixed the run compares, windows in turn in one process: the float32 trainer, the trainer after
set_precision("mixed") (on a second handle), the float32 yardstick, and a second yardstick, the same torch stack under
torch.autocast(float16) with torch.amp.GradScaler; the mixed rates are also given against the 2.5 PFLOP/s fp16 matrix peak.
The quality part then trains in mixed mode and reports the scale and the applied / skipped steps.  Without the argument the
run and its output are what they were.

Features.  How many of the inference kernels' Fourier features differ from the trainer's (the oracle's) on a 64 x 64 texel grid
and at random (u, v).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ipu_path_trace_amd import nif_assets, ptmi  # noqa: E402
from tests import nif_train_model as M  # noqa: E402

EMB, HIDDEN, LAYERS, BATCH = 12, 320, 6, 65536
PEAK_TFLOPS = 157.0
PEAK_F16_TFLOPS = 2500.0


def procedural_hdr(height=256, width=512):
    """Sky gradient, a sun four orders of magnitude above it, a ground band and fine stripes: smooth, positive, HDR."""
    r, c = np.meshgrid(np.arange(height) / height, np.arange(width) / width, indexing="ij")
    sky = 0.3 + 0.5 * (1.0 - r) ** 2
    sun = 4000.0 * np.exp(-(((r - 0.25) * 2) ** 2 + (c - 0.6) ** 2) / 0.0008)
    ground = np.where(r > 0.55, 0.08 + 0.05 * np.sin(40 * np.pi * c) * np.sin(24 * np.pi * r), 0.0)
    base = np.where(r > 0.55, 0.0, sky) + sun + ground
    return np.stack([base * 1.1, base, base * 0.85], -1).astype(np.float32)


def inference_features(r, u, v):
    """The Fourier features the INFERENCE kernels form at (u, v), [n, 4 E] float64, read back through pt_nif_infer with probe
    models: neuron 2 i = +feature, neuron 2 i + 1 = -feature, head = their difference (exact in binary16), no tone map."""
    out = np.empty((u.size, 4 * EMB), np.float64)
    for f0 in range(0, 4 * EMB, 3):
        k0 = np.zeros((4 * EMB, 32), np.float16)
        k1 = np.zeros((32, 3), np.float16)
        for i in range(3):
            k0[f0 + i, 2 * i], k0[f0 + i, 2 * i + 1] = 1.0, -1.0
            k1[2 * i, i], k1[2 * i + 1, i] = 1.0, -1.0
        r.init_nif_weights([(k0, None, True), (k1, None, False)], EMB, 1.0, [0.0, 0.0, 0.0], log_tonemap=False)
        out[:, f0:f0 + 3] = r.nif_infer(u, v)
    return out


def torch_yardstick(shapes, skip, autocast=False):
    import torch

    dev = torch.device("cuda")

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = torch.nn.ModuleList([torch.nn.Linear(rows, cols) for rows, cols, _ in shapes])

        def forward(self, feats):
            x = feats
            for l, layer in enumerate(self.layers):
                if l == skip and l > 0:
                    x = torch.cat([x, feats], dim=1)
                x = layer(x)
                if l + 1 < len(self.layers):
                    x = torch.relu(x)
            return x

    net = Net().to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-7)
    feats = torch.rand(BATCH, 4 * EMB, device=dev) * 2 - 1
    target = torch.rand(BATCH, 3, device=dev) * 2 - 1

    def window(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            loss = torch.mean((net(feats) - target) ** 2)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    scaler = torch.amp.GradScaler("cuda") if autocast else None

    def window_autocast(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                y = net(feats)
            loss = torch.mean((y.float() - target) ** 2)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    return window_autocast if autocast else window


def main_mixed(steps, repeats, quality_steps):
    img = procedural_hdr()
    handles = []
    for precision in (None, "mixed"):
        r = ptmi.Renderer(32, 32)
        r.set_env_map(img, "nearest")
        handles.append((r, r.train_nif(embedding_dim=EMB, hidden=HIDDEN, layer_count=LAYERS, batch=BATCH, seed=1, precision=precision)))
    shapes = handles[0][1].shapes
    flops = 3 * BATCH * nif_assets.flops_per_sample([(np.empty((rows, cols)), np.empty(cols), relu) for rows, cols, relu in shapes])
    print("model %d x %d, embedding %d, batch %d: %.1f GFLOP per step (3 x forward)" % (LAYERS, HIDDEN, EMB, BATCH, flops / 1e9))

    def ours(t):
        def window(n):
            t0 = time.perf_counter()
            t.steps(n)
            return (time.perf_counter() - t0) * 1e3 / n
        return window

    runs = [("pt_nif_train_steps, f32 (fp32 MFMA)", ours(handles[0][1])), ("pt_nif_train_steps, mixed (fp16 MFMA)", ours(handles[1][1])),
            ("torch.nn.Linear + torch.optim.Adam, float32", torch_yardstick(shapes, LAYERS // 2)),
            ("torch, autocast(float16) + GradScaler", torch_yardstick(shapes, LAYERS // 2, autocast=True))]
    for _, w in runs:
        w(steps)
    times = [[] for _ in runs]
    for _ in range(repeats):
        for i, (_, w) in enumerate(runs):
            times[i].append(w(steps))
    print("%d steps per window, median of %d windows taken in turn" % (steps, repeats))
    for (name, _), xs in zip(runs, times):
        m = float(np.median(xs))
        tf = flops / (m * 1e-3) / 1e12
        print("  %-46s %8.3f ms per step (min %.3f, max %.3f)  %7.1f TFLOP/s = %4.1f %% of the %g TFLOP/s fp32 peak, %4.1f %% of the %g TFLOP/s fp16 peak"
              % (name, m, min(xs), max(xs), tf, 100.0 * tf / PEAK_TFLOPS, PEAK_TFLOPS, 100.0 * tf / PEAK_F16_TFLOPS, PEAK_F16_TFLOPS))
    print("  slowest mixed window %.3f ms, fastest f32 window %.3f ms: mixed is %s beyond the run's spread"
          % (max(times[1]), min(times[0]), "FASTER" if max(times[1]) < min(times[0]) else "NOT faster"))
    print("  mixed step / f32 step = %.3f; mixed step / autocast yardstick step = %.3f"
          % (float(np.median(times[1])) / float(np.median(times[0])), float(np.median(times[1])) / float(np.median(times[3]))))
    print("  state after the windows: %s" % handles[1][1].precision_state())
    for r, t in handles:
        t.close()
    r = handles[1][0]
    handles[0][0].close()
    t = r.train_nif(embedding_dim=EMB, hidden=HIDDEN, layer_count=LAYERS, batch=BATCH, seed=1, precision="mixed")
    t0 = time.perf_counter()
    loss = t.steps(quality_steps)
    wall = time.perf_counter() - t0
    enc = t.encode_params()
    tgt = M.targets(img, np.asarray(enc["mean"], np.float32), np.float32(enc["max"])).astype(np.float32).astype(np.float64)
    u, v = M.grid_uv(img.shape[0], img.shape[1])
    y = np.concatenate([M.forward(t.weights(), M.encode(EMB, u[i:i + 16384], v[i:i + 16384]))[0] for i in range(0, u.size, 16384)])
    mse = float(np.mean((y - tgt.reshape(-1, 3)) ** 2))
    print("mixed quality on the procedural %d x %d map after %d steps (%.1f s): last batch loss %.4e, full-image MSE %.4e, PSNR %.2f dB "
          "(normalised log domain, peak 2); %s" % (img.shape[1], img.shape[0], quality_steps, wall, loss, mse, 10 * np.log10(4.0 / mse),
                                                   t.precision_state()))
    t.close()
    r.close()


def main():
    mixed = False
    if "--precision" in sys.argv:
        at = sys.argv.index("--precision")
        if at + 1 >= len(sys.argv) or sys.argv[at + 1] not in ("f32", "mixed"):
            sys.exit("--precision takes f32 or mixed")
        mixed = sys.argv[at + 1] == "mixed"
        del sys.argv[at:at + 2]
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    quality_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    if mixed:
        return main_mixed(steps, repeats, quality_steps)
    img = procedural_hdr()
    r = ptmi.Renderer(32, 32)
    r.set_env_map(img, "nearest")
    t = r.train_nif(embedding_dim=EMB, hidden=HIDDEN, layer_count=LAYERS, batch=BATCH, seed=1)
    flops = 3 * BATCH * nif_assets.flops_per_sample([(np.empty((rows, cols)), np.empty(cols), relu) for rows, cols, relu in t.shapes])
    print("model %d x %d, embedding %d, batch %d: %.1f GFLOP per step (3 x forward)" % (LAYERS, HIDDEN, EMB, BATCH, flops / 1e9))

    def ours(n):
        t0 = time.perf_counter()
        t.steps(n)
        return (time.perf_counter() - t0) * 1e3 / n

    theirs = torch_yardstick(t.shapes, LAYERS // 2)
    ours(steps)
    theirs(steps)
    a, b = [], []
    for _ in range(repeats):
        a.append(ours(steps))
        b.append(theirs(steps))
    ma, mb = float(np.median(a)), float(np.median(b))
    print("%d steps per window, median of %d windows taken in turn" % (steps, repeats))
    for name, m, xs in (("pt_nif_train_steps (hand-written HIP, fp32 MFMA)", ma, a), ("torch.nn.Linear + torch.optim.Adam, float32", mb, b)):
        print("  %-50s %8.3f ms per step (min %.3f, max %.3f)  %6.1f TFLOP/s = %4.1f %% of the %g TFLOP/s fp32 matrix peak"
              % (name, m, min(xs), max(xs), flops / (m * 1e-3) / 1e12, 100.0 * flops / (m * 1e-3) / 1e12 / PEAK_TFLOPS, PEAK_TFLOPS))
    print("  hand-written step / yardstick step = %.2f" % (ma / mb))

    # quality: a fresh model, `quality_steps` steps
    t.close()
    t = r.train_nif(embedding_dim=EMB, hidden=HIDDEN, layer_count=LAYERS, batch=BATCH, seed=1)
    t0 = time.perf_counter()
    loss = t.steps(quality_steps)
    wall = time.perf_counter() - t0
    enc = t.encode_params()
    tgt = M.targets(img, np.asarray(enc["mean"], np.float32), np.float32(enc["max"])).astype(np.float32).astype(np.float64)
    u, v = M.grid_uv(img.shape[0], img.shape[1])
    y = np.concatenate([M.forward(t.weights(), M.encode(EMB, u[i:i + 16384], v[i:i + 16384]))[0] for i in range(0, u.size, 16384)])
    mse = float(np.mean((y - tgt.reshape(-1, 3)) ** 2))
    print("quality on the procedural %d x %d map after %d steps (%.1f s): last batch loss %.4e, full-image MSE %.4e, PSNR %.2f dB "
          "(normalised log domain, peak 2)" % (img.shape[1], img.shape[0], quality_steps, wall, loss, mse, 10 * np.log10(4.0 / mse)))
    t.install()
    folded = np.array([np.float32(np.float32(m) - np.float32(enc["eps"])) for m in enc["mean"]], np.float64)
    with np.errstate(divide="ignore"):
        yh = (np.log(r.nif_infer(u, v).astype(np.float64)) - folded) / enc["max"]
    d = yh - y
    print("binary16 export (%s) against the float64 forward pass of the float32 weights: max |dy| %.3e, rms %.3e; its own full-image MSE %.4e, "
          "PSNR %.2f dB" % (r.nif_kernel_name(), float(np.max(np.abs(d))), float(np.sqrt(np.mean(d ** 2))),
                            float(np.mean((yh - tgt.reshape(-1, 3)) ** 2)), 10 * np.log10(4.0 / float(np.mean((yh - tgt.reshape(-1, 3)) ** 2)))))
    t.close()
    # the inference kernels' features (v_sin_f32 / v_cos_f32) against the trainer's (= the oracle's)
    try:
        rng = np.random.Generator(np.random.Philox(3))
        for what, (gu, gv) in (("the 64 x 64 texel grid", M.grid_uv(64, 64)),
                               ("4096 random (u, v)", (rng.random(4096, dtype=np.float32), rng.random(4096, dtype=np.float32)))):
            d = np.abs(inference_features(r, gu, gv) - M.encode(EMB, gu, gv))
            print("features, inference kernels against the trainer's encode on %s, %d values: %d differ (%.4f %%), largest difference "
                  "%.3e (one half-precision step below 1 is 4.9e-4)" % (what, d.size, int(np.count_nonzero(d)), 100.0 * np.count_nonzero(d) / d.size,
                                                                       float(d.max())))
    except ptmi.PtError as e:
        print("features: not measured (%s)" % e)
    r.close()


if __name__ == "__main__":
    main()
