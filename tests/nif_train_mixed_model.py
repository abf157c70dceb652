"""A numpy model of the NIF trainer's mixed-precision step (include/ptmi.h, PT_NIF_TRAIN_MIXED_F16), built on nif_train_model.py
and following the header's contract literally: half inputs to every matrix product, binary32 results, a loss scale S, binary32
masters, and the skip / grow state machine of S.

`acc` is how a matrix product and a column sum are formed: np.float64 = the exact products summed in binary64 and rounded to
binary32 once (the best any summation order can do), np.float32 = numpy's own binary32 order.  The difference between the two
runs on a test's very inputs is what the GPU tolerances are calibrated with: the device's tiled order is a
third order of the same binary32 sums.

`ftz=True` is a deliberately wrong model for the sensitivity tests: halves below the normal range are flushed to zero."""
import numpy as np

from tests import nif_train_model as M

SLABS = 32                       # kTrainSlabs
MAX_SCALE = 2.0 ** 30
HALF_MAX = 65504.0


def half(x, ftz=False):
    """binary32 values rounded to binary16 (nearest even), returned as float32 values of half precision."""
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.asarray(x, np.float32).astype(np.float16)
    if ftz:
        h = np.where(np.abs(h) < np.float16(2.0 ** -14), np.float16(0), h)
    return h.astype(np.float32)


def matmul(a, b, acc):
    """float32 [m, n] = a @ b over half values, summed as `acc` says."""
    with np.errstate(over="ignore", invalid="ignore"):
        if acc == np.float64:
            return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
        return a.astype(np.float32) @ b.astype(np.float32)


def colsum(a, acc):
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(acc).sum(axis=0).astype(np.float32)


def slab_rows(n):
    """Rows of one batch slab: ceil(n / 32) rounded up to the half GEMM's K tile of 32."""
    return (-(-n // SLABS) + 31) // 32 * 32


def masters(layers):
    return [(np.asarray(k, np.float32), np.zeros(np.asarray(k).shape[1], np.float32) if b is None else np.asarray(b, np.float32), bool(r))
            for k, b, r in layers]


def forward(layers, feats, acc=np.float64, ftz=False):
    """(y float32, inputs, pre): the head output, every layer's half input matrix (float32 values) and its binary32
    pre-activation."""
    feats = np.asarray(feats, np.float32)
    x, inputs, pre = feats, [], []
    for k, b, relu in masters(layers):
        if x.shape[1] != k.shape[0]:
            x = np.concatenate([x, feats], axis=1)
        z = matmul(x, half(k, ftz), acc) + b
        inputs.append(x)
        pre.append(z)
        x = half(np.maximum(z, np.float32(0)), ftz) if relu else z
    return x, inputs, pre


def loss_and_gradients(layers, feats, target, scale, acc=np.float64, ftz=False):
    """(loss, [(dW, db)] unscaled float32, info).  Non-finite gradients mean overflow.  info["peak"] = the largest magnitude
    among the finite scaled gradients about to be rounded to half (what follows an overflow is not finite): beyond 65504 the pass overflows, and its distance from 65504 is how
    far the pass is from changing its verdict; info["subnormal"] = how many of them land, nonzero, below the half's normal
    range (and lose bits there)."""
    layers = masters(layers)
    target = np.asarray(target, np.float32)
    y, inputs, _ = forward(layers, feats, acc, ftz)
    n = target.shape[0]
    d = (y - target).astype(np.float32)
    with np.errstate(over="ignore"):
        loss = np.float32(np.mean(d.astype(np.float64) ** 2))
    c = np.float32(2.0 * float(scale) / (3.0 * n))
    inv = np.float32(1.0 / float(scale))
    info = {"peak": 0.0, "subnormal": 0}

    def rounded(x):
        with np.errstate(over="ignore", invalid="ignore"):
            info["peak"] = max(info["peak"], float(np.max(np.abs(np.where(np.isfinite(x), x, np.float32(0))))))
            info["subnormal"] += int(np.sum((x != 0) & (np.abs(x) < np.float32(2.0 ** -14))))
            return half(x, ftz)

    with np.errstate(over="ignore", invalid="ignore"):
        dz = rounded(d * c)
    rows = slab_rows(n)
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        k = layers[l][0]
        dw = np.zeros(k.shape, np.float32)
        db = np.zeros(k.shape[1], np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            for s in range(SLABS):                       # partials in slab order, binary32
                sl = slice(s * rows, min(n, (s + 1) * rows))
                if sl.start >= n:
                    pw, pb = np.zeros_like(dw), np.zeros_like(db)
                else:
                    pw, pb = matmul(inputs[l][sl].T, dz[sl], acc), colsum(dz[sl], acc)
                dw, db = (pw, pb) if s == 0 else (dw + pw, db + pb)
            grads[l] = (dw * inv, db * inv)
        if l == 0:
            break
        width = layers[l - 1][0].shape[1]                # the feature columns of a concat layer carry no gradient
        with np.errstate(over="ignore", invalid="ignore"):
            below = matmul(dz, half(k, ftz).T, acc)[:, :width]
            dz = rounded(np.where(inputs[l][:, :width] > 0, below, np.float32(0)))
    return loss, grads, info


def finite(grads):
    return all(np.isfinite(dw).all() and np.isfinite(db).all() for dw, db in grads)


class Trainer:
    """The mixed step with its state machine.  The masters, moments and Adam's arithmetic are held in `acc` (the library:
    binary32); w16 is always half((float32) w)."""

    def __init__(self, layers, loss_scale=65536.0, dynamic=True, growth_interval=2000, learning_rate=1e-3, beta1=0.9, beta2=0.999,
                 eps=1e-7, acc=np.float64):
        self.acc = acc
        self.adam = M.Adam(masters(layers), learning_rate, beta1, beta2, eps, dtype=acc)
        self.S, self.dynamic, self.growth = float(loss_scale), bool(dynamic), int(growth_interval)
        self.good = self.applied = self.skipped = 0
        self.history = []                                # per step: state() after it
        self.margins = []                                # per step: | peak / 65504 - 1 |, peak = loss_and_gradients' info["peak"]

    @property
    def layers(self):
        return self.adam.layers

    def step(self, feats, target):
        """One step; returns (loss, applied?)."""
        a, dtype = self.adam, self.acc
        now = [(k.astype(np.float32), b.astype(np.float32), r) for k, b, r in a.layers]
        loss, grads, info = loss_and_gradients(now, feats, target, self.S, self.acc)
        self.margins.append(abs(info["peak"] / HALF_MAX - 1.0))
        if not finite(grads):
            self.skipped += 1
            if self.dynamic:
                self.S, self.good = max(self.S * 0.5, 1.0), 0
            self.history.append(self.state())
            return loss, False
        a.t = self.applied + 1
        c1, c2, one = dtype(1.0 / (1.0 - float(a.b1) ** a.t)), dtype(1.0 / (1.0 - float(a.b2) ** a.t)), dtype(1.0)
        for l, (k, b, _) in enumerate(a.layers):
            for i, (w, g) in enumerate(((k, grads[l][0].astype(dtype)), (b, grads[l][1].astype(dtype)))):
                m = a.m[l][i] = a.b1 * a.m[l][i] + (one - a.b1) * g
                v = a.v[l][i] = a.b2 * a.v[l][i] + ((one - a.b2) * g) * g
                w -= (a.lr * (m * c1)) / (np.sqrt(v * c2) + a.eps)
        self.applied += 1
        self.good += 1
        if self.dynamic and self.good >= self.growth:
            self.S, self.good = min(self.S * 2.0, MAX_SCALE), 0
        self.history.append(self.state())
        return loss, True

    def state(self):
        return {"loss_scale": self.S, "good_steps": self.good, "applied_steps": self.applied, "skipped_steps": self.skipped}


def relu_safe_batch_mixed(layers, embedding_dim, batch, seed, margin=1e-4):
    """nif_train_model.relu_safe_batch with the candidates selected on the MIXED model's own pre-activations (binary64 sums):
    every |z| > margin, so that no ReLU flips with the summation order.  Returns (u, v, rejected share of the candidates seen)."""
    rng = np.random.Generator(np.random.Philox(seed))
    u = rng.random(4 * batch, dtype=np.float32)
    v = rng.random(4 * batch, dtype=np.float32)
    _, _, pre = forward(layers, M.encode(embedding_dim, u, v), np.float64)
    ok = np.ones(u.size, bool)
    for z, (_, _, relu) in zip(pre, layers):
        if relu:
            ok &= np.all(np.abs(z) > margin, axis=1)
    keep = np.flatnonzero(ok)[:batch]
    assert keep.size == batch, "not enough ReLU-safe candidates"
    seen = keep[-1] + 1
    return u[keep], v[keep], float(seen - batch) / float(seen)
