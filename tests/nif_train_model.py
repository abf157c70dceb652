"""A numpy model of the NIF trainer (include/ptmi.h, pt_nif_train_*): encode, forward, loss, backward and Adam, in float64 by
default (`dtype=np.float32` runs the same expressions in float32: the yardstick the GPU tolerances are calibrated with).

Layers are [(kernel [in, out], bias [out], relu)] as nif_assets.synthetic_nif builds them; a layer whose input is wider than the
previous layer's output takes concat(x, features) (NifModel.cpp:305-308)."""
import numpy as np


def encode(embedding_dim, u, v):
    """Fourier features [n, 4 E] = [sin u, sin v, cos u, cos v] x E as float64 values of half precision: the argument
    (coord - 1) 2 2^j in float32 rounded to half, its sine correctly rounded to float32 (through float64), rounded to half --
    orc_nif_encode restated (tests/test_nif_train_model.py checks the two equal)."""
    u = np.asarray(u, np.float32).ravel()
    v = np.asarray(v, np.float32).ravel()
    out = np.empty((u.size, 4 * embedding_dim), np.float64)
    for h, coord in enumerate((u, v)):
        x = (coord - np.float32(1.0)) * np.float32(2.0)
        with np.errstate(over="ignore", invalid="ignore"):
            for j in range(embedding_dim):
                a = (x * np.float32(2.0 ** j)).astype(np.float16).astype(np.float64)
                out[:, h * embedding_dim + j] = np.sin(a).astype(np.float32).astype(np.float16)
                out[:, 2 * embedding_dim + h * embedding_dim + j] = np.cos(a).astype(np.float32).astype(np.float16)
    return out


def cast_layers(layers, dtype=np.float64):
    return [(np.asarray(k, dtype), np.zeros(np.asarray(k).shape[1], dtype) if b is None else np.asarray(b, dtype), bool(relu))
            for k, b, relu in layers]


def forward(layers, feats, dtype=np.float64):
    """Returns (y, inputs, pre): the head output, every layer's input matrix and its pre-activation."""
    layers = cast_layers(layers, dtype)
    feats = np.asarray(feats, dtype)
    x, inputs, pre = feats, [], []
    for k, b, relu in layers:
        if x.shape[1] != k.shape[0]:
            x = np.concatenate([x, feats], axis=1)
        assert x.shape[1] == k.shape[0]
        z = x @ k + b
        inputs.append(x)
        pre.append(z)
        x = np.maximum(z, 0) if relu else z
    return x, inputs, pre


def loss_and_gradients(layers, feats, target, dtype=np.float64):
    """MSE over batch x 3 and [(dW, db)] per layer."""
    layers = cast_layers(layers, dtype)
    target = np.asarray(target, dtype)
    y, inputs, pre = forward(layers, feats, dtype)
    d = y - target
    loss = dtype(np.mean(d.astype(np.float64) ** 2))
    dz = d * dtype(2.0 / d.size)
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        k = layers[l][0]
        grads[l] = (inputs[l].T @ dz, dz.sum(axis=0))
        if l == 0:
            break
        width = layers[l - 1][0].shape[1]            # the feature columns of a concat layer carry no gradient
        dz = (dz @ k.T)[:, :width] * (pre[l - 1] > 0)
    return loss, grads


class Adam:
    """m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, w -= lr (m c1) / (sqrt(v c2) + eps), c = 1 / (1 - b^t)."""

    def __init__(self, layers, learning_rate=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, dtype=np.float64):
        self.dtype = dtype
        self.layers = [(k.copy(), b.copy(), r) for k, b, r in cast_layers(layers, dtype)]
        # the library holds its constants in float32: the model uses those very values
        self.lr, self.b1, self.b2, self.eps = (dtype(np.float32(x)) for x in (learning_rate, beta1, beta2, eps))
        self.m = [[np.zeros_like(k), np.zeros_like(b)] for k, b, _ in self.layers]
        self.v = [[np.zeros_like(k), np.zeros_like(b)] for k, b, _ in self.layers]
        self.t = 0

    def step(self, feats, target):
        dtype = self.dtype
        loss, grads = loss_and_gradients(self.layers, feats, target, dtype)
        self.t += 1
        c1 = dtype(1.0 / (1.0 - float(self.b1) ** self.t))
        c2 = dtype(1.0 / (1.0 - float(self.b2) ** self.t))
        one = dtype(1.0)
        for l, (k, b, _) in enumerate(self.layers):
            for i, (w, g) in enumerate(((k, grads[l][0]), (b, grads[l][1]))):
                m = self.m[l][i] = self.b1 * self.m[l][i] + (one - self.b1) * g
                v = self.v[l][i] = self.b2 * self.v[l][i] + ((one - self.b2) * g) * g
                w -= (self.lr * (m * c1)) / (np.sqrt(v * c2) + self.eps)
        return loss


def procedural_map(height=8, width=16):
    """The smooth, positive HDR test map: 0.5 + 0.4 sin(2 pi c / W) cos(pi r / H) + 0.05 k (k = channel), rows 0-1 times 4."""
    r, c, k = np.meshgrid(np.arange(height), np.arange(width), np.arange(3), indexing="ij")
    img = 0.5 + 0.4 * np.sin(2 * np.pi * c / width) * np.cos(np.pi * r / height) + 0.05 * k
    img[:2] *= 4.0
    return img.astype(np.float32)


def encode_params(img, eps=1e-8, log_tone_map=True):
    """(mean [3], max) in float64 from the float32 image and the float32 eps."""
    L = image_l(img, eps, log_tone_map)
    mean = L.reshape(-1, 3).mean(axis=0)
    return mean, float(np.max(np.abs(L - mean)))


def image_l(img, eps=1e-8, log_tone_map=True):
    img = np.asarray(img, np.float32).astype(np.float64)
    return np.log(img + np.float64(np.float32(eps))) if log_tone_map else img


def targets(img, mean, max_value, eps=1e-8, log_tone_map=True):
    """(L - mean) / max in float64, mean and max as given (the library's float32 values)."""
    return (image_l(img, eps, log_tone_map) - np.asarray(mean, np.float64)) / np.float64(max_value)


def grid_uv(height, width):
    """u = r / H, v = c / W by one float32 division each, row-major over the image."""
    r, c = np.divmod(np.arange(height * width), width)
    return (r.astype(np.float32) / np.float32(height)), (c.astype(np.float32) / np.float32(width))


def image_loss(layers, embedding_dim, tgt):
    """MSE of the model over every texel of the target image [H, W, 3], float64."""
    u, v = grid_uv(tgt.shape[0], tgt.shape[1])
    y, _, _ = forward(layers, encode(embedding_dim, u, v))
    return float(np.mean((y - tgt.reshape(-1, 3)) ** 2))


def relu_safe_batch(layers, embedding_dim, batch, seed, margin=1e-4):
    """`batch` samples (u, v) out of 4 x batch seeded candidates whose float64 pre-activations all keep |z| > margin, so that no
    ReLU can flip between float32 and float64; returns (u, v, fraction of the candidates seen that were rejected)."""
    rng = np.random.Generator(np.random.Philox(seed))
    u = rng.random(4 * batch, dtype=np.float32)
    v = rng.random(4 * batch, dtype=np.float32)
    _, _, pre = forward(layers, encode(embedding_dim, u, v))
    ok = np.ones(u.size, bool)
    for z, (_, _, relu) in zip(pre, layers):
        if relu:
            ok &= np.all(np.abs(z) > margin, axis=1)
    keep = np.flatnonzero(ok)[:batch]
    assert keep.size == batch, "not enough ReLU-safe candidates"
    seen = keep[-1] + 1
    return u[keep], v[keep], float(seen - batch) / float(seen)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11; constants as Random123) on uint32 arrays; returns the four output words."""
    c = [np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1, mask = np.uint64(k0), np.uint64(k1), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return [x.astype(np.uint32) for x in c]


def batch_indices(seed, step, batch, height, width):
    """Texel index of every sample of step `step`: floor(word 0 x H W / 2^32) of block (i, step low, step high, "NIFB")."""
    w0 = philox4x32_10(np.arange(batch), step & 0xFFFFFFFF, step >> 32, 0x4E494642, seed & 0xFFFFFFFF, seed >> 32)[0]
    return ((w0.astype(np.uint64) * np.uint64(height * width)) >> np.uint64(32)).astype(np.int64)


def batch(seed, step, batch_size, tgt):
    """(u, v, target float64 [batch, 3], index) of step `step` on the target image tgt [H, W, 3]."""
    height, width = tgt.shape[:2]
    idx = batch_indices(seed, step, batch_size, height, width)
    r, c = np.divmod(idx, width)
    return (r.astype(np.float32) / np.float32(height)), (c.astype(np.float32) / np.float32(width)), tgt.reshape(-1, 3)[idx], idx
