"""A float64 statement of the edge-avoiding A-trous filter of include/ptmi.h (pt_denoise) -- test infrastructure only.

Plain numpy in float64, straight from the definition in the header and vectorised over taps: each of the 25 offsets is one
shifted-array expression, with the three exponentials as the definition writes them.  It is a model, not a port of the kernel:
it knows no binary32 rounding, no tiles, and forms the product w_c w_n w_d where the kernel takes one exponential of a sum.
"""
import numpy as np

K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)        # the B3 spline: h(dx, dy) = K[|dx|] K[|dy|]
ALBEDO_FLOOR = 1e-3
DEPTH_FLOOR = 1e-6
DEFAULTS = dict(iterations=5, sigma_colour=4.0, sigma_normal=0.5, sigma_depth=0.1, object_stop=1, demodulate=1)


def _shift(a, dx, dy):
    """(a[q] for q = p + (dx, dy), valid): b[y, x] = a[y + dy, x + dx] where that lies inside the image."""
    H, W = a.shape[:2]
    b = np.zeros_like(a)
    valid = np.zeros((H, W), bool)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
        valid[ys, xs] = True
    return b, valid


def iteration(c, i, normal, depth, ids, sigma_colour, sigma_normal, sigma_depth, object_stop):
    """c_{i+1} from c_i: step 2^i, taps outside the image skipped, the centre tap's weight 1 exactly."""
    s = 2 ** i
    num = K[0] * K[0] * c
    den = np.full(c.shape[:2], K[0] * K[0])
    sc = sigma_colour * 2.0 ** -i
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                cq, valid = _shift(c, dx * s, dy * s)
                if not valid.any():
                    continue
                w = np.full(c.shape[:2], K[abs(dx)] * K[abs(dy)])
                if sigma_colour > 0:
                    w = w * np.exp(-np.sum((c - cq) ** 2, axis=-1) / sc ** 2)
                if sigma_normal > 0:
                    nq, _ = _shift(normal, dx * s, dy * s)
                    w = w * np.exp(-np.sum((normal - nq) ** 2, axis=-1) / sigma_normal ** 2)
                if sigma_depth > 0:
                    dq, _ = _shift(depth, dx * s, dy * s)
                    w = w * np.exp(-(depth - dq) ** 2 / (sigma_depth * np.maximum(depth, DEPTH_FLOOR)) ** 2)
                use = valid.copy()
                if object_stop:
                    iq, _ = _shift(ids, dx * s, dy * s)
                    use &= ids == iq
                # a tap that is not used contributes nothing: its colour is not even multiplied
                num = num + np.where(use[..., None], w[..., None] * np.where(use[..., None], cq, 0.0), 0.0)
                den = den + np.where(use, w, 0.0)
    return num / den[..., None]


def denoise(image, features, **params):
    """The filter over image [H, W, 3] (B, G, R) with the feature buffers `features` (dict of object_id, depth, normal, albedo as
    Renderer.feature_buffers returns them).  Returns (result, working maximum): the result in float64 and the largest finite
    magnitude any iterate took, demodulated where demodulation is on (the M of the error bound)."""
    p = dict(DEFAULTS, **params)
    c = np.asarray(image, np.float64).copy()
    normal = np.asarray(features["normal"], np.float64)
    depth = np.asarray(features["depth"], np.float64)
    ids = np.asarray(features["object_id"])
    factor = np.maximum(np.asarray(features["albedo"], np.float64), ALBEDO_FLOOR) if p["demodulate"] else np.ones_like(c)
    c = c / factor
    finite = np.abs(c[np.isfinite(c)])
    working_max = float(finite.max()) if finite.size else 0.0
    for i in range(int(p["iterations"])):
        c = iteration(c, i, normal, depth, ids, float(p["sigma_colour"]), float(p["sigma_normal"]), float(p["sigma_depth"]),
                      int(p["object_stop"]))
    return c * factor, working_max


def flat_features(H, W, ids=None):
    """Feature buffers of a featureless image: one object (or `ids`), one depth, one normal, albedo 1."""
    return {"object_id": np.zeros((H, W), np.int32) if ids is None else np.asarray(ids, np.int32),
            "depth": np.ones((H, W), np.float32), "normal": np.tile(np.float32([0, 0, 1]), (H, W, 1)),
            "albedo": np.ones((H, W, 3), np.float32)}
