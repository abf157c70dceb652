"""The float64 model of the A-trous filter (tests/denoise_model.py) checked against closed forms on the CPU, so that the yardstick
of tests/test_gpu_denoise.py is trusted before the GPU sees it."""
import numpy as np
import pytest

from tests import denoise_model as M

ALL_OFF = dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, object_stop=0, demodulate=0)


def _two_objects(H, W):
    ids = np.zeros((H, W), np.int32)
    ids[:, W // 2:] = 3
    ids[H // 3: H // 2, 1:4] = -1                     # a patch of misses inside object 0
    return ids


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (17, 33)])
@pytest.mark.parametrize("params", [dict(), ALL_OFF, dict(iterations=6, demodulate=0)])
def test_a_constant_image_is_a_fixed_point(shape, params):
    H, W = shape
    f = M.flat_features(H, W, _two_objects(H, W))
    f["albedo"][..., 1] = 0.25
    img = np.full((H, W, 3), 1.75) * [1.0, 0.5, 2.0]
    out, m = M.denoise(img, f, **params)
    assert np.max(np.abs(out - img)) <= 8 * np.finfo(np.float64).eps * img.max()
    assert m == pytest.approx(img[..., 1].max() / 0.25 if params.get("demodulate", 1) else img.max())


def test_all_stops_off_is_the_b3_convolution_with_renormalised_borders():
    rng = np.random.default_rng(5)
    H, W = 9, 12
    img = rng.uniform(0, 4, (H, W, 3))
    out, _ = M.denoise(img, M.flat_features(H, W), iterations=1, **ALL_OFF)
    k1 = np.array([1, 4, 6, 4, 1]) / 16.0
    want = np.zeros_like(img)
    for y in range(H):
        for x in range(W):
            acc, wsum = np.zeros(3), 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        w = k1[dy + 2] * k1[dx + 2]
                        acc += w * img[y + dy, x + dx]
                        wsum += w
            want[y, x] = acc / wsum
    assert np.max(np.abs(out - want)) <= 1e-14
    # ... and the second iteration has holes: step 2
    out2, _ = M.denoise(img, M.flat_features(H, W), iterations=2, **ALL_OFF)
    y, x = 4, 6
    acc = sum(k1[dy + 2] * k1[dx + 2] * out[y + 2 * dy, x + 2 * dx] for dy in range(-2, 3) for dx in range(-2, 3))
    assert np.abs(out2[y, x] - acc).max() <= 1e-14    # every tap inside: the weights sum to 1


@pytest.mark.parametrize("iterations", [1, 3, 6])
def test_object_stop_keeps_every_object_within_its_own_range(iterations):
    rng = np.random.default_rng(9)
    H, W = 17, 33
    ids = _two_objects(H, W)
    f = M.flat_features(H, W, ids)
    img = rng.uniform(0, 1, (H, W, 3))
    img[ids == 3] += 10.0                             # disjoint ranges: any leak shows
    img[ids == -1] += 100.0
    out, _ = M.denoise(img, f, iterations=iterations, demodulate=0)
    for k in np.unique(ids):
        m = ids == k
        for ch in range(3):
            assert img[m, ch].min() - 1e-12 <= out[m, ch].min() and out[m, ch].max() <= img[m, ch].max() + 1e-12
    leaky, _ = M.denoise(img, f, iterations=iterations, demodulate=0, object_stop=0, sigma_colour=0.0)
    assert leaky[ids == 0].max() > 2.0                # the property is the stop's doing
    # a NaN on one object stays there
    img[0, 0] = np.nan
    out, _ = M.denoise(img, f, iterations=iterations, demodulate=0)
    assert np.isnan(out[0, 0]).all() and np.isfinite(out[ids != 0]).all()
