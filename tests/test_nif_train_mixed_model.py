"""The numpy model of the mixed-precision trainer step (tests/nif_train_mixed_model.py): the calibration of the GPU tolerances,
the model's sensitivity to the mistakes the GPU tests must catch, and the loss-scale state machine.  No GPU.

Calibration: the same mixed model with its sums formed in numpy's binary32 order against binary64-then-rounded,
on the very inputs of tests/test_gpu_nif_train_mixed.py, per tensor and relative to that tensor's largest magnitude.  The
recorded figures are below; the GPU bounds are 8 x those (the factor covers the other summation order of a tiled reduction,
including the activations that fall on the other side of a half rounding).  numpy's binary32 order depends on the BLAS kernels
the host picks, so the test that re-measures them accepts a factor of 4 either way: the bound then still is at least twice what
this host measures."""
import functools

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import nif_train_mixed_model as X
from tests import nif_train_model as M

SHAPES = [(2, 32, 2, 256), (12, 64, 4, 512), (12, 96, 3, 256)]   # embedding, hidden, hidden layers, batch
# (shape, S, n): the gradient cases of the GPU test; S = 1 keeps half subnormals in play, n = 100 is the ragged batch
GRAD_CASES = [(SHAPES[0], 1024.0, 256), (SHAPES[0], 1.0, 256), (SHAPES[1], 1024.0, 512), (SHAPES[1], 1024.0, 100), (SHAPES[2], 1024.0, 256)]

# recorded order differences (this file's test_calibration re-measures and prints them)
GRAD_DIFF = {SHAPES[0]: 8.46e-6, SHAPES[1]: 3.38e-5, SHAPES[2]: 5.75e-5}
LOSS_DIFF = 8.39e-7
ADAM_DIFF = {SHAPES[0]: 9.96e-8, SHAPES[1]: 1.48e-3, SHAPES[2]: 4.90e-5}
GRAD_TOL = {k: 8 * v for k, v in GRAD_DIFF.items()}
LOSS_TOL = 8 * LOSS_DIFF
ADAM_TOL = {k: 8 * v for k, v in ADAM_DIFF.items()}

ADAM_SEED, ADAM_SCALE = 5, 1024.0
SKIP_SHAPE, SKIP_SCALE, SKIP_GROWTH, SKIP_SEED = SHAPES[0], 2.0 ** 30, 4, 5


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


def grad_errors(got, want):
    return [max(rel(g[0], w[0]), rel(g[1], w[1])) for g, w in zip(got, want)]


@functools.lru_cache(maxsize=None)
def gradient_inputs(shape):
    """(layers, u, v, target, rejected share) of one shape: synthetic weights, a ReLU-safe batch selected on the mixed model's
    own pre-activations (seed 7), targets from Philox(11)."""
    emb, hidden, count, batch = shape
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=count, embedding_dim=emb, dtype=np.float32)
    u, v, rejected = X.relu_safe_batch_mixed(layers, emb, batch, seed=7)
    tgt = np.random.Generator(np.random.Philox(11)).uniform(-1, 1, (batch, 3)).astype(np.float32)
    return layers, u, v, tgt, rejected


@functools.lru_cache(maxsize=None)
def model_gradients(shape, scale, n, acc=np.float64, ftz=False):
    layers, u, v, tgt, _ = gradient_inputs(shape)
    return X.loss_and_gradients(layers, M.encode(shape[0], u[:n], v[:n]), tgt[:n], scale, acc, ftz)


def map_targets(img=None):
    """The target image of the procedural 16 x 8 map from the float32 mean and max, rounded to float32 (the library computes the
    same to within a few ulp)."""
    img = M.procedural_map() if img is None else img
    mean, mx = M.encode_params(img)
    return M.targets(img, np.asarray(mean, np.float32), np.float32(mx)).astype(np.float32)


def adam_run(shape, steps, acc, batches=None, seed=ADAM_SEED):
    """The model's weights after `steps` static-scale mixed steps from the synthetic weights, on the trainer's own batches."""
    emb, hidden, count, batch = shape
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=count, embedding_dim=emb, dtype=np.float32)
    tgt = map_targets()
    t = X.Trainer(layers, loss_scale=ADAM_SCALE, dynamic=False, acc=acc)
    for s in range(steps):
        u, v, tg = batches[s] if batches else M.batch(seed, s, batch, tgt)[:3]
        _, applied = t.step(M.encode(emb, u, v), tg)
        assert applied
    return t.layers


def skip_run(batches=None, acc=np.float64):
    """The skip-and-scale run: 2/32/2, batch 256, S = 2^30, dynamic, growth_interval 4, until four steps have been applied.
    Returns (trainer, steps run, leading skipped steps)."""
    emb, hidden, count, batch = SKIP_SHAPE
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=count, embedding_dim=emb, dtype=np.float32)
    tgt = map_targets()
    t = X.Trainer(layers, loss_scale=SKIP_SCALE, dynamic=True, growth_interval=SKIP_GROWTH, acc=acc)
    steps, leading = 0, None
    while t.applied < SKIP_GROWTH:
        u, v, tg = batches(steps) if batches else M.batch(SKIP_SEED, steps, batch, tgt)[:3]
        _, applied = t.step(M.encode(emb, u, v), tg)
        if applied and leading is None:
            leading = steps
        steps += 1
        assert steps < 64
    return t, steps, leading


def test_calibration():
    grad = {s: 0.0 for s in SHAPES}
    loss = 0.0
    for shape, scale, n in GRAD_CASES:
        l64, g64, _ = model_gradients(shape, scale, n)
        l32, g32, _ = model_gradients(shape, scale, n, np.float32)
        e = max(grad_errors(g32, g64))
        le = abs(float(l32) - float(l64)) / float(l64)
        print("gradients %s S %g n %d: order difference %.2e, loss %.2e" % (shape, scale, n, e, le))
        grad[shape], loss = max(grad[shape], e), max(loss, le)
    adam = {}
    for shape in SHAPES:
        adam[shape] = 0.0
        for steps in (1, 3):
            a, b = adam_run(shape, steps, np.float32), adam_run(shape, steps, np.float64)
            e = max(grad_errors(a, b))
            print("Adam %s, %d step(s): order difference %.2e" % (shape, steps, e))
            adam[shape] = max(adam[shape], e)
    print("measured: GRAD_DIFF %s LOSS_DIFF %.2e ADAM_DIFF %s" % ({k: "%.2e" % v for k, v in grad.items()}, loss, {k: "%.2e" % v for k, v in adam.items()}))
    for s in SHAPES:
        assert GRAD_DIFF[s] / 4 <= grad[s] <= 4 * GRAD_DIFF[s]
        assert ADAM_DIFF[s] / 4 <= adam[s] <= 4 * ADAM_DIFF[s]
    assert LOSS_DIFF / 4 <= loss <= 4 * LOSS_DIFF


@pytest.mark.parametrize("shape", SHAPES)
def test_rejection_share(shape):
    rejected = gradient_inputs(shape)[4]
    print("%s: rejected %.3f" % (shape, rejected))
    assert rejected <= 0.10


def test_the_scale_cancels_where_no_half_is_subnormal():
    """g = g_scaled / S is the same bits for S = 1024 and S = 65536 -- both powers of two, so every product, sum and rounding
    scales exactly -- as long as no scaled gradient falls below the half's normal range at the smaller scale, where it loses
    bits the larger scale keeps.  The batch is the first of seeds 7, 8, ... on which the model meets no such value at S = 1024;
    on the GPU test's own batch (seed 7) the model counts them and the gradients may differ in those few elements."""
    emb, hidden, count, batch = SHAPES[0]
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=count, embedding_dim=emb, dtype=np.float32)
    tgt = np.random.Generator(np.random.Philox(11)).uniform(-1, 1, (batch, 3)).astype(np.float32)
    for seed in range(7, 40):
        u, v, _ = X.relu_safe_batch_mixed(layers, emb, batch, seed=seed)
        feats = M.encode(emb, u, v)
        _, small, info = X.loss_and_gradients(layers, feats, tgt, 1024.0, np.float32)
        print("seed %d: %d subnormal scaled gradients at S = 1024" % (seed, info["subnormal"]))
        if info["subnormal"] == 0:
            break
    else:
        pytest.fail("no batch without subnormal gradients")
    _, large, info = X.loss_and_gradients(layers, feats, tgt, 65536.0, np.float32)
    assert info["subnormal"] == 0 and X.finite(large)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(small, large))


def test_flushing_subnormal_halves_leaves_the_bound():
    shape = SHAPES[0]
    _, want, info = model_gradients(shape, 1.0, 256)
    _, got, _ = model_gradients(shape, 1.0, 256, np.float64, True)
    e = max(grad_errors(got, want))
    print("S = 1, halves flushed to zero: %.2e against the bound %.2e (%d subnormal gradients)" % (e, GRAD_TOL[shape], info["subnormal"]))
    assert info["subnormal"] > 0 and e > GRAD_TOL[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_float32_trainers_answer_leaves_the_bound(shape):
    layers, u, v, tgt, _ = gradient_inputs(shape)
    _, want, _ = model_gradients(shape, 1024.0, shape[3])
    _, f32 = M.loss_and_gradients(layers, M.encode(shape[0], u, v), tgt)
    e = max(grad_errors(f32, want))
    print("%s: the float32 trainer's gradients differ by %.2e in the layer that differs most, bound %.2e" % (shape, e, GRAD_TOL[shape]))
    assert e > GRAD_TOL[shape]


def test_overflow_is_skipped_and_the_scale_halves():
    layers, u, v, tgt, _ = gradient_inputs(SHAPES[0])
    feats = M.encode(2, u, v)
    _, grads, _ = X.loss_and_gradients(layers, feats, tgt, 2.0 ** 30)
    assert not X.finite(grads)
    t = X.Trainer(layers, loss_scale=2.0 ** 30, dynamic=True)
    before = [(k.copy(), b.copy()) for k, b, _ in t.layers]
    loss, applied = t.step(feats, tgt)
    assert not applied and np.isfinite(loss)
    assert t.state() == {"loss_scale": 2.0 ** 29, "good_steps": 0, "applied_steps": 0, "skipped_steps": 1}
    assert all(np.array_equal(k, a) and np.array_equal(b, c) for (k, b, _), (a, c) in zip(t.layers, before))
    s = X.Trainer(layers, loss_scale=2.0 ** 30, dynamic=False)
    s.step(feats, tgt)
    assert s.state() == {"loss_scale": 2.0 ** 30, "good_steps": 0, "applied_steps": 0, "skipped_steps": 1}
    one = X.Trainer(layers, loss_scale=1.0, dynamic=True)     # the floor
    one.S = 1.0
    _, grads, _ = X.loss_and_gradients(layers, feats, tgt * np.float32(1e30), 1.0)
    assert not X.finite(grads)
    one.step(feats, tgt * np.float32(1e30))
    assert one.state()["loss_scale"] == 1.0 and one.state()["skipped_steps"] == 1


def test_the_scale_grows_after_growth_interval_applied_steps():
    layers, u, v, tgt, _ = gradient_inputs(SHAPES[0])
    feats = M.encode(2, u, v)
    t = X.Trainer(layers, loss_scale=1024.0, dynamic=True, growth_interval=2)
    t.step(feats, tgt)
    assert t.state() == {"loss_scale": 1024.0, "good_steps": 1, "applied_steps": 1, "skipped_steps": 0}
    t.step(feats, tgt)
    assert t.state() == {"loss_scale": 2048.0, "good_steps": 0, "applied_steps": 2, "skipped_steps": 0}
    cap = X.Trainer(layers, loss_scale=2.0 ** 30, dynamic=True, growth_interval=1)
    _, applied = cap.step(feats, X.forward(layers, feats)[0])  # y - t = 0: finite at any scale, and the cap holds
    assert applied and cap.state()["loss_scale"] == 2.0 ** 30
    fixed = X.Trainer(layers, loss_scale=1024.0, dynamic=False, growth_interval=1)
    fixed.step(feats, tgt)
    assert fixed.state() == {"loss_scale": 1024.0, "good_steps": 1, "applied_steps": 1, "skipped_steps": 0}


def test_the_skip_runs_seed_keeps_its_distance_from_the_half_maximum():
    """The GPU skip test follows the model's verdict step by step; that is safe only where the largest scaled gradient is not
    near 65504, the point at which another summation order could turn the verdict.  Every step of the run -- the last skipped
    and the first applied one among them -- keeps 10 % distance."""
    t, steps, leading = skip_run()
    print("skip run: %d steps, %d leading skipped, state %s, margins %s" % (steps, leading, t.state(), " ".join("%.2f" % m for m in t.margins)))
    assert leading >= 2 and t.applied == SKIP_GROWTH
    assert min(t.margins) >= 0.10
    assert t.state()["good_steps"] == 0 and t.state()["loss_scale"] == SKIP_SCALE / 2.0 ** t.skipped * 2.0
