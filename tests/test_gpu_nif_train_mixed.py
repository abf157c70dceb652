"""The trainer's mixed-precision mode (pt_nif_train_set_precision, include/ptmi.h) against the numpy model of
tests/nif_train_mixed_model.py, which follows the header's contract literally.

The tolerances are imported from tests/test_nif_train_mixed_model.py, where they are calibrated on these very inputs without a
GPU: 8 x the difference between numpy's binary32 order and binary64-then-rounded sums of the same model."""
import ctypes as C

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import nif_train_mixed_model as X
from tests import nif_train_model as M
from tests.test_nif_train_mixed_model import (ADAM_SCALE, ADAM_SEED, ADAM_TOL, GRAD_CASES, GRAD_TOL, LOSS_TOL, SHAPES, SKIP_GROWTH, SKIP_SCALE,
                                              SKIP_SEED, SKIP_SHAPE, adam_run, grad_errors, gradient_inputs, model_gradients, skip_run)

pytestmark = pytest.mark.gpu

NIF_RTOL = 2e-2            # the suite's NIF tolerance (half-precision inference against the oracle)
NOT_READY = -5


def _renderer(ptmi_lib, img, size=32):
    r = ptmi_lib.Renderer(size, size, max_path_length=6)
    r.set_env_map(img, "nearest")
    return r


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("shape,scale,n", GRAD_CASES)
def test_gradients_against_the_mixed_model(ptmi_lib, shape, scale, n):
    emb, hidden, count, batch = shape
    layers, u, v, tgt, rejected = gradient_inputs(shape)
    assert rejected <= 0.10
    want_loss, want, info = model_gradients(shape, scale, n)
    r = _renderer(ptmi_lib, M.procedural_map())
    t = r.train_nif(embedding_dim=emb, hidden=hidden, layer_count=count, batch=batch, precision={"mode": "mixed", "loss_scale": scale, "dynamic": 0})
    t.set_weights(layers)
    before, state = t.weights(), t.precision_state()
    assert state == {"mode": "mixed", "loss_scale": scale, "good_steps": 0, "applied_steps": 0, "skipped_steps": 0}
    loss, got = t.gradients(u[:n], v[:n], tgt[:n])
    errs = grad_errors(got, want)
    print("shape %s S %g n %d: %d subnormal scaled gradients in the model, loss rel %.2e (bound %.2e), gradient errors %s (bound %.2e)"
          % (shape, scale, n, info["subnormal"], abs(loss - want_loss) / want_loss, LOSS_TOL, " ".join("%.2e" % e for e in errs), GRAD_TOL[shape]))
    assert abs(loss - want_loss) <= LOSS_TOL * want_loss
    assert max(errs) <= GRAD_TOL[shape]
    assert _same(before, t.weights()) and t.precision_state() == state                # the hook moves no weight and no state
    assert all(np.array_equal(a[0], np.asarray(l[0], np.float32)) for a, l in zip(before, layers))
    t.set_precision("f32")                                                             # and it is not the float answer
    _, f32 = t.gradients(u[:n], v[:n], tgt[:n])
    far = max(grad_errors(got, f32))
    print("    the f32 mode's gradients differ by %.2e in the layer that differs most" % far)
    assert far > GRAD_TOL[shape]
    t.close()
    r.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_adam_steps_against_the_mixed_model(ptmi_lib, shape):
    emb, hidden, count, batch = shape
    layers = gradient_inputs(shape)[0]
    r = _renderer(ptmi_lib, M.procedural_map())
    t = r.train_nif(embedding_dim=emb, hidden=hidden, layer_count=count, batch=batch, seed=ADAM_SEED,
                    precision={"mode": "mixed", "loss_scale": ADAM_SCALE, "dynamic": 0})
    batches = [t.batch(s) for s in range(3)]
    for steps in (1, 3):
        t.set_weights(layers)                                                          # resets the moments and both step counts
        t.steps(steps)
        want = adam_run(shape, steps, np.float64, batches=batches)
        errs = grad_errors(t.weights(), want)
        print("shape %s, %d step(s): weight errors %s (bound %.2e)" % (shape, steps, " ".join("%.2e" % e for e in errs), ADAM_TOL[shape]))
        assert max(errs) <= ADAM_TOL[shape]
        assert t.precision_state() == {"mode": "mixed", "loss_scale": ADAM_SCALE, "good_steps": steps, "applied_steps": steps, "skipped_steps": 0}
        assert not np.array_equal(t.weights()[0][0], np.asarray(layers[0][0], np.float32))
    t.close()
    r.close()


def test_overflow_skips_the_step_and_moves_the_scale(ptmi_lib):
    emb, hidden, count, batch = SKIP_SHAPE
    layers = gradient_inputs(SKIP_SHAPE)[0]
    r = _renderer(ptmi_lib, M.procedural_map())
    t = r.train_nif(embedding_dim=emb, hidden=hidden, layer_count=count, batch=batch, seed=SKIP_SEED,
                    precision={"mode": "mixed", "loss_scale": SKIP_SCALE, "dynamic": 1, "growth_interval": SKIP_GROWTH})
    t.set_weights(layers)
    model, steps, leading = skip_run(batches=t.batch)
    print("model: %d steps, %d leading skipped, margins %s" % (steps, leading, " ".join("%.2f" % m for m in model.margins)))
    assert leading >= 2 and min(model.margins) >= 0.10
    start = t.weights()
    for s in range(steps):
        loss = t.steps(1)
        got = t.precision_state()
        assert np.isfinite(loss)
        assert got == dict(model.history[s], mode="mixed"), "after step %d" % s
        if s < leading:                                                                # skipped: the masters keep their bits, S has halved
            assert _same(start, t.weights()) and got["loss_scale"] == SKIP_SCALE / 2.0 ** (s + 1)
    got = t.precision_state()
    print("after the run: %s" % got)
    assert got["applied_steps"] == SKIP_GROWTH and got["good_steps"] == 0              # one doubling after four applied steps
    assert got["loss_scale"] == 2.0 * model.history[-2]["loss_scale"]
    assert not _same(start, t.weights())
    t.close()
    r.close()


def test_two_mixed_runs_with_one_seed_give_the_same_bits(ptmi_lib):
    img = M.procedural_map()
    out = []
    for seed in (3, 3, 4):
        r = _renderer(ptmi_lib, img)
        t = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, seed=seed, precision="mixed")
        loss = t.steps(20)
        out.append((t.weights(), loss, t.precision_state()))
        t.close()
        r.close()
    (a, la, sa), (b, lb, sb), (c, _, _) = out
    assert la == lb and sa == sb and _same(a, b)
    assert not np.array_equal(a[0][0], c[0][0])


def test_the_float_path_is_untouched(ptmi_lib):
    img = M.procedural_map()
    lib = ptmi_lib.load_library()
    out = []
    for switch in (False, True):
        r = _renderer(ptmi_lib, img)
        if switch:                                                                     # no trainer yet
            p = ptmi_lib.default_nif_train_precision(mode="mixed")
            assert lib.pt_nif_train_set_precision(r.handle, C.byref(p)) == NOT_READY
            assert "no trainer" in lib.pt_last_error(r.handle).decode()
        t = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, seed=3)
        assert t.precision_state() == {"mode": "f32", "loss_scale": 1.0, "good_steps": 0, "applied_steps": 0, "skipped_steps": 0}
        if switch:
            t.set_precision("mixed")
            assert t.precision_state()["mode"] == "mixed" and t.precision_state()["loss_scale"] == 65536.0
            t.set_precision("f32")
        loss = t.steps(20)
        assert t.precision_state() == {"mode": "f32", "loss_scale": 1.0, "good_steps": 0, "applied_steps": 20, "skipped_steps": 0}
        out.append((t.weights(), loss))
        t.close()
        r.close()
    (a, la), (b, lb) = out
    assert la == lb and _same(a, b)


@pytest.fixture(scope="module")
def converged(ptmi_lib):
    """The convergence run of test_gpu_nif_train.py -- the procedural 16 x 8 map, embedding 4, 2 x 64, batch 256, learning rate
    1e-3, 200 steps -- in mixed mode with the default dynamic scale, and the float64 model from the same initial weights on
    the same batches."""
    img = M.procedural_map(8, 16)
    r = _renderer(ptmi_lib, img)
    t = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, learning_rate=1e-3, seed=9, precision="mixed")
    enc = t.encode_params()
    tgt = M.targets(img, np.asarray(enc["mean"], np.float32), np.float32(enc["max"])).astype(np.float32).astype(np.float64)
    start = t.weights()
    adam = M.Adam(start, learning_rate=1e-3)
    for s in range(200):
        u, v, tg = t.batch(s)
        adam.step(M.encode(4, u, v), tg)
    t.steps(200)
    yield {"r": r, "t": t, "img": img, "tgt": tgt, "enc": enc, "start": start, "model": adam.layers}
    t.close()
    r.close()


def test_mixed_training_converges_like_the_float64_model(converged):
    tgt = converged["tgt"]
    first = M.image_loss(converged["start"], 4, tgt)
    last = M.image_loss(converged["t"].weights(), 4, tgt)
    model = M.image_loss(converged["model"], 4, tgt)
    state = converged["t"].precision_state()
    print("full-image loss %.4e -> %.4e (%.3e of the initial value); float64 model %.4e; ratio to the model %.3f; %s"
          % (first, last, last / first, model, last / model, state))
    assert state["applied_steps"] + state["skipped_steps"] == 200
    assert last <= 0.05 * first
    assert last <= 4.0 * model


def test_export_and_install_in_mixed_mode(ptmi_lib, oracle, converged):
    r, t, enc = converged["r"], converged["t"], converged["enc"]
    half = t.export()
    full = t.weights()
    for (hk, hb, _), (fk, fb, _) in zip(half, full):                                   # half(weights()) bit for bit
        assert hk.dtype == np.float16 and np.array_equal(hk, fk.astype(np.float16)) and np.array_equal(hb, fb.astype(np.float16))
    folded = [float(np.float32(np.float32(m) - np.float32(enc["eps"]))) for m in enc["mean"]]
    u, v = M.grid_uv(8, 16)
    t.install()
    installed = r.nif_infer(u, v)
    want = oracle.Nif(half, 4, enc["max"], folded).infer(u, v)
    np.testing.assert_allclose(installed, want, rtol=NIF_RTOL, atol=1e-6)
    r.init_render_settings(samples_per_step=4)                                         # a render runs on it, and training goes on
    work = ptmi_lib.worklist(32, 32)
    r.setup(work)
    r.path_trace()
    st = r.read_results(work)
    assert st.escaped > 0 and np.isfinite(work["r"]).all() and "envmap" not in r.nif_kernel_name()
    before = t.precision_state()
    assert np.isfinite(t.steps(2))
    after = t.precision_state()
    assert after["applied_steps"] + after["skipped_steps"] == before["applied_steps"] + before["skipped_steps"] + 2


def test_mixed_training_leaves_rendering_alone(ptmi_lib):
    img = M.procedural_map(8, 16)
    r = ptmi_lib.Renderer(64, 64, max_path_length=6)
    r.set_env_map(img, "bilinear")

    def film():
        r.init_render_settings(seed=20, samples_per_step=8)
        r.init_render_settings(seed=21, samples_per_step=8)                            # a new seed restarts the sample sequence
        work = ptmi_lib.worklist(64, 64)
        r.setup(work)
        r.path_trace()
        r.read_results(work)
        return work.tobytes()

    before = film()
    t = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, precision="mixed")
    t.steps(5)
    t.close()
    assert film() == before
    r.close()
