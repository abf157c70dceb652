"""The on-device NIF trainer (pt_nif_train_*, include/ptmi.h) against the float64 model of tests/nif_train_model.py.

Calibrated tolerances.  The same model run in numpy float32 against float64 on the very inputs of these tests
gives, per tensor and relative to that tensor's largest magnitude,
    gradients   7.86e-7  (shapes 2/32/2, 12/64/4, 12/96/3: 2.63e-7, 7.30e-7, 7.86e-7)
    loss        3.46e-8  relative
    Adam        2.49e-6  (weights after 1 and 3 steps on the trainer's own batches; 12/96/3 is the largest)
and the bounds below are 8 x those: the factor covers the other summation order of a tiled reduction."""
import ctypes as C

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import nif_train_model as M

pytestmark = pytest.mark.gpu

GRAD_TOL = 8 * 7.86e-7
LOSS_TOL = 8 * 3.46e-8
ADAM_TOL = 8 * 2.49e-6
NIF_RTOL = 2e-2            # the suite's NIF tolerance (half-precision inference against the oracle)
NOT_READY = -5

SHAPES = [(2, 32, 2, 256), (12, 64, 4, 512), (12, 96, 3, 256)]   # embedding, hidden, hidden layers, batch


def _renderer(ptmi_lib, img, size=32):
    r = ptmi_lib.Renderer(size, size, max_path_length=6)
    r.set_env_map(img, "nearest")
    return r


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


def _library_targets(img, enc):
    """The float64 formula with the library's float32 mean and max, rounded to float32."""
    return M.targets(img, np.asarray(enc["mean"], np.float32), np.float32(enc["max"])).astype(np.float32)


@pytest.mark.parametrize("height,width", [(3, 5), (32, 64)])
def test_batch_and_encode_params(ptmi_lib, height, width):
    img = M.procedural_map(height, width)
    r = _renderer(ptmi_lib, img)
    t = r.train_nif(embedding_dim=2, hidden=32, layer_count=2, batch=256, seed=5)
    enc = t.encode_params()
    mean, mx = M.encode_params(img)
    assert np.max(np.abs(np.asarray(enc["mean"]) - mean) / np.abs(mean)) <= 1e-6 and abs(enc["max"] - mx) / mx <= 1e-6
    want_t = _library_targets(img, enc).reshape(-1, 3)
    hit = np.zeros(height * width, bool)
    worst = 0.0
    for step in range(8):
        u, v, tg = t.batch(step)
        rr, cc = np.rint(u * height).astype(np.int64), np.rint(v * width).astype(np.int64)
        assert rr.min() >= 0 and rr.max() < height and cc.min() >= 0 and cc.max() < width
        assert np.array_equal(u, rr.astype(np.float32) / np.float32(height)) and np.array_equal(v, cc.astype(np.float32) / np.float32(width))
        idx = rr * width + cc
        assert np.array_equal(idx, M.batch_indices(5, step, 256, height, width))      # the documented Philox draw
        ulp = np.spacing(np.abs(want_t[idx]))
        worst = max(worst, float(np.max(np.abs(tg.astype(np.float64) - want_t[idx]) / ulp)))
        hit[idx] = True
    print("targets: worst error %.2f ulp" % worst)
    assert worst <= 4.0
    a, b = t.batch(3), t.batch(3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(t.batch(3)[0], t.batch(4)[0]) or not np.array_equal(t.batch(3)[1], t.batch(4)[1])
    if height * width == 15:
        assert hit.all()
    t.close()
    r.close()


@pytest.mark.parametrize("emb,hidden,count,batch", SHAPES)
def test_gradients_against_the_float64_model(ptmi_lib, emb, hidden, count, batch):
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=count, embedding_dim=emb, dtype=np.float32)
    u, v, rejected = M.relu_safe_batch(layers, emb, batch, seed=7)
    assert rejected <= 0.10
    tgt = np.random.Generator(np.random.Philox(11)).uniform(-1, 1, (batch, 3)).astype(np.float32)
    want_loss, want = M.loss_and_gradients(layers, M.encode(emb, u, v), tgt)
    r = _renderer(ptmi_lib, M.procedural_map())
    t = r.train_nif(embedding_dim=emb, hidden=hidden, layer_count=count, batch=batch)
    t.set_weights(layers)
    before = t.weights()
    loss, got = t.gradients(u, v, tgt)
    errs = [max(_rel(g[0], w[0]), _rel(g[1], w[1])) for g, w in zip(got, want)]
    print("shape %s: rejected %.3f, loss rel %.2e, gradient errors %s" % ((emb, hidden, count, batch), rejected, abs(loss - want_loss) / want_loss,
                                                                            " ".join("%.2e" % e for e in errs)))
    assert abs(loss - want_loss) <= LOSS_TOL * want_loss
    assert max(errs) <= GRAD_TOL
    after = t.weights()                                                                # the hook moves nothing
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, after))
    assert all(np.array_equal(a[0], np.asarray(l[0], np.float32)) for a, l in zip(after, layers))
    t.close()
    r.close()


@pytest.mark.parametrize("emb,hidden,count,batch", SHAPES)
def test_adam_steps_against_the_float64_model(ptmi_lib, emb, hidden, count, batch):
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=count, embedding_dim=emb, dtype=np.float32)
    r = _renderer(ptmi_lib, M.procedural_map())
    t = r.train_nif(embedding_dim=emb, hidden=hidden, layer_count=count, batch=batch, seed=5)
    batches = [t.batch(s) for s in range(3)]
    for steps in (1, 3):
        t.set_weights(layers)                                                          # resets the moments and the step counter
        t.steps(steps)
        adam = M.Adam(layers, learning_rate=1e-3)
        for s in range(steps):
            u, v, tg = batches[s]
            adam.step(M.encode(emb, u, v), tg)
        errs = [max(_rel(g[0], w[0]), _rel(g[1], w[1])) for g, w in zip(t.weights(), adam.layers)]
        print("shape %s, %d step(s): weight errors %s" % ((emb, hidden, count, batch), steps, " ".join("%.2e" % e for e in errs)))
        assert max(errs) <= ADAM_TOL
        assert not np.array_equal(t.weights()[0][0], np.asarray(layers[0][0], np.float32))
    t.close()
    r.close()


def test_two_runs_with_one_seed_give_the_same_bits(ptmi_lib):
    img = M.procedural_map()
    out = []
    for seed in (3, 3, 4):
        r = _renderer(ptmi_lib, img)
        t = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, seed=seed)
        loss = t.steps(20)
        out.append((t.weights(), loss))
        t.close()
        r.close()
    (a, la), (b, lb), (c, _) = out
    assert la == lb and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert not np.array_equal(a[0][0], c[0][0])


@pytest.fixture(scope="module")
def converged(ptmi_lib):
    """The convergence run of the issue: the procedural 16 x 8 map, embedding 4, 2 x 64, batch 256, learning rate 1e-3, 200
    steps -- and the float64 model from the same initial weights on the same batches.  The renderer stays open for the export
    and install checks."""
    img = M.procedural_map(8, 16)
    r = _renderer(ptmi_lib, img)
    t = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, learning_rate=1e-3, seed=9)
    enc = t.encode_params()
    tgt = _library_targets(img, enc).astype(np.float64)
    start = t.weights()
    adam = M.Adam(start, learning_rate=1e-3)
    for s in range(200):
        u, v, tg = t.batch(s)
        adam.step(M.encode(4, u, v), tg)
    t.steps(200)
    yield {"r": r, "t": t, "img": img, "tgt": tgt, "enc": enc, "start": start, "model": adam.layers}
    t.close()
    r.close()


def test_training_converges_like_the_float64_model(converged):
    tgt = converged["tgt"]
    first = M.image_loss(converged["start"], 4, tgt)
    last = M.image_loss(converged["t"].weights(), 4, tgt)
    model = M.image_loss(converged["model"], 4, tgt)
    print("full-image loss %.4e -> %.4e (%.3e of the initial value); float64 model %.4e; ratio to the model %.3f"
          % (first, last, last / first, model, last / model))
    # Glorot weights differ by kind: every kernel inside its limit, zero biases
    for (k, b, _), (rows, cols, _) in zip(converged["start"], converged["t"].shapes):
        lim = np.sqrt(6.0 / (rows + cols))
        assert np.all(np.abs(k) <= lim) and np.std(k) > 0.4 * lim and not b.any()
    assert last <= 0.05 * first
    assert last <= 4.0 * model


def test_export_and_install(ptmi_lib, oracle, converged):
    r, t, enc = converged["r"], converged["t"], converged["enc"]
    half = t.export()
    full = t.weights()
    for (hk, hb, _), (fk, fb, _) in zip(half, full):                                   # round to nearest even
        assert hk.dtype == np.float16 and np.array_equal(hk, fk.astype(np.float16)) and np.array_equal(hb, fb.astype(np.float16))
    folded = [float(np.float32(np.float32(m) - np.float32(enc["eps"]))) for m in enc["mean"]]
    u, v = M.grid_uv(8, 16)
    t.install()
    installed = r.nif_infer(u, v)
    name = r.nif_kernel_name()
    assert name and "envmap" not in name
    r.init_nif_weights(half, 4, enc["max"], folded, log_tonemap=True)
    uploaded = r.nif_infer(u, v)
    assert np.array_equal(installed, uploaded)
    want = oracle.Nif(half, 4, enc["max"], folded).infer(u, v)
    np.testing.assert_allclose(installed, want, rtol=NIF_RTOL, atol=1e-6)
    # the installed NIF reproduces the map: the float64 forward pass of the float32 weights, decoded, bounds the fit; the
    # half-precision path adds the suite's 2e-2
    y, _, _ = M.forward(full, M.encode(4, u, v))
    decoded = np.exp(y * enc["max"] + np.asarray(folded))
    texels = converged["img"].reshape(-1, 3).astype(np.float64)
    fit = float(np.max(np.abs(decoded - texels) / texels))
    got = float(np.max(np.abs(installed - texels) / texels))
    print("map reproduction: float64 forward pass of the float32 weights %.3e relative, installed binary16 NIF %.3e" % (fit, got))
    assert got <= fit + NIF_RTOL
    # a render runs on the installed NIF, and training goes on after the install
    r.init_render_settings(samples_per_step=4)
    work = ptmi_lib.worklist(32, 32)
    r.setup(work)
    r.path_trace()
    st = r.read_results(work)
    assert st.escaped > 0 and np.isfinite(work["r"]).all() and "envmap" not in r.nif_kernel_name()
    assert np.isfinite(t.steps(2))


def test_training_leaves_rendering_alone(ptmi_lib):
    img = M.procedural_map(8, 16)
    r = ptmi_lib.Renderer(64, 64, max_path_length=6)
    lib = ptmi_lib.load_library()
    p = ptmi_lib.default_nif_train_params(embedding_dim=4, hidden=64, layer_count=2, batch=256)
    assert lib.pt_nif_train_begin(r.handle, C.byref(p)) == NOT_READY                    # no map yet
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
    t = r.train_nif(p)
    t.steps(5)
    t.close()
    assert film() == before
    loss = C.c_float()
    assert lib.pt_nif_train_steps(r.handle, 1, C.byref(loss)) == NOT_READY              # after end: an error, not a crash
    assert "no trainer" in lib.pt_last_error(r.handle).decode()
    r.close()


def test_a_new_trainer_retires_the_old_object(ptmi_lib):
    r = _renderer(ptmi_lib, M.procedural_map())
    old = r.train_nif(embedding_dim=2, hidden=32, layer_count=2, batch=256)
    new = r.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256)
    with pytest.raises(ptmi_lib.PtError):
        old.steps(1)
    old.close()                                                                        # must not end the handle's (new) trainer
    assert np.isfinite(new.steps(2)) and new.shapes[0][:2] == (16, 64)
    new.close()
    with pytest.raises(ptmi_lib.PtError):
        new.steps(1)
    r.close()
