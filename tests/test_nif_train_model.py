"""The float64 model of the NIF trainer (tests/nif_train_model.py) checked on its own, without a device: its features against
the oracle's, its gradients against finite differences, its Adam on the procedural map."""
import numpy as np

from ipu_path_trace_amd import nif_assets
from tests import nif_train_model as M


def test_features_equal_the_oracle(oracle):
    rng = np.random.Generator(np.random.Philox(3))
    u = np.concatenate([rng.random(300, dtype=np.float32), np.arange(8, dtype=np.float32) / np.float32(8)])
    v = np.concatenate([rng.random(300, dtype=np.float32), np.arange(8, dtype=np.float32) / np.float32(16)])
    for emb in (2, 12):
        got = M.encode(emb, u, v)
        want = np.stack([oracle.nif_encode(emb, u[i], v[i]) for i in range(u.size)]).astype(np.float64)
        assert np.array_equal(got, want)
        assert np.array_equal(got, got.astype(np.float16).astype(np.float64))          # half values


def test_philox_matches_the_known_answer():
    """Random123's known-answer vectors for philox4x32-10."""
    zero = M.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in zero] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = M.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)
    assert [int(x) for x in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    idx = M.batch_indices(5, 3, 4096, 8, 16)
    assert idx.min() >= 0 and idx.max() < 128 and np.unique(idx).size == 128


def test_analytic_gradients_agree_with_central_differences():
    emb, hidden = 2, 32
    layers = M.cast_layers(nif_assets.synthetic_nif(hidden=hidden, layer_count=2, embedding_dim=emb, dtype=np.float32))
    u, v, _ = M.relu_safe_batch(layers, emb, 64, seed=1)
    feats = M.encode(emb, u, v)
    tgt = np.random.Generator(np.random.Philox(2)).uniform(-1, 1, (64, 3))
    loss, grads = M.loss_and_gradients(layers, feats, tgt)
    rng = np.random.Generator(np.random.Philox(4))
    h = 1e-6
    for l, (k, b, _) in enumerate(layers):
        for arr, g in ((k, grads[l][0]), (b, grads[l][1])):
            for _ in range(6):
                i = tuple(rng.integers(0, s) for s in arr.shape)
                keep = arr[i]
                arr[i] = keep + h
                up = M.loss_and_gradients(layers, feats, tgt)[0]
                arr[i] = keep - h
                down = M.loss_and_gradients(layers, feats, tgt)[0]
                arr[i] = keep
                fd = (up - down) / (2 * h)
                assert abs(fd - g[i]) <= 1e-7 * max(1.0, abs(g[i])) + 1e-9, (l, i, fd, g[i])
    assert loss > 0


def test_adam_fits_the_procedural_map():
    """200 steps at learning rate 1e-3 and batch 256 bring the full-image loss under 0.05 of its initial value."""
    emb = 4
    img = M.procedural_map(8, 16)
    mean, mx = M.encode_params(img)
    tgt = M.targets(img, mean, mx)
    assert abs(np.max(np.abs(tgt)) - 1.0) < 1e-12 and np.allclose(tgt.reshape(-1, 3).mean(axis=0), 0.0, atol=1e-12)
    rng = np.random.Generator(np.random.Philox(9))
    layers = []
    for rows, cols, relu in ((4 * emb, 64, True), (64 + 4 * emb, 64, True), (64, 3, False)):
        lim = np.sqrt(6.0 / (rows + cols))
        layers.append((rng.uniform(-lim, lim, (rows, cols)), np.zeros(cols), relu))
    first = M.image_loss(layers, emb, tgt)
    adam = M.Adam(layers, learning_rate=1e-3)
    for step in range(200):
        u, v, t, _ = M.batch(9, step, 256, tgt)
        adam.step(M.encode(emb, u, v), t)
    last = M.image_loss(adam.layers, emb, tgt)
    print("full-image loss %.4e -> %.4e (ratio %.3e)" % (first, last, last / first))
    assert last <= 0.05 * first
