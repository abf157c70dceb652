"""ipu_trace --train-nif on the GPU: an HDR image in, assets out, and a render with --assets on them."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import nif_train_model as M
from tests.test_nif_train_abi import write_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")


def read_ptnif(path):
    """The inverse of nif_assets.write_ptnif: ([(kernel, bias, relu)], embedding_dim)."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"PTNIF1\0\0"
    n, emb = struct.unpack_from("<II", raw, 8)
    at, layers = 16, []
    for _ in range(n):
        rows, cols, dtype, relu, has_bias = struct.unpack_from("<IIIII", raw, at)
        at += 20
        dt = np.float32 if dtype else np.float16
        k = np.frombuffer(raw, dt, rows * cols, at).reshape(rows, cols)
        at += k.nbytes
        b = None
        if has_bias:
            b = np.frombuffer(raw, dt, cols, at)
            at += b.nbytes
        layers.append((k, b, bool(relu)))
    assert at == len(raw)
    return layers, emb


def test_train_nif_writes_assets_that_render(ptmi_lib, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    img = M.procedural_map(8, 16)
    write_pfm(str(tmp_path / "map.pfm"), img)
    out = tmp_path / "trained"
    r = subprocess.run([exe, "--train-nif", str(tmp_path / "map.pfm"), "--train-steps", "50", "--train-out", str(out), "--train-layer-size", "64",
                        "--train-layer-count", "2", "--train-embedding-dimension", "4", "--train-batch", "256", "--train-seed", "9"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Training step 50 of 50: loss" in r.stdout
    assets = out / "assets.extra"
    assert (assets / "nif_metadata.txt").exists() and (assets / "converted.ptnif").exists()
    # the metadata round-trips the trainer's values: the same model through the Python binding gives the same numbers
    meta = nif_assets.load_metadata(str(assets / "nif_metadata.txt"))
    rr = ptmi_lib.Renderer(32, 32, max_path_length=6)
    rr.set_env_map(img, "nearest")
    t = rr.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, seed=9)
    enc = t.encode_params()
    t.steps(50)
    assert meta["max"] == enc["max"] and meta["eps"] == enc["eps"] and meta["log_tone_map"]
    assert meta["mean_folded"] == [float(np.float32(np.float32(m) - np.float32(enc["eps"]))) for m in enc["mean"]]
    assert (meta["embedding_dimension"], meta["hidden_size"], meta["layer_count"]) == (4, 64, 2) and meta["original_image_shape"] == [8, 16, 3]
    layers, emb = read_ptnif(str(assets / "converted.ptnif"))
    assert emb == 4 and [k.shape for k, _, _ in layers] == [(16, 64), (80, 64), (64, 3)]
    for (k, b, relu), (hk, hb, hrelu) in zip(layers, t.export()):                       # deterministic: the CLI trained the same model
        assert np.array_equal(k, hk) and np.array_equal(b, hb) and relu == hrelu
    t.close()
    # a render with --assets on the result against the Python film made from the same weights
    W, H, spp = 48, 32, 4
    r = subprocess.run([exe, "--assets", str(assets), "-w", str(W), "-h", str(H), "-s", str(spp), "--samples-per-step", str(spp),
                        "--max-path-length", "6", "-o", str(tmp_path / "img.png"), "--save-interval", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    subprocess.check_call(["make", "-C", HOST, "-s"])
    host = C.CDLL(os.path.join(HOST, "libpthost.so"))
    host.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=np.float32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert host.pth_read_exr(str(tmp_path / "img.exr").encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    rr.close()
    py = ptmi_lib.Renderer(W, H, max_path_length=6)
    py.init_nif_weights(layers, emb, meta["max"], meta["mean_folded"], log_tonemap=True)
    py.init_render_settings(samples_per_step=spp)
    work = ptmi_lib.worklist(W, H)
    py.setup(work)
    py.path_trace()
    py.read_results(work)
    py.close()
    inv = np.float32(1.0) / work["sampleCount"].astype(np.float32)
    want = np.stack([work["b"] * inv, work["g"] * inv, work["r"] * inv], -1).reshape(H, W, 3)
    assert np.array_equal(film, want)
