"""ipu_trace --train-nif --train-precision mixed on the GPU: the logged loss is finite, the scale and the step counts are
reported, the precision is recorded, and the assets load through --assets."""
import os
import re
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import nif_train_model as M
from tests.test_gpu_nif_train_cli import read_ptnif
from tests.test_nif_train_abi import write_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")


def test_train_nif_in_mixed_precision_writes_assets_that_load(ptmi_lib, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    img = M.procedural_map(8, 16)
    write_pfm(str(tmp_path / "map.pfm"), img)
    out = tmp_path / "trained"
    r = subprocess.run([exe, "--train-nif", str(tmp_path / "map.pfm"), "--train-steps", "50", "--train-out", str(out), "--train-layer-size", "64",
                        "--train-layer-count", "2", "--train-embedding-dimension", "4", "--train-batch", "256", "--train-seed", "9",
                        "--train-precision", "mixed"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    loss = re.search(r"Training step 50 of 50: loss (\S+)", r.stdout)
    assert loss and np.isfinite(float(loss.group(1)))
    done = re.search(r"precision mixed, loss scale (\S+), (\d+) steps applied, (\d+) skipped", r.stdout)
    assert done, r.stdout[-2000:]
    assert float(done.group(1)) >= 1.0 and int(done.group(2)) + int(done.group(3)) == 50 and int(done.group(2)) > 0
    assets = out / "assets.extra"
    text = (assets / "nif_metadata.txt").read_text()
    assert '"--train-precision", "mixed"' in text
    meta = nif_assets.load_metadata(str(assets / "nif_metadata.txt"))
    assert (meta["embedding_dimension"], meta["hidden_size"], meta["layer_count"]) == (4, 64, 2)
    # the same model through the binding gives the same weights: the CLI ran the library's mixed step
    rr = ptmi_lib.Renderer(32, 32, max_path_length=6)
    rr.set_env_map(img, "nearest")
    t = rr.train_nif(embedding_dim=4, hidden=64, layer_count=2, batch=256, seed=9, precision="mixed")
    t.steps(50)
    layers, emb = read_ptnif(str(assets / "converted.ptnif"))
    assert emb == 4
    for (k, b, relu), (hk, hb, hrelu) in zip(layers, t.export()):
        assert np.array_equal(k, hk) and np.array_equal(b, hb) and relu == hrelu
    t.close()
    rr.close()
    r = subprocess.run([exe, "--assets", str(assets), "-w", "48", "-h", "32", "-s", "4", "--samples-per-step", "4", "--max-path-length", "6",
                        "-o", str(tmp_path / "img.png"), "--save-interval", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert (tmp_path / "img.exr").exists()
