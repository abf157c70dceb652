"""HDR environment map (pt_set_env_map / pt_env_map_lookup): the C-ABI, the binding and the CLI's option checks, without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_set_env_map", "pt_env_map_lookup")


def test_env_map_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    for name in ("set_env_map", "env_map_lookup"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    assert (ptmi_lib.ENV_FILTER_NEAREST, ptmi_lib.ENV_FILTER_BILINEAR) == (0, 1)
    assert ptmi_lib.ENV_FILTERS == {"nearest": 0, "bilinear": 1}
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "enum { PT_ENV_FILTER_NEAREST = 0, PT_ENV_FILTER_BILINEAR = 1 };" in header
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and ptmi_lib.ABI_VERSION == 5
    assert C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80


def test_null_handle(ptmi_lib):
    lib = ptmi_lib.load_library()
    img = np.ones((2, 2, 3), dtype=np.float32)
    assert lib.pt_set_env_map(None, img.ctypes.data, 2, 2, 1) == -1
    assert lib.pt_set_env_map(None, None, 0, 0, 7) == -1
    u = np.zeros(1, dtype=np.float32)
    out = np.zeros(3, dtype=np.float32)
    assert lib.pt_env_map_lookup(None, u.ctypes.data, u.ctypes.data, 1, out.ctypes.data) == -1
    assert lib.pt_env_map_lookup(None, None, None, 0, None) == -1


def _run(args, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return subprocess.run([exe, "--assets", str(tmp_path), "-o", str(tmp_path / "out.png"), "--compile-only"] + args,
                          capture_output=True, text=True, timeout=120)


def _pfm(path, bgr):
    h, w, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(bgr[::-1, :, ::-1], dtype="<f4").tobytes())


def test_cli_validates_the_map_without_a_device(tmp_path):
    good = tmp_path / "sky.pfm"
    _pfm(str(good), np.full((4, 8, 3), 0.5, dtype=np.float32))
    r = _run(["--env-map", str(good)], tmp_path)          # no NIF assets in tmp_path: none are loaded
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "8 x 4" in r.stdout + r.stderr
    r = _run(["--env-map", str(good), "--env-map-filter", "cubic"], tmp_path)
    assert r.returncode != 0 and "--env-map-filter" in r.stdout + r.stderr
    r = _run(["--env-map", str(good), "--constant-env", "1,1,1"], tmp_path)
    assert r.returncode != 0 and "--constant-env" in r.stdout + r.stderr
    cut = tmp_path / "cut.pfm"
    cut.write_bytes(good.read_bytes()[:100])
    r = _run(["--env-map", str(cut)], tmp_path)
    assert r.returncode != 0 and "cut.pfm" in r.stdout + r.stderr and "offset" in r.stdout + r.stderr
    bad = np.full((4, 8, 3), 0.5, dtype=np.float32)
    bad[2, 5, 1] = -1.0
    _pfm(str(tmp_path / "neg.pfm"), bad)
    r = _run(["--env-map", str(tmp_path / "neg.pfm")], tmp_path)
    assert r.returncode != 0 and "row 2, column 5, channel 1" in r.stdout + r.stderr
    r = _run(["--env-map", str(tmp_path / "sky.jpg")], tmp_path)
    assert r.returncode != 0 and "unknown environment-map format" in r.stdout + r.stderr
