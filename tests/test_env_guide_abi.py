"""Environment guide (pt_set_env_guide / pt_env_guide_sample / pt_env_guide_eval): the C-ABI, the binding and the CLI's option
checks, without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_set_env_guide", "pt_env_guide_sample", "pt_env_guide_eval")


def test_env_guide_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    for name in ("set_env_guide", "env_guide_sample", "env_guide_eval"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "#define PT_ENV_GUIDE_MAX_ROWS 1024" in header and "#define PT_ENV_GUIDE_MAX_COLS 2048" in header
    assert "#define PT_ENV_GUIDE_MAX_ALPHA 0.9f" in header
    assert (ptmi_lib.ENV_GUIDE_MAX_ROWS, ptmi_lib.ENV_GUIDE_MAX_COLS, ptmi_lib.ENV_GUIDE_MAX_ALPHA) == (1024, 2048, 0.9)
    assert C.sizeof(ptmi_lib.EnvGuide) == 32
    assert ptmi_lib.default_env_guide_grid(64, 32) == (32, 64) and ptmi_lib.default_env_guide_grid(5, 3) == (2, 4)
    assert ptmi_lib.default_env_guide_grid(16384, 8192) == (1024, 2048)
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and ptmi_lib.ABI_VERSION == 5
    assert C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80


def test_null_handle(ptmi_lib):
    lib = ptmi_lib.load_library()
    img = np.ones((2, 2, 3), dtype=np.float32)
    g = ptmi_lib.EnvGuide()
    g.struct_size, g.width, g.height, g.rows, g.cols, g.alpha, g.bgr = C.sizeof(g), 2, 2, 2, 2, 0.5, img.ctypes.data
    assert lib.pt_set_env_guide(None, C.byref(g)) == -1
    assert lib.pt_set_env_guide(None, None) == -1
    w = np.zeros(1, dtype=np.uint32)
    uv, cell, d = np.zeros(2, np.float32), np.zeros(1, np.uint32), np.zeros(3, np.float32)
    assert lib.pt_env_guide_sample(None, w.ctypes.data, w.ctypes.data, w.ctypes.data, 1, uv.ctypes.data, cell.ctypes.data) == -1
    assert lib.pt_env_guide_sample(None, None, None, None, 0, None, None) == -1
    assert lib.pt_env_guide_eval(None, d.ctypes.data, 1, cell.ctypes.data, uv.ctypes.data) == -1
    assert lib.pt_env_guide_eval(None, None, 0, None, None) == -1


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


def test_cli_validates_the_guide_without_a_device(tmp_path):
    sky = tmp_path / "sky.pfm"
    img = np.full((6, 12, 3), 0.5, dtype=np.float32)
    img[1, 3] = 90.0
    _pfm(str(sky), img)
    out = lambda r: r.stdout + r.stderr
    r = _run(["--env-map", str(sky), "--env-guide", "map"], tmp_path)
    assert r.returncode == 0, out(r)[-3000:]
    assert "12 x 6 image, 4 x 8 cells" in out(r)                                   # the default grid
    r = _run(["--env-map", str(sky), "--env-guide", str(sky), "--env-guide-size", "2x4", "--env-guide-alpha", "0.25"], tmp_path)
    assert r.returncode == 0 and "2 x 4 cells, alpha 0.25" in out(r), out(r)[-3000:]
    r = _run(["--constant-env", "1,1,1", "--env-guide", str(sky)], tmp_path)          # a guide needs no map: it is sampling, not light
    assert r.returncode == 0, out(r)[-3000:]
    r = _run(["--constant-env", "1,1,1", "--env-guide", "map"], tmp_path)
    assert r.returncode != 0 and "--env-guide map needs --env-map" in out(r)
    for size, field in (("3x8", "rows"), ("4x6", "cols"), ("8x8", "rows"), ("4x16", "cols"), ("4", "--env-guide-size"),
                        ("4x8x2", "--env-guide-size")):
        r = _run(["--env-map", str(sky), "--env-guide", "map", "--env-guide-size", size], tmp_path)
        assert r.returncode != 0 and field in out(r), (size, out(r)[-2000:])
    for alpha in ("0.95", "-0.5", "nan"):
        r = _run(["--env-map", str(sky), "--env-guide", "map", "--env-guide-alpha", alpha], tmp_path)
        assert r.returncode != 0 and "alpha" in out(r), (alpha, out(r)[-2000:])
    black = tmp_path / "black.pfm"
    _pfm(str(black), np.zeros((4, 8, 3), dtype=np.float32))
    r = _run(["--constant-env", "1,1,1", "--env-guide", str(black)], tmp_path)
    assert r.returncode != 0 and "black.pfm" in out(r) and "total mass" in out(r)
    bad = img.copy()
    bad[2, 5, 1] = -1.0
    _pfm(str(tmp_path / "neg.pfm"), bad)
    r = _run(["--constant-env", "1,1,1", "--env-guide", str(tmp_path / "neg.pfm")], tmp_path)
    assert r.returncode != 0 and "row 2, column 5, channel 1" in out(r)
    cut = tmp_path / "cut.pfm"
    cut.write_bytes(sky.read_bytes()[:60])
    r = _run(["--constant-env", "1,1,1", "--env-guide", str(cut)], tmp_path)
    assert r.returncode != 0 and "cut.pfm" in out(r)
    r = _run(["--constant-env", "1,1,1", "--env-guide", str(tmp_path / "sky.jpg")], tmp_path)
    assert r.returncode != 0 and "unknown environment-map format" in out(r)
