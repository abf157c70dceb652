"""Emitter guide (pt_set_light_guide / pt_get_light_guide_info / pt_light_guide_sample / pt_light_guide_eval): the C-ABI, the
binding and the CLI's option checks, without a GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_set_light_guide", "pt_get_light_guide_info", "pt_light_guide_sample", "pt_light_guide_eval")


def test_light_guide_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    for name in ("set_light_guide", "light_guide_info", "light_guide_sample", "light_guide_eval"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "#define PT_LIGHT_GUIDE_MAX_BETA 0.9f" in header and ptmi_lib.LIGHT_GUIDE_MAX_BETA == 0.9
    # pt_light_guide: two 4-byte fields; pt_light_guide_info: five and three arrays of 32
    assert C.sizeof(ptmi_lib.LightGuide) == 8 and C.sizeof(ptmi_lib.LightGuideInfo) == 4 * (5 + 3 * 32)
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and ptmi_lib.ABI_VERSION == 5
    assert C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80


def test_null_handle(ptmi_lib):
    lib = ptmi_lib.load_library()
    g = ptmi_lib.LightGuide(8, 0.5)
    assert lib.pt_set_light_guide(None, C.byref(g)) == -1
    assert lib.pt_set_light_guide(None, None) == -1
    assert lib.pt_set_light_guide(None, C.byref(ptmi_lib.LightGuide(8, 7.0))) == -1
    info = ptmi_lib.LightGuideInfo()
    info.struct_size = C.sizeof(info)
    assert lib.pt_get_light_guide_info(None, C.byref(info)) == -1
    f = np.zeros(3, np.float32)
    w = np.zeros(1, np.uint32)
    assert lib.pt_light_guide_sample(None, f.ctypes.data, f.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data, 1,
                                     f.ctypes.data, w.ctypes.data) == -1
    assert lib.pt_light_guide_sample(None, None, None, None, None, None, 0, None, None) == -1
    assert lib.pt_light_guide_eval(None, f.ctypes.data, f.ctypes.data, f.ctypes.data, 1, f.ctypes.data, f.ctypes.data) == -1
    assert lib.pt_light_guide_eval(None, None, None, None, 0, None, None) == -1


def _run(args, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return subprocess.run([exe, "--assets", str(tmp_path), "-o", str(tmp_path / "out.png"), "--compile-only", "--constant-env", "1,1,1"] + args,
                          capture_output=True, text=True, timeout=120)


def _pfm(path, bgr):
    h, w, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(bgr[::-1, :, ::-1], dtype="<f4").tobytes())


LAMP_SCENE = {"objects": [
    {"shape": "sphere", "material": "diffuse", "centre": [0, -1, -4], "radius": 1, "colour": [0.8, 0.5, 0.25]},
    {"shape": "sphere", "material": "emissive", "centre": [1.5, 2, -3], "radius": 0.2, "emission": [50, 50, 50]},
    {"shape": "disc", "material": "emissive", "centre": [-2, 1, -4], "radius": 0.3, "normal": [0.2, -1, 0.1], "emission": [20, 20, 20]}]}


def test_cli_validates_beta_without_a_device(tmp_path):
    out = lambda r: r.stdout + r.stderr
    r = _run([], tmp_path)
    assert r.returncode == 0 and "light guide" not in out(r), out(r)[-3000:]           # the default 0 means off
    r = _run(["--light-guide-beta", "0.5"], tmp_path)                                   # the built-in scene has no emitter
    assert r.returncode == 0 and "light guide: inactive: the scene has no emitter" in out(r), out(r)[-3000:]
    for beta in ("0.95", "-0.5", "nan", "inf"):
        r = _run(["--light-guide-beta", beta], tmp_path)
        assert r.returncode != 0 and "beta must be in" in out(r), (beta, out(r)[-2000:])
    sky = tmp_path / "sky.pfm"
    img = np.full((6, 12, 3), 0.5, dtype=np.float32)
    img[1, 3] = 90.0
    _pfm(str(sky), img)
    r = _run(["--env-guide", str(sky), "--env-guide-alpha", "0.5", "--light-guide-beta", "0.5"], tmp_path)
    assert r.returncode != 0 and "alpha + beta" in out(r), out(r)[-2000:]
    r = _run(["--env-guide", str(sky), "--env-guide-alpha", "0.5", "--light-guide-beta", "0.4"], tmp_path)
    assert r.returncode == 0, out(r)[-3000:]
    scene = tmp_path / "lamps.json"
    scene.write_text(json.dumps(LAMP_SCENE))
    r = _run(["--scene", str(scene), "--light-guide-beta", "0.25"], tmp_path)
    assert r.returncode == 0 and "light guide: beta 0.25, 2 emitters" in out(r), out(r)[-3000:]
