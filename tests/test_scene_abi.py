"""Runtime scene (pt_set_scene / pt_get_scene): the C-ABI, the binding, the built-in table against the oracle and the CLI's
--scene checks, without a GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_set_scene", "pt_get_scene")


def test_scene_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    S = ptmi_lib.SceneObject
    assert C.sizeof(S) == 48 and ptmi_lib.SCENE_DTYPE.itemsize == 48
    assert [(n, S.__dict__[n].offset) for n, _ in S._fields_] == [
        ("shape", 0), ("material", 4), ("centre", 8), ("radius", 20), ("normal", 24), ("colour", 36)]
    assert [(n, ptmi_lib.SCENE_DTYPE.fields[n][1]) for n in ptmi_lib.SCENE_DTYPE.names] == [
        ("shape", 0), ("material", 4), ("centre", 8), ("radius", 20), ("normal", 24), ("colour", 36)]
    for name in ("set_scene", "scene"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80
    assert C.sizeof(ptmi_lib.Layer) == 32 and ptmi_lib.TRACE_DTYPE.itemsize == 20 and ptmi_lib.PATH_DTYPE.itemsize == 48


def test_null_handle(ptmi_lib):
    lib = ptmi_lib.load_library()
    objs = ptmi_lib.builtin_scene()
    assert lib.pt_set_scene(None, objs.ctypes.data, len(objs)) == -1
    assert lib.pt_set_scene(None, None, 0) == -1
    n = C.c_uint32(99)
    assert lib.pt_get_scene(None, None, 0, C.byref(n)) == 0 and n.value == 6   # size query
    small = np.zeros(5, dtype=ptmi_lib.SCENE_DTYPE)
    assert lib.pt_get_scene(None, small.ctypes.data, 5, C.byref(n)) == -1
    assert lib.pt_get_scene(None, small.ctypes.data, 5, None) == -1


def test_builtin_scene_matches_the_oracle(ptmi_lib, oracle):
    """The six objects of codelets.cpp:111-144 as the library hands them out equal the oracle's table bit for bit."""
    s = ptmi_lib.builtin_scene()
    assert len(s) == 6
    L = oracle.lib()
    for i in range(6):
        cc, col = np.zeros(3, np.float32), np.zeros(3, np.float32)
        rad, ty = C.c_float(), C.c_int32()
        L.orc_scene_object(i, cc.ctypes.data, C.byref(rad), col.ctypes.data, C.byref(ty))
        assert np.array_equal(s[i]["centre"], cc), i
        assert s[i]["radius"] == np.float32(rad.value), i
        assert np.array_equal(s[i]["colour"], col), i
        assert s[i]["material"] == ty.value & 0xff, i
        assert s[i]["shape"] == (ptmi_lib.SHAPE_DISC if ty.value >> 8 else ptmi_lib.SHAPE_SPHERE), i
        exp_n = [0, 1, 0] if s[i]["shape"] == ptmi_lib.SHAPE_DISC else [0, 0, 0]
        assert np.array_equal(s[i]["normal"], np.float32(exp_n)), i
    assert list(s["material"]) == [0, 1, 2, 0, 2, 0]


def test_scene_array_from_dicts(ptmi_lib):
    a = ptmi_lib.scene_array([
        {"shape": "sphere", "material": "emissive", "centre": (1, 2, 3), "radius": 0.5, "emission": (4, 5, 6)},
        {"shape": "disc", "material": "specular", "centre": (0, -1, 0), "radius": 2, "normal": (0, 2, 0)},
        {"shape": 0, "material": 2, "centre": (0, 0, -3), "radius": 1, "colour": (0.5, 0.5, 0.5)}])
    assert list(a["shape"]) == [0, 1, 0] and list(a["material"]) == [3, 1, 2]
    assert list(a[0]["colour"]) == [4, 5, 6] and list(a[1]["colour"]) == [1, 1, 1] and list(a[1]["normal"]) == [0, 2, 0]
    with pytest.raises(ValueError):
        ptmi_lib.scene_array([{"shape": "sphere", "material": "diffuse", "centre": (0, 0, 0), "radius": 1, "color": (1, 1, 1)}])
    with pytest.raises(KeyError):
        ptmi_lib.scene_array([{"shape": "cube", "material": "diffuse", "centre": (0, 0, 0), "radius": 1}])


def test_header_states_the_scene_contract():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("int pt_set_scene(pt_handle h, const pt_scene_object* objects, uint32_t n);",
              "int pt_get_scene(pt_handle h, pt_scene_object* out, uint32_t capacity, uint32_t* n);",
              "#define PT_MAX_SCENE_OBJECTS 32", "typedef struct pt_scene_object", "PT_MATERIAL_EMISSIVE = 3",
              "PT_SHAPE_DISC = 1", "#define PTMI_ABI_VERSION 5"):
        assert s in text, s
    scene = text[text.index("Runtime scene"):text.index("int pt_get_scene")]
    flat = " ".join(scene.replace("*", " ").split())
    for s in ("EXTENSION", "compile-time", "n outside 1..32", "shape or material out of range", "not finite", "radius <= 0",
              "negative colour component", "disc normal of length zero", "previous scene stays in force",
              "n / sqrtf(dot(n, n))", "bit-identically to no call", "next pt_path_trace / pt_trace_paths",
              "does not touch the worklist", "NIF memo", "paths that reached the environment", "= NIF evaluations",
              "does not count emitter paths", "escaped = 2", "h == NULL gives the built-in table"):
        assert s in flat, s
    memo = text[text.index("Persistent memo of NIF evaluations"):text.index("int pt_get_nif_memo_stats")]
    assert "not pt_set_scene" in " ".join(memo.replace("*", " ").split())


def _exe():
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return exe


GOOD = [{"shape": "sphere", "centre": [0, 0, -3], "radius": 1, "material": "diffuse", "colour": [1.6, 1.6, 1.6]},
        {"shape": "disc", "centre": [0, -1.6, -5], "normal": [0, 1, 0], "radius": 3.5, "material": "specular"},
        {"shape": "sphere", "centre": [2, 3, -4], "radius": 0.3, "material": "emissive", "emission": [8, 8, 8]}]


def _with(i, **kw):
    objs = json.loads(json.dumps(GOOD))
    objs[i].update(kw)
    return json.dumps({"objects": objs})


def test_cli_lists_and_validates_scene(tmp_path):
    exe = _exe()
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--scene" in help_text
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    bad = {
        "invalid_json": '{"objects": [',
        "unknown_shape": _with(0, shape="cube"),
        "unknown_material": _with(0, material="glow"),
        "zero_radius": _with(0, radius=0),
        "negative_radius": _with(1, radius=-2),
        "too_many": json.dumps({"objects": [GOOD[0]] * 33}),
        "none": json.dumps({"objects": []}),
        "zero_normal": _with(1, normal=[0, 0, 0]),
        "not_finite": '{"objects": [{"shape": "sphere", "centre": [0, 0, 1e999], "radius": 1, "material": "diffuse"}]}',
        "negative_colour": _with(0, colour=[1, -0.5, 1]),
        "unknown_key": _with(0, color=[1, 1, 1]),
    }
    cases = [("missing", str(tmp_path / "no_such_scene.json"))]
    for name, text in bad.items():
        p = tmp_path / (name + ".json")
        p.write_text(text)
        cases.append((name, str(p)))
    for name, path in cases:
        r = subprocess.run(base + ["--scene", path], capture_output=True, text=True)
        assert r.returncode == 1 and "--scene" in r.stdout, (name, r.returncode, r.stdout[-500:])
        assert "Could not attach" not in r.stdout and "Tracebuffer" not in r.stdout, name
    r = subprocess.run(base + ["--scene", str(tmp_path / "too_many.json")], capture_output=True, text=True)
    assert "object count must be 1..32" in r.stdout
    r = subprocess.run(base + ["--scene", str(tmp_path / "zero_radius.json")], capture_output=True, text=True)
    assert "scene object 0: radius must be > 0" in r.stdout
    r = subprocess.run(base + ["--scene", str(tmp_path / "negative_colour.json")], capture_output=True, text=True)
    assert "scene object 0: colour" in r.stdout
    r = subprocess.run(base + ["--scene", str(tmp_path / "not_finite.json")], capture_output=True, text=True)
    assert "scene object 0: centre must be finite" in r.stdout
    good = tmp_path / "good.json"
    good.write_text(json.dumps({"objects": GOOD}))
    r = subprocess.run(base + ["--scene", str(good), "--compile-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, r.stdout[-500:]
    assert not (tmp_path / "x.png").exists()
