"""Triangles and parallelograms in runtime scenes (pt_set_scene_ex / pt_get_scene_ex): the C-ABI, every validation message in
the stated order with a NULL handle, the binding and the CLI's --scene forms, without a GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
OFFSETS = [("shape", 0), ("material", 4), ("centre", 8), ("radius", 20), ("normal", 24), ("colour", 36), ("vertex", 48)]


def test_entry_points_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_scene_ex", "pt_get_scene_ex"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    D = P.SCENE_EX_DTYPE
    assert D.itemsize == 84
    assert [(n, D.fields[n][1]) for n in D.names] == OFFSETS
    assert D.fields["vertex"][0].shape == (3, 3)
    # the first 48 bytes are pt_scene_object, field for field
    assert [(n, D.fields[n][1], D.fields[n][0]) for n in P.SCENE_DTYPE.names] == \
           [(n, P.SCENE_DTYPE.fields[n][1], P.SCENE_DTYPE.fields[n][0]) for n in P.SCENE_DTYPE.names]
    assert (P.SHAPE_TRIANGLE, P.SHAPE_PARALLELOGRAM) == (2, 3)
    for name in ("set_scene", "scene", "scene_ex"):
        assert callable(getattr(P.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.Config) == 56 and C.sizeof(P.Stats) == 80 and C.sizeof(P.SceneObject) == 48
    assert P.SCENE_DTYPE.itemsize == 48 and P.TRACE_DTYPE.itemsize == 20 and P.PATH_DTYPE.itemsize == 48


def _good(P):
    return P.scene_array_ex([
        {"shape": "sphere", "material": "diffuse", "centre": (0, 0, -3), "radius": 1, "colour": (0.5, 0.6, 0.7)},
        {"shape": "disc", "material": "specular", "centre": (0, -1, -3), "radius": 2, "normal": (0, 2, 0)},
        {"shape": "triangle", "material": "emissive", "vertices": ((0, 0, -2), (1, 0, -2), (0, 1, -2)), "emission": (4, 5, 6)},
        {"shape": "parallelogram", "material": "refractive", "vertices": ((-1, -1, -4), (1, -1, -4), (-1, 1, -4))}])


def _rejected(P, table, n=None, stride=84):
    lib = P.load_library()
    ptr = None if table is None else table.ctypes.data
    rc = lib.pt_set_scene_ex(None, ptr, len(table) if n is None else n, stride)
    assert rc == -1
    return lib.pt_last_error(None).decode()


def test_every_validation_message_in_the_stated_order(ptmi_lib):
    """With a NULL handle every check runs and the handle is refused last: each table below carries the fault under test and
    every LATER fault of the list as well, so the message shows the order."""
    P = ptmi_lib
    nan, inf = np.float32("nan"), np.float32("inf")
    t = _good(P)
    assert _rejected(P, t) == "pt_set_scene_ex: null handle"              # 10: a valid table reaches the handle
    bad = t.copy()
    bad[3]["vertex"] = ((0, 0, 0), (1, 1, 1), (2, 2, 2))                   # 9 collinear
    assert _rejected(P, bad) == "scene object 3: vertices are collinear"
    bad[3]["vertex"] = ((0, 0, 0), (0, 0, 0), (1, 2, 3))                   # a zero edge is collinear too
    assert _rejected(P, bad) == "scene object 3: vertices are collinear"
    bad[3]["vertex"] = ((3e38, 0, 0), (-3e38, 0, 0), (0, 1, 0))            # e1 overflows
    assert _rejected(P, bad) == "scene object 3: vertex differences and their cross product must be finite"
    bad[3]["vertex"] = ((0, 0, 0), (1e30, 0, 0), (0, 1e30, 0))             # the cross product overflows
    assert _rejected(P, bad) == "scene object 3: vertex differences and their cross product must be finite"
    bad[3]["vertex"] = ((0, 0, 0), (1, 1, 1), (2, 2, 2))
    bad[1]["normal"] = 0                                                   # 8 the disc rule
    assert _rejected(P, bad) == "scene object 1: disc normal must have a non-zero finite length"
    bad[0]["radius"] = 0                                                   # 8 the sphere rule, an earlier object
    assert _rejected(P, bad) == "scene object 0: radius must be > 0 (got 0)"
    bad[0]["colour"] = (1, -0.5, 1)                                        # 7 before 8 on the same object
    assert _rejected(P, bad) == "scene object 0: colour components must be >= 0 (got -0.5)"
    bad[0]["centre"] = (0, inf, 0)                                         # 6 before 7
    assert _rejected(P, bad) == "scene object 0: centre must be finite (got inf)"
    bad[0]["material"] = 4                                                 # 5 before 6
    assert _rejected(P, bad).startswith("scene object 0: material must be 0 (diffuse), 1 (specular), 2 (refractive) or 3 (emissive) (got 4)")
    bad[0]["shape"] = 4                                                    # 4 before 5
    assert _rejected(P, bad) == "scene object 0: shape must be 0 (sphere), 1 (disc), 2 (triangle) or 3 (parallelogram) (got 4)"
    assert _rejected(P, None, n=4) == "scene: null object table"          # 3
    assert _rejected(P, None, n=33) == "scene: object count must be 1..32 (got 33)"   # 2 before 3
    assert _rejected(P, bad, n=0) == "scene: object count must be 1..32 (got 0)"
    assert _rejected(P, None, n=33, stride=48) == "scene: stride must be 84 (sizeof(pt_scene_object_ex)) (got 48)"   # 1 before 2
    assert _rejected(P, None, n=0) == "pt_set_scene_ex: null handle"      # (NULL, 0, stride) is valid: the built-in scene

    # 6, field by field: a polygon's vertex and colour are checked, its centre, radius and normal are ignored ...
    p = _good(P)
    p[2]["centre"], p[2]["radius"], p[2]["normal"] = (nan, inf, 0), -inf, (nan, nan, nan)
    assert _rejected(P, p) == "pt_set_scene_ex: null handle"
    p[2]["vertex"][1, 2] = nan
    assert _rejected(P, p) == "scene object 2: vertex must be finite (got nan)"
    p = _good(P)
    p[3]["colour"] = (1, 1, inf)
    assert _rejected(P, p) == "scene object 3: colour must be finite (got inf)"
    p = _good(P)
    p[3]["colour"] = (1, 1, -1)
    assert _rejected(P, p) == "scene object 3: colour components must be >= 0 (got -1)"
    # ... and a sphere's or disc's vertex is ignored, its own fields checked as pt_set_scene checks them
    p = _good(P)
    p[0]["vertex"], p[1]["vertex"] = nan, inf
    assert _rejected(P, p) == "pt_set_scene_ex: null handle"
    for field, text in (("radius", "radius"), ("normal", "normal"), ("colour", "colour")):
        p = _good(P)
        p[1][field] = nan
        assert _rejected(P, p) == "scene object 1: %s must be finite (got nan)" % text


def test_pt_set_scene_keeps_its_text_and_refuses_polygons():
    text = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "ptmi_scene.h")).read()
    assert 'shape must be 0 (sphere) or 1 (disc) (got ' in text


def test_get_scene_ex_without_a_handle_is_the_builtin_table(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    n = C.c_uint32(99)
    assert lib.pt_get_scene_ex(None, None, 0, C.byref(n)) == 0 and n.value == 6    # size query
    small = np.zeros(5, dtype=P.SCENE_EX_DTYPE)
    assert lib.pt_get_scene_ex(None, small.ctypes.data, 5, C.byref(n)) == -1
    assert lib.pt_get_scene_ex(None, small.ctypes.data, 5, None) == -1
    ex, plain = P.builtin_scene_ex(), P.builtin_scene()
    assert len(ex) == 6 and not ex["vertex"].any()
    for name in P.SCENE_DTYPE.names:
        assert np.array_equal(ex[name], plain[name]), name


def test_scene_array_ex_forms(ptmi_lib):
    P = ptmi_lib
    a = _good(P)
    assert a.dtype == P.SCENE_EX_DTYPE and list(a["shape"]) == [0, 1, 2, 3] and list(a["material"]) == [0, 1, 3, 2]
    assert a[2]["vertex"].tolist() == [[0, 0, -2], [1, 0, -2], [0, 1, -2]] and list(a[2]["colour"]) == [4, 5, 6]
    assert not a[0]["vertex"].any() and list(a[1]["normal"]) == [0, 2, 0] and list(a[3]["colour"]) == [1, 1, 1]
    assert not a[2]["centre"].any() and a[2]["radius"] == 0
    b = P.scene_array_ex([{"shape": 2, "material": 0, "vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0]]}])      # numbers for names
    assert b[0]["shape"] == 2 and b[0]["vertex"][1, 0] == 1
    assert P.scene_array_ex(a) is a or np.array_equal(P.scene_array_ex(a), a)
    plain = P.builtin_scene()
    up = P.scene_array_ex(plain)                                         # a 48-byte table widens with zero vertices
    assert up.dtype == P.SCENE_EX_DTYPE and not up["vertex"].any() and np.array_equal(up["centre"], plain["centre"])
    assert P.has_polygon(a) and not P.has_polygon(plain) and not P.has_polygon([{"shape": "disc"}])
    with pytest.raises(ValueError):      # a polygon takes no centre
        P.scene_array_ex([{"shape": "triangle", "material": "diffuse", "vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "centre": (0, 0, 0)}])
    with pytest.raises(ValueError):      # ... and a sphere no vertices
        P.scene_array_ex([{"shape": "sphere", "material": "diffuse", "centre": (0, 0, 0), "radius": 1, "vertices": [[0, 0, 0]] * 3}])
    with pytest.raises(ValueError):
        P.scene_array_ex([{"shape": "triangle", "material": "diffuse", "vertices": [[0, 0, 0], [1, 0, 0]]}])
    with pytest.raises(KeyError):
        P.scene_array_ex([{"shape": "cube", "material": "diffuse", "centre": (0, 0, 0), "radius": 1}])
    with pytest.raises(KeyError):        # the 48-byte form does not know the new names
        P.scene_array([{"shape": "triangle", "material": "diffuse", "centre": (0, 0, 0), "radius": 1}])


def test_stored_normal_is_the_binary32_expression(ptmi_lib):
    """The model's copy of the stored table (what the CPU tests trace through) forms n as the header states."""
    from tests import scene_poly_model as PM
    t = PM.stored_scene_ex([{"shape": "triangle", "material": "diffuse", "vertices": ((0.1, 0.2, -2.0), (1.3, 0.1, -2.2), (0.2, 1.1, -1.9))},
                            {"shape": "disc", "material": "diffuse", "centre": (0, 0, -1), "radius": 1, "normal": (0, 3, 4)}])
    f = np.float32
    v = t[0]["vertex"]
    e1, e2 = v[1] - v[0], v[2] - v[0]
    c = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    assert np.allclose(t[0]["normal"], c / np.linalg.norm(c), atol=2e-7) and abs(float(np.linalg.norm(t[0]["normal"].astype(np.float64))) - 1) < 2e-7
    assert np.array_equal(t[0]["centre"], v[0]) and t[0]["radius"] == 0
    assert np.array_equal(t[1]["normal"], f([0, 0.6, 0.8])) and not t[1]["vertex"].any()


def test_header_states_the_polygon_contract():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("enum { PT_SHAPE_TRIANGLE = 2, PT_SHAPE_PARALLELOGRAM = 3 };", "typedef struct pt_scene_object_ex",
              "int pt_set_scene_ex(pt_handle h, const pt_scene_object_ex* objects, uint32_t n, uint32_t stride",
              "int pt_get_scene_ex(pt_handle h, pt_scene_object_ex* out, uint32_t capacity, uint32_t* n);",
              "float vertex[3][3];", "#define PTMI_ABI_VERSION 5",
              "int pt_set_scene(pt_handle h, const pt_scene_object* objects, uint32_t n);"):
        assert s in text, s
    part = text[text.index("Polygons in a runtime scene"):text.index("int pt_get_scene_ex")]
    flat = " ".join(part.replace("*", " ").split())
    for s in ("EXTENSION", "84 bytes", "a + b <= 1", "v1 + v2 - v0", "n = c / sqrtf(dot(c, c))", "det == 0 -> miss", "t > 1e-5 else miss",
              "two-sided", "dot(n, d) > 0 ? -n : n", "NOT watertight", "R^T (v0 - position)", "vertices are collinear",
              "previous scene stays in force", "(NULL, 0, stride) restores the built-in scene", "use pt_get_scene_ex",
              "same scene bit for bit", "object_id is the index", "that is, flipped"):
        assert s in flat, s
    guide = text[text.index("Emitter-guided diffuse sampling"):text.index("int pt_set_light_guide")]
    assert "An emissive polygon (pt_set_scene_ex) is skipped by the table" in " ".join(guide.replace("*", " ").split())


def test_light_guide_table_skips_polygons(tmp_path):
    """ptlight::build over a table with an emissive polygon and an emissive sphere lists the sphere alone (a stand-alone host
    program over csrc/ptmi_light_guide.h: no device)."""
    src = tmp_path / "lg.cpp"
    src.write_text('''
#include <cstdio>
#include "ptmi_light_guide.h"
int main() {
  pt_scene_object s[3] = {};
  s[0].shape = PT_SHAPE_PARALLELOGRAM; s[0].material = PT_MATERIAL_EMISSIVE; s[0].colour[0] = s[0].colour[1] = s[0].colour[2] = 5.f;
  s[1].shape = PT_SHAPE_SPHERE; s[1].material = PT_MATERIAL_EMISSIVE; s[1].radius = 0.5f; s[1].colour[0] = s[1].colour[1] = s[1].colour[2] = 2.f;
  s[2].shape = PT_SHAPE_TRIANGLE; s[2].material = PT_MATERIAL_EMISSIVE; s[2].colour[1] = 1.f;
  ptlight::Table T;
  ptlight::build(0.5f, s, 3, T);
  std::printf("%u %u %u %g\\n", T.n, T.n_draw, T.object_index[0], (double)T.probability[0]);
  return 0;
}
''')
    exe = tmp_path / "lg"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["1", "1", "1", "1"]


def _exe():
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return exe


GOOD = [{"shape": "parallelogram", "vertices": [[-2, -1, -1], [2, -1, -1], [-2, -1, -5]], "material": "diffuse", "colour": [0.7, 0.7, 0.7]},
        {"shape": "triangle", "vertices": [[-1, -1, -4], [1, -1, -4], [0, 1, -4]], "material": "specular"},
        {"shape": "sphere", "centre": [0, 0, -3], "radius": 0.5, "material": "refractive"},
        {"shape": "parallelogram", "vertices": [[-0.5, 2, -2.5], [0.5, 2, -2.5], [-0.5, 2, -3.5]], "material": "emissive", "emission": [8, 8, 8]}]


def _with(i, drop=(), **kw):
    objs = json.loads(json.dumps(GOOD))
    objs[i].update(kw)
    for k in drop:
        del objs[i][k]
    return json.dumps({"objects": objs})


def test_cli_accepts_and_validates_polygons(tmp_path):
    exe = _exe()
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "parallelogram" in help_text and "vertices" in help_text
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    bad = {
        "collinear": (_with(1, vertices=[[0, 0, -1], [1, 1, -2], [2, 2, -3]]), "scene object 1: vertices are collinear"),
        "two_points": (_with(1, vertices=[[0, 0, -1], [1, 1, -2]]), "scene object 1: \"vertices\" must be an array of 3 points"),
        "no_vertices": (_with(0, drop=("vertices",)), "scene object 0: \"vertices\" is missing"),
        "centre_on_polygon": (_with(0, centre=[0, 0, 0]), "scene object 0: \"centre\" does not apply"),
        "vertices_on_sphere": (_with(2, vertices=[[0, 0, 0]] * 3), "scene object 2: \"vertices\" does not apply"),
        "not_finite": (_with(3, vertices=[[0, 0, 1e999], [1, 0, 0], [0, 1, 0]]), "scene object 3: vertex must be finite"),
        "negative_colour": (_with(0, colour=[1, -1, 1]), "scene object 0: colour components must be >= 0"),
        "zero_radius": (_with(2, radius=0), "scene object 2: radius must be > 0"),
        "unknown_shape": (_with(0, shape="quad"), "unknown shape 'quad' (sphere, disc, triangle, parallelogram)"),
    }
    for name, (text, message) in bad.items():
        p = tmp_path / (name + ".json")
        p.write_text(text)
        r = subprocess.run(base + ["--scene", str(p)], capture_output=True, text=True)
        assert r.returncode == 1 and "--scene" in r.stdout and message in r.stdout, (name, r.returncode, r.stdout[-600:])
        assert "Could not attach" not in r.stdout and "Tracebuffer" not in r.stdout, name      # refused before a device is attached
    good = tmp_path / "good.json"
    good.write_text(json.dumps({"objects": GOOD}))
    r = subprocess.run(base + ["--scene", str(good), "--compile-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, r.stdout[-500:]
