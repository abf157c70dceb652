"""Polygon lamps of the emitter guide (pt_set_light_guide_ex / pt_get_light_guide_flags): the header, the host table with vertices,
the validation order, the exported symbols, the binding and the CLI's option, without a GPU."""
import ctypes as C
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from tests import light_guide_poly_model as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
CSRC = os.path.join(ROOT, "ipu_path_trace_amd", "csrc")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("enum { PT_LIGHT_GUIDE_POLYGONS = 1 };", "typedef struct pt_light_guide_ex {", "uint32_t flags;",
              "int pt_set_light_guide_ex(pt_handle h, const pt_light_guide_ex* g);",
              "int pt_get_light_guide_flags(pt_handle h, uint32_t* flags);", "#define PTMI_ABI_VERSION 5"):
        assert s in text, s
    # the new names come after pt_set_light_guide, whose own paragraph keeps its sentence and says where the switch is
    assert text.index("int pt_set_light_guide(") < text.index("PT_LIGHT_GUIDE_POLYGONS")
    guide = " ".join(text[text.index("Emitter-guided diffuse sampling"):text.index("int pt_set_light_guide")].replace("*", " ").split())
    assert "An emissive polygon (pt_set_scene_ex) is skipped by the table unless pt_set_light_guide_ex asks for polygons" in guide
    part = " ".join(text[text.index("Polygon lamps"):text.index("int pt_get_light_guide_flags")].replace("*", " ").split())
    for s in ("EXTENSION", "PTMI_ABI_VERSION stays 5", "pt_set_light_guide_ex with flags = 0", "S = sqrtf(dot(c, c))", "0.5 S (triangle)",
              "m_k = Y(colour_k) 2 A_p / pi", "reach = fmaxf(0, fmaxf(d1, d2))", "fmaxf(0, d1) + fmaxf(0, d2)", "|hgt| > 1e-5 and d0 + reach > 0",
              "if a + b > 1 then a = 1 - a, b = 1 - b", "(kTwoPi (l2 l)) / (|hgt| A_p)", "(kTwoPi (t t)) / (|dn| A_p)", "epsilon included",
              "The rim rule", "flipped normal", "not recomputed under a camera", "a flags bit other than PT_LIGHT_GUIDE_POLYGONS",
              "the previous guide and its flags stay in force", "0 without one"):
        assert s in part, s


def test_entry_points_are_exported_and_bound(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_light_guide_ex", "pt_get_light_guide_flags"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert C.sizeof(P.LightGuideEx) == 12 and [f[0] for f in P.LightGuideEx._fields_] == ["struct_size", "beta", "flags"]
    assert P.LIGHT_GUIDE_POLYGONS == 1
    sig = inspect.signature(P.Renderer.set_light_guide)
    assert sig.parameters["polygons"].default is False and callable(P.Renderer.light_guide_flags)
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.LightGuide) == 8 and C.sizeof(P.LightGuideInfo) == 404
    assert C.sizeof(P.Config) == 56 and C.sizeof(P.Stats) == 80 and C.sizeof(P.SceneObject) == 48


def _rejected(P, size, beta, flags):
    lib = P.load_library()
    g = P.LightGuideEx(size, beta, flags)
    assert lib.pt_set_light_guide_ex(None, C.byref(g)) == -1
    return lib.pt_last_error(None).decode()


def test_validation_order_and_messages_without_a_device(ptmi_lib):
    """With a NULL handle every check runs and the handle is refused last; each guide carries the fault under test and every
    later one.  (alpha + beta needs an environment guide on a handle: the stand-alone program checks it, and the GPU test.)"""
    P = ptmi_lib
    nan = float("nan")
    assert _rejected(P, 12, 0.5, 1) == "pt_set_light_guide_ex: null handle"
    assert _rejected(P, 12, 0.5, 0) == "pt_set_light_guide_ex: null handle"
    assert _rejected(P, 12, 0.0, 1) == "pt_set_light_guide_ex: null handle"
    assert _rejected(P, 12, 0.5, 6) == "light guide: flags must be 0 or PT_LIGHT_GUIDE_POLYGONS (1) (got 6)"
    assert _rejected(P, 12, 0.5, 0x80000001) == "light guide: flags must be 0 or PT_LIGHT_GUIDE_POLYGONS (1) (got 2147483649)"
    assert _rejected(P, 12, nan, 6) == "light guide: beta must be in [0, 0.9] (got nan)"
    assert _rejected(P, 12, 0.95, 6) == "light guide: beta must be in [0, 0.9] (got 0.95)"
    assert _rejected(P, 12, -0.5, 1).startswith("light guide: beta must be in [0, 0.9]")
    assert _rejected(P, 12, float("inf"), 1).startswith("light guide: beta must be in [0, 0.9]")
    assert _rejected(P, 8, nan, 6) == "light guide: struct_size must be 12 (got 8)"
    assert _rejected(P, 0, 0.5, 1) == "light guide: struct_size must be 12 (got 0)"
    lib = P.load_library()
    assert lib.pt_set_light_guide_ex(None, None) == -1 and lib.pt_last_error(None).decode() == "pt_set_light_guide_ex: null handle"
    flags = C.c_uint32(7)
    assert lib.pt_get_light_guide_flags(None, C.byref(flags)) == -1 and flags.value == 0
    assert lib.pt_get_light_guide_flags(None, None) == -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """light_guide_poly_main, built with the sanitizers: nothing is loaded into Python."""
    out = str(tmp_path_factory.mktemp("light_guide_poly") / "light_guide_poly_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out, os.path.join(ROOT, "tests", "light_guide_poly_main.cpp")])
    return out


def test_check_order_and_table_under_the_sanitizers(exe):
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-3000:]


def _mixed_lamps():
    """Sphere / disc / triangle / parallelogram lamps in turn among diffuse objects, one emitter in five black, random sizes."""
    rng = np.random.default_rng(21)
    objs = []
    for i in range(32):
        kind = i % 4
        emits = i % 3 != 2
        col = tuple(float(x) for x in (np.zeros(3) if (emits and i % 5 == 0) else rng.uniform(0.1, 9.0, 3).astype(np.float32)))
        o = dict(material="emissive" if emits else "diffuse", colour=col)
        if kind == 0:
            o.update(shape="sphere", centre=tuple(rng.uniform(-3, 3, 3)), radius=float(rng.uniform(0.05, 0.6)))
        elif kind == 1:
            o.update(shape="disc", centre=tuple(rng.uniform(-3, 3, 3)), radius=float(rng.uniform(0.05, 0.6)), normal=tuple(rng.normal(size=3)))
        else:
            v0 = rng.uniform(-3, 3, 3)
            o.update(shape="triangle" if kind == 2 else "parallelogram",
                     vertices=(tuple(v0), tuple(v0 + rng.uniform(-1, 1, 3)), tuple(v0 + rng.uniform(-1, 1, 3))))
        objs.append(o)
    return objs


def _lines(P, objs):
    t = P.scene_array_ex(objs)
    return ["%d %d " % (o["shape"], o["material"]) + " ".join("%.9g" % x for x in
            list(o["centre"]) + [o["radius"]] + list(o["normal"]) + list(o["colour"]) + list(o["vertex"].ravel())) for o in t]


@pytest.mark.parametrize("scene", ["two_polygons", "mixed_32", "black_polygon_last"])
def test_the_header_table_equals_the_model(exe, ptmi_lib, scene):
    """ptlight::build with vertices lists the polygons with the model's masses, thresholds and p_k; the four-argument call over
    the same table still skips them."""
    sphere = dict(shape="sphere", material="emissive", centre=(0, 1, -2), radius=0.25, colour=(3.0, 2.0, 1.0))
    rect = dict(shape="parallelogram", material="emissive", vertices=((-0.5, 3, -0.5), (0.5, 3, -0.5), (-0.5, 3, 0.5)), colour=(6.0, 4.5, 3.0))
    tri = dict(shape="triangle", material="emissive", vertices=((0, 2, 0), (2, 2.5, 0), (2, 2.5, 0.01)), colour=(50.0, 50.0, 50.0))
    objs = {"two_polygons": [rect, dict(rect, material="diffuse"), sphere, tri], "mixed_32": _mixed_lamps(),
            "black_polygon_last": [sphere, tri, dict(rect, colour=(0.0, 0.0, 0.0))]}[scene]
    stored = [LP.stored([dict(o, vertices=o["vertices"])])[0] if LP.is_polygon(o) else o for o in objs]
    for mode in ("vertices", "plain"):
        r = subprocess.run([exe, "table", "0.3", mode], input="\n".join(_lines(ptmi_lib, objs)) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [x.split() for x in r.stdout.strip().split("\n")]
        T = LP.Table(stored, 0.3, polygons=mode == "vertices")
        n, n_draw, beta_thr, active, polygons = (int(x) for x in rows[0])
        assert (n, n_draw, beta_thr, bool(active), bool(polygons)) == (T.n, T.n_draw, T.beta_thr, T.active, T.lists_polygon)
        assert len(rows) == 1 + T.n
        for k, row in enumerate(rows[1:]):
            assert int(row[0]) == T.index[k] and int(row[1]) == int(T.threshold[k]) and int(row[2]) == int(T.weight[k]), (mode, k, row)
            assert np.float32(row[3]) == T.p[k] and abs(float(row[4]) - T.mass[k]) <= 1e-15 * max(T.mass[k], 1e-300), (mode, k, row)
        if mode == "vertices":
            assert polygons and any(LP.is_polygon(objs[i]) for i in T.index)
        else:
            assert not polygons and not any(LP.is_polygon(objs[i]) for i in T.index)


def _run(args, tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return subprocess.run([exe, "--assets", str(tmp_path), "-o", str(tmp_path / "out.png"), "--compile-only", "--constant-env", "1,1,1"] + args,
                          capture_output=True, text=True, timeout=120)


BOX = {"objects": [
    {"shape": "parallelogram", "vertices": [[-2, -1, -1], [2, -1, -1], [-2, -1, -5]], "material": "diffuse", "colour": [0.7, 0.7, 0.7]},
    {"shape": "sphere", "centre": [0, 0, -3], "radius": 0.5, "material": "emissive", "emission": [2, 2, 2]},
    {"shape": "parallelogram", "vertices": [[-0.5, 2, -2.5], [0.5, 2, -2.5], [-0.5, 2, -3.5]], "material": "emissive", "emission": [8, 8, 8]},
    {"shape": "triangle", "vertices": [[-1, 1, -4], [1, 1, -4], [0, 2, -4]], "material": "emissive", "emission": [1, 2, 3]}]}


def test_cli_option_and_its_error(tmp_path):
    out = lambda r: r.stdout + r.stderr
    exe = os.path.join(HOST, "ipu_trace")
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--light-guide-polygons" in help_text
    scene = tmp_path / "box.json"
    scene.write_text(json.dumps(BOX))
    r = _run(["--scene", str(scene), "--light-guide-polygons"], tmp_path)                       # no beta: an error naming the option
    assert r.returncode != 0 and "--light-guide-polygons needs --light-guide-beta > 0" in out(r), out(r)[-2000:]
    assert "Could not attach" not in out(r)
    r = _run(["--scene", str(scene), "--light-guide-polygons", "--light-guide-beta", "0"], tmp_path)
    assert r.returncode != 0 and "--light-guide-polygons" in out(r), out(r)[-2000:]
    r = _run(["--scene", str(scene), "--light-guide-beta", "0.25"], tmp_path)                  # the default: the sphere alone
    assert r.returncode == 0 and "light guide: beta 0.25, 1 emitters" in out(r) and "polygons included" not in out(r), out(r)[-3000:]
    r = _run(["--scene", str(scene), "--light-guide-beta", "0.25", "--light-guide-polygons"], tmp_path)
    assert r.returncode == 0 and "light guide: beta 0.25, 3 emitters, polygons included" in out(r), out(r)[-3000:]
    r = _run(["--light-guide-beta", "0.25", "--light-guide-polygons"], tmp_path)                # the built-in scene: accepted, inert
    assert r.returncode == 0 and "light guide: inactive: the scene has no emitter" in out(r), out(r)[-3000:]
