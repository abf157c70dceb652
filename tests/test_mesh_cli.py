"""`ipu_trace --scene` with "shape": "mesh" without a GPU: a bad mesh is refused before any device is attached, with the library's
own message or the reader's; a good file passes --compile-only; "scale" and "translate" are documented."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
V = [[0, 0, -2], [1, 0, -2], [0, 1, -2], [1, 1, -2.5]]
T = [[0, 1, 2], [1, 3, 2]]
GOOD = [{"shape": "sphere", "centre": [0, 0, -3], "radius": 0.5, "material": "refractive"},
        {"shape": "mesh", "material": "diffuse", "colour": [0.7, 0.6, 0.5], "vertices": V, "triangles": T, "scale": 0.5, "translate": [0, 0.1, -1]},
        {"shape": "mesh", "material": "emissive", "emission": [4, 4, 4], "file": "lamp.obj", "scale": [1, 1, 2]}]
OBJ = "v -0.5 2 -2.5\nv 0.5 2 -2.5\nv 0.5 2 -3.5\nv -0.5 2 -3.5\nf 1/1 2/1 3/1 4/1\n"


def _exe():
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return exe


def _with(i, drop=(), **kw):
    objs = json.loads(json.dumps(GOOD))
    objs[i].update(kw)
    for k in drop:
        del objs[i][k]
    return json.dumps({"objects": objs})


def test_cli_accepts_and_validates_meshes(tmp_path):
    exe = _exe()
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "\"mesh\"" in help_text and "triangles" in help_text and "x.obj" in help_text
    assert "\"scale\"" in help_text and "\"translate\"" in help_text and "binary32 on the host" in help_text
    (tmp_path / "lamp.obj").write_text(OBJ)
    (tmp_path / "broken.obj").write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    bad = {
        "collinear": (_with(1, vertices=[[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]]), "scene object 1, mesh 0, triangle 0: vertices are collinear"),
        "index": (_with(1, triangles=[[0, 1, 4]]), "scene object 1, mesh 0, triangle 0: indices[2] must be < n_vertices = 4 (got 4)"),
        "negative_index": (_with(1, triangles=[[0, 1, -1]]), "scene object 1: \"triangles\" must hold non-negative integers"),
        "no_triangles": (_with(1, drop=("triangles",)), "scene object 1: a mesh needs \"file\", or \"vertices\" and \"triangles\""),
        "empty": (_with(1, triangles=[]), "scene object 1: \"triangles\" must be a non-empty array"),
        "both": (_with(2, vertices=V, triangles=T), "scene object 2: give \"file\" or \"vertices\" and \"triangles\", not both"),
        "centre_on_mesh": (_with(1, centre=[0, 0, 0]), "scene object 1: \"centre\" does not apply to a mesh"),
        "file_on_sphere": (_with(0, file="lamp.obj"), "scene object 0: \"file\" does not apply to a sphere"),
        "scale_on_sphere": (_with(0, scale=2), "scene object 0: \"scale\" does not apply to a sphere"),
        "missing_file": (_with(2, file="nothing.obj"), "nothing.obj: cannot open the file"),
        "broken_file": (_with(2, file="broken.obj"), "broken.obj: line 3: vertex index 3 with 2 vertices read so far"),
        "not_finite": (_with(1, scale=1e39), "scene object 1, mesh 0, triangle 0: vertices[0] must be finite"),
        "negative_colour": (_with(1, colour=[1, -1, 1]), "scene object 1: colour components must be >= 0"),
        "unknown_shape": (_with(1, shape="quad"), "unknown shape 'quad' (sphere, disc, triangle, parallelogram), or mesh"),
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
