"""`ipu_trace --scene` with "normals" on a mesh, without a GPU: bad normals are refused before any device is attached, with the
library's own message (ptmesh::check_normals) or the reader's; good ones pass --compile-only; the keys are documented."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
V = [[0, 0, -2], [1, 0, -2], [0, 1, -2], [1, 1, -2.5]]
T = [[0, 1, 2], [1, 3, 2]]
N = [[0, 0, 1], [0, 0.1, 1], [0.1, 0, 1], [0, 0, 2]]
GOOD = [{"shape": "sphere", "centre": [0, 0, -3], "radius": 0.5, "material": "refractive"},
        {"shape": "mesh", "material": "diffuse", "vertices": V, "triangles": T, "normals": N, "scale": 0.5, "translate": [0, 0.1, -1]},
        {"shape": "mesh", "material": "specular", "file": "quad.obj", "normals": "file"},
        {"shape": "mesh", "material": "diffuse", "vertices": V, "triangles": T, "normals": N[:2], "normal_indices": [[0, 1, 0], [1, 1, 0]]}]
OBJ = "v -0.5 2 -2.5\nv 0.5 2 -2.5\nv 0.5 2 -3.5\nv -0.5 2 -3.5\nvn 0 -1 0\nvn 0.1 -1 0\nf 1//1 2//2 3//1 4//-1\n"


def _with(i, drop=(), **kw):
    objs = json.loads(json.dumps(GOOD))
    objs[i].update(kw)
    for k in drop:
        del objs[i][k]
    return json.dumps({"objects": objs})


def test_cli_accepts_and_validates_mesh_normals(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "\"normals\"" in help_text and "\"normal_indices\"" in help_text and "non-uniform" in help_text
    (tmp_path / "quad.obj").write_text(OBJ)
    (tmp_path / "partial.obj").write_text(OBJ + "f 1 2 3\n")
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    nan_n = json.loads(json.dumps(N))
    bad = {
        "zero": (_with(1, normals=[[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]]), "mesh 0: triangle 0: normals[1] must have a finite dot(n, n) > 0 (got 0)"),
        "not_finite": (_with(1, normals=[[0, 0, 1], [0, 0, 1], [0, 0, 1], [1e39, 0, 1]]), "mesh 0: triangle 1: normals[3] must be finite (got inf)"),
        "count": (_with(1, normals=N[:3]), "mesh 0: n_normals must equal n_vertices = 4 when normal_indices is null (got 3)"),
        "index": (_with(3, normal_indices=[[0, 1, 0], [1, 2, 0]]), "mesh 2: triangle 1: normal_indices[1] must be < n_normals = 2 (got 2)"),
        "index_rows": (_with(3, normal_indices=[[0, 1, 0]]), "scene object 3: \"normal_indices\" must hold one index triple per triangle"),
        "negative_index": (_with(3, normal_indices=[[0, 1, 0], [1, -1, 0]]), "scene object 3: \"normal_indices\" must hold non-negative integers"),
        "indices_alone": (_with(3, drop=("normals",)), "scene object 3: \"normal_indices\" needs \"normals\""),
        "shape": (_with(1, normals=[[0, 0, 1, 0]] * 4), "scene object 1: \"normals\" must hold arrays of 3 numbers"),
        "word": (_with(2, normals="smooth"), "scene object 2: \"normals\" must be \"file\" or an array of directions"),
        "file_without_file": (_with(1, normals="file"), "scene object 1: \"normals\": \"file\" needs \"file\""),
        "file_with_indices": (_with(2, normal_indices=[[0, 0, 0], [0, 0, 0]]), "scene object 2: \"normal_indices\" does not apply to \"normals\": \"file\""),
        "face_without_normal": (_with(2, file="partial.obj"), "partial.obj: line 8: a face corner without a normal index"),
        "non_uniform_scale": (_with(1, scale=[1, 2, 1]), "scene object 1: a non-uniform \"scale\" cannot be combined with \"normals\""),
        "on_a_sphere": (_with(0, normals=N), "scene object 0: \"normals\" does not apply to a sphere"),
    }
    for name, (text, message) in bad.items():
        p = tmp_path / (name + ".json")
        p.write_text(text)
        r = subprocess.run(base + ["--scene", str(p)], capture_output=True, text=True)
        assert r.returncode == 1 and "--scene" in r.stdout and message in r.stdout, (name, r.returncode, r.stdout[-600:])
        assert "Could not attach" not in r.stdout and "Tracebuffer" not in r.stdout, name      # refused before a device is attached
    for name, text in (("good", json.dumps({"objects": GOOD})), ("flat_with_vn", _with(2, drop=("normals",))),
                       ("uniform_triple", _with(1, scale=[2, 2, 2]))):
        p = tmp_path / (name + ".json")
        p.write_text(text)
        r = subprocess.run(base + ["--scene", str(p), "--compile-only"], capture_output=True, text=True)
        assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, (name, r.stdout[-500:])
