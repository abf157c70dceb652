"""`ipu_trace --scene` with "texture" on a mesh, without a GPU: a bad texture is refused before any device is attached, with the
library's own message (ptmesh::check_texture), the OBJ reader's or the image reader's; good ones pass --compile-only; the keys and
the limit to linear float images are documented."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.mesh_texture_fixtures import write_pfm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
V = [[0, 0, -2], [1, 0, -2], [0, 1, -2], [1, 1, -2.5]]
T = [[0, 1, 2], [1, 3, 2]]
UV = [[0, 0], [1, 0], [0, 1], [1.5, -0.25]]
GOOD = [{"shape": "sphere", "centre": [0, 0, -3], "radius": 0.5, "material": "refractive"},
        {"shape": "mesh", "material": "diffuse", "vertices": V, "triangles": T, "texture": "tex.pfm", "uvs": UV, "scale": [0.5, 1, 0.5]},
        {"shape": "mesh", "material": "emissive", "file": "quad.obj", "texture": "tex.pfm", "uvs": "file", "texture_filter": "nearest",
         "texture_wrap": "clamp"},
        {"shape": "mesh", "material": "diffuse", "vertices": V, "triangles": T, "texture": "tex.pfm", "uvs": UV[:2],
         "uv_indices": [[0, 1, 0], [1, 1, 0]], "normals": [[0, 0, 1]] * 4}]
OBJ = "v -0.5 2 -2.5\nv 0.5 2 -2.5\nv 0.5 2 -3.5\nv -0.5 2 -3.5\nvt 0 0\nvt 1 0.5\nvn 0 -1 0\nf 1/1/1 2/2/1 3/1/1 4/-1/1\n"


def _with(i, drop=(), **kw):
    objs = json.loads(json.dumps(GOOD))
    objs[i].update(kw)
    for k in drop:
        del objs[i][k]
    return json.dumps({"objects": objs})


def test_cli_accepts_and_validates_mesh_textures(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    for word in ("\"texture\"", "\"uvs\"", "\"uv_indices\"", "\"texture_filter\"", "\"texture_wrap\"", "no sRGB decoding"):
        assert word in help_text, word
    (tmp_path / "quad.obj").write_text(OBJ)
    (tmp_path / "partial.obj").write_text(OBJ + "f 1//1 2//1 3//1\n")
    image = 0.25 + np.arange(45, dtype=np.float32).reshape(3, 5, 3) / 64
    write_pfm(tmp_path / "tex.pfm", image)
    negative = image.copy()
    negative[1, 2, 0] = -1.0
    write_pfm(tmp_path / "negative.pfm", negative)
    (tmp_path / "tex.png").write_bytes(b"\x89PNG\r\n\x1a\n")
    (tmp_path / "short.pfm").write_bytes(b"PF\n5 3\n-1.0\n" + b"\0" * 20)
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    bad = {
        "texel": (_with(1, texture="negative.pfm"), "mesh 0: texture: texel (row 1, column 2) channel 0 must be finite and >= 0 (got -1)"),
        "count": (_with(1, uvs=UV[:3]), "mesh 0: texture: n_uvs must equal n_vertices = 4 when uv_indices is null (got 3)"),
        "not_finite": (_with(1, uvs=[[0, 0], [1, 0], [0, 1], [1e39, 0]]), "mesh 0: triangle 1: uvs[3] must be finite (got inf)"),
        "index": (_with(3, uv_indices=[[0, 1, 0], [1, 2, 0]]), "mesh 2: triangle 1: uv_indices[1] must be < n_uvs = 2 (got 2)"),
        "index_rows": (_with(3, uv_indices=[[0, 1, 0]]), "scene object 3: \"uv_indices\" must hold one index triple per triangle"),
        "negative_index": (_with(3, uv_indices=[[0, 1, 0], [1, -1, 0]]), "scene object 3: \"uv_indices\" must hold non-negative integers"),
        "uvs_alone": (_with(1, drop=("texture",)), "scene object 1: \"uvs\" needs \"texture\""),
        "filter_alone": (_with(0, texture_filter="nearest", shape="mesh", vertices=V, triangles=T, drop=("centre", "radius")),
                         "scene object 0: \"texture_filter\" needs \"texture\""),
        "texture_alone": (_with(1, drop=("uvs",)), "scene object 1: \"texture\" needs \"uvs\""),
        "shape": (_with(1, uvs=[[0, 0, 1]] * 4), "scene object 1: \"uvs\" must hold arrays of 2 numbers"),
        "word": (_with(2, uvs="obj"), "scene object 2: \"uvs\" must be \"file\" or an array of (s, t) pairs"),
        "file_without_file": (_with(1, uvs="file"), "scene object 1: \"uvs\": \"file\" needs \"file\""),
        "file_with_indices": (_with(2, uv_indices=[[0, 0, 0], [0, 0, 0]]), "scene object 2: \"uv_indices\" does not apply to \"uvs\": \"file\""),
        "face_without_vt": (_with(2, file="partial.obj"), "partial.obj: line 9: a face corner without a texture index"),
        "filter": (_with(2, texture_filter="cubic"), "scene object 2: unknown \"texture_filter\" 'cubic' (nearest, bilinear)"),
        "wrap": (_with(2, texture_wrap="mirror"), "scene object 2: unknown \"texture_wrap\" 'mirror' (repeat, clamp)"),
        "not_a_string": (_with(1, texture=3), "scene object 1: \"texture\" must be a string"),
        "eight_bit": (_with(1, texture="tex.png"), "scene object 1: \"texture\": "),
        "truncated": (_with(1, texture="short.pfm"), "scene object 1: \"texture\": "),
        "missing": (_with(1, texture="nowhere.pfm"), "scene object 1: \"texture\": "),
        "on_a_sphere": (_with(0, texture="tex.pfm"), "scene object 0: \"texture\" does not apply to a sphere"),
    }
    for name, (text, message) in bad.items():
        p = tmp_path / (name + ".json")
        p.write_text(text)
        r = subprocess.run(base + ["--scene", str(p)], capture_output=True, text=True)
        assert r.returncode == 1 and "--scene" in r.stdout and message in r.stdout, (name, r.returncode, r.stdout[-600:])
        assert "Could not attach" not in r.stdout and "Tracebuffer" not in r.stdout, name      # refused before a device is attached
    for name, text in (("good", json.dumps({"objects": GOOD})), ("untextured_with_vt", _with(2, drop=("texture", "uvs", "texture_filter", "texture_wrap"))),
                       ("normals_and_uvs_from_file", _with(2, normals="file"))):
        p = tmp_path / (name + ".json")
        p.write_text(text)
        r = subprocess.run(base + ["--scene", str(p), "--compile-only"], capture_output=True, text=True)
        assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, (name, r.stdout[-500:])
