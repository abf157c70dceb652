"""`ipu_trace --scene` with "texture" end to end on the GPU: an .obj with vt lines, "uvs": "file" and a .pfm texture, beside an inline
mesh with inline "uvs", gives the EXR that the Python binding's render of the same scene with set_mesh_texture gives, bit for bit;
the same file WITHOUT the keys renders untextured, although the .obj holds vt lines."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_normals_fixtures as NF
from tests import mesh_texture_fixtures as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
F32 = np.float32
W, H = 64, 48
SKY = (0.75, 1.5, 3.0)


def _read_exr(path):
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=np.float32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert L.pth_read_exr(str(path).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    return film


def test_cli_renders_a_texture_from_an_obj_and_inline_like_the_binding(ptmi_lib, tmp_path):
    P = ptmi_lib
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    spp = 8
    (fv, ft, _), (sv, st, tex), _ = F.meshes("bilinear_repeat")           # the ball: per-corner indices, what an OBJ's v/vt carries
    suv, si = tex["uvs"], tex["uv_indices"]
    fuv = F.planar_uvs(fv, -0.5, 2.5)                                    # the field: per-vertex uvs, inline
    image = F.image_5x3()
    F.write_pfm(tmp_path / "tex.pfm", image)
    obj = "".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in sv) + "".join("vt %r %r\n" % tuple(float(x) for x in q) for q in suv) + \
        "".join("f " + " ".join("%d/%d" % (a + 1, b + 1) for a, b in zip(t, i)) + "\n" for t, i in zip(st.tolist(), si.tolist()))
    (tmp_path / "ball.obj").write_text(obj)
    camera = {"position": [0.05, 0.02, 0.0], "look_at": [0.03, -0.04, -0.55], "up": [0.05, 1, 0]}

    def objects(textured):
        ball = {"shape": "mesh", "material": "diffuse", "colour": [0.9, 0.95, 0.9], "file": "ball.obj"}
        field = {"shape": "mesh", "material": "diffuse", "colour": [0.8, 0.7, 0.5], "vertices": fv.tolist(), "triangles": ft.tolist()}
        if textured:
            ball.update(texture="tex.pfm", uvs="file")
            field.update(texture="tex.pfm", uvs=fuv.astype(np.float64).tolist(), texture_filter="nearest", texture_wrap="clamp")
        return [ball, {"shape": "sphere", "material": "emissive", "emission": [6.0, 4.5, 3.0], "centre": [-0.1, 0.15, -0.5], "radius": 0.04}, field]

    def cli(textured, name):
        path = tmp_path / (name + ".json")
        path.write_text(json.dumps({"objects": objects(textured), "camera": camera}))
        r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in SKY), "-w", str(W), "-h", str(H),
                            "-s", str(spp), "--samples-per-step", str(spp), "--max-path-length", "7", "-o", str(tmp_path / (name + ".png")),
                            "--save-interval", "1", "--scene", str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        return _read_exr(tmp_path / (name + ".exr"))

    def binding(textured):
        ball = {"shape": "mesh", "material": "diffuse", "colour": (0.9, 0.95, 0.9), "vertices": sv, "triangles": st}
        field = {"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": fv, "triangles": ft}
        if textured:
            ball.update(texture=image, uvs=suv, uv_indices=si)
            field.update(texture=image, uvs=fuv, texture_filter="nearest", texture_wrap="clamp")
        scene = [ball, {"shape": "sphere", "material": "emissive", "colour": (6.0, 4.5, 3.0), "centre": (-0.1, 0.15, -0.5), "radius": 0.04}, field]
        r = P.Renderer(W, H, max_path_length=7, roulette_depth=3, iterations_per_batch=2)
        try:
            r.set_constant_env(SKY)
            r.init_render_settings(seed=1, samples_per_step=spp)
            r.set_scene(scene)
            r.set_camera(**camera)
            assert [r.mesh_texture_info(k)["has_texture"] for k in range(2)] == [int(textured)] * 2
            rec = P.worklist(W, H)
            r.setup(rec)
            r.path_trace()
            r.read_results(rec)
            r.film_accumulate()
            out = np.zeros((H, W, 3), F32)
            out[rec["v"], rec["u"]] = r.gather_hdr(W * H, P.HDR_FILM)[0]
            ids = r.feature_buffers()["object_id"]
        finally:
            r.close()
        assert all(np.count_nonzero(ids == k) > 10 for k in (0, 2))
        return out

    textured, plain = binding(True), binding(False)
    assert np.array_equal(cli(True, "textured"), textured) and len(np.unique(textured.reshape(-1, 3), axis=0)) > 500
    assert np.array_equal(cli(False, "plain"), plain)                  # vt lines in the file, no "texture" key: the ball keeps its one colour
    assert not np.array_equal(textured, plain)
