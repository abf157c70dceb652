"""`ipu_trace --scene` with meshes end to end on the GPU: an inline mesh and an .obj file (with "scale" and "translate") give the EXR
that the Python binding's render of the same scene gives, bit for bit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
F32 = np.float32
W, H = 64, 48
SKY = (0.75, 1.5, 3.0)


def _read_exr(path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=np.float32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert L.pth_read_exr(str(path).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    return film


def _pyramid():
    """A square pyramid of 6 triangles (the base as a quad in the .obj), a fifth of a unit across."""
    v = [[-0.1, -0.1, -0.1], [0.1, -0.1, -0.1], [0.1, -0.1, 0.1], [-0.1, -0.1, 0.1], [0.0, 0.12, 0.0]]
    faces = [[0, 1, 2, 3], [0, 4, 1], [1, 4, 2], [2, 4, 3], [3, 4, 0]]
    return v, faces


def test_cli_renders_inline_and_obj_meshes_like_the_binding(ptmi_lib, tmp_path):
    P = ptmi_lib
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    spp = 8
    v, faces = _pyramid()
    (tmp_path / "models").mkdir()
    obj = "# pyramid\r\n" + "".join("v %r %r %r\r\n" % tuple(p) for p in v) + "vn 0 1 0\n" + \
        "".join("f " + " ".join("%d//1" % (i + 1) if k % 2 else "%d" % (i - len(v)) for i in f) + "\n" for k, f in enumerate(faces))
    (tmp_path / "models" / "pyramid.obj").write_text(obj)
    tris = [[f[0], f[k], f[k + 1]] for f in faces for k in range(1, len(f) - 1)]                 # the reader's fan
    scale, translate = [1.0, 1.5, 1.0], [0.08, -0.02, -0.6]
    floor_v = [[-0.5, -0.2, -1.0], [0.5, -0.2, -1.0], [0.5, -0.22, -0.2], [-0.5, -0.22, -0.2]]
    objects = [
        {"shape": "mesh", "material": "refractive", "colour": [0.9, 0.95, 0.9], "file": "models/pyramid.obj", "scale": scale, "translate": translate},
        {"shape": "sphere", "material": "emissive", "emission": [6.0, 4.5, 3.0], "centre": [-0.1, 0.15, -0.5], "radius": 0.04},
        {"shape": "mesh", "material": "diffuse", "colour": [0.8, 0.7, 0.5], "vertices": floor_v, "triangles": [[0, 1, 2], [0, 2, 3]]},
        {"shape": "mesh", "material": "specular", "vertices": v, "triangles": tris, "scale": 0.5, "translate": [-0.12, -0.1, -0.55]}]
    camera = {"position": [0.05, 0.02, 0.15], "look_at": [0.0, -0.02, -0.3], "up": [0.05, 1, 0]}
    path = tmp_path / "meshes.json"
    path.write_text(json.dumps({"objects": objects, "camera": camera}))
    base = [exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in SKY), "-w", str(W), "-h", str(H),
            "-s", str(spp), "--samples-per-step", str(spp), "--max-path-length", "7", "-o", str(tmp_path / "out.png"),
            "--save-interval", "1"]
    r = subprocess.run(base + ["--scene", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    exr = _read_exr(tmp_path / "out.exr")

    def placed(points, s, t):      # v * scale, then + translate, one rounded binary32 operation each: what the CLI documents
        s = np.broadcast_to(F32(s), (3,))
        return F32(F32(F32(points) * s) + F32(t))
    scene = [
        {"shape": "mesh", "material": "refractive", "colour": objects[0]["colour"], "vertices": placed(v, scale, translate), "triangles": np.uint32(tris)},
        {"shape": "sphere", "material": "emissive", "colour": objects[1]["emission"], "centre": objects[1]["centre"], "radius": 0.04},
        {"shape": "mesh", "material": "diffuse", "colour": objects[2]["colour"], "vertices": F32(floor_v), "triangles": np.uint32([[0, 1, 2], [0, 2, 3]])},
        {"shape": "mesh", "material": "specular", "colour": (1.0, 1.0, 1.0), "vertices": placed(v, 0.5, [-0.12, -0.1, -0.55]), "triangles": np.uint32(tris)}]
    lib_r = P.Renderer(W, H, max_path_length=7, roulette_depth=3, iterations_per_batch=2)
    try:
        lib_r.set_constant_env(SKY)
        lib_r.init_render_settings(seed=1, samples_per_step=spp)
        lib_r.set_scene(scene)
        lib_r.set_camera(**camera)
        assert [lib_r.mesh_info(k)["n_triangles"] for k in range(3)] == [6, 2, 6]
        rec = P.worklist(W, H)
        lib_r.setup(rec)
        lib_r.path_trace()
        lib_r.read_results(rec)
        lib_r.film_accumulate()
        image = np.zeros((H, W, 3), F32)
        image[rec["v"], rec["u"]] = lib_r.gather_hdr(W * H, P.HDR_FILM)[0]
        ids = lib_r.feature_buffers()["object_id"]
    finally:
        lib_r.close()
    assert np.array_equal(exr, image) and len(np.unique(image.reshape(-1, 3), axis=0)) > 500
    assert all(np.count_nonzero(ids == k) > 10 for k in (0, 2, 3))                      # the three meshes are in view
