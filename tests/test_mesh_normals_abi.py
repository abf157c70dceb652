"""Vertex normals of meshes (pt_set_mesh_normals, pt_get_mesh_normals_info, pt_mesh_shade): the C-ABI without a GPU -- symbols, struct
layouts, that nothing pinned moved, the NULL-handle rules, the binding's argument checks and the vertex_normals helper.  (Everything
that needs a handle: tests/test_gpu_mesh_normals.py; the validation's messages: tests/test_mesh_normals.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import scene_mesh_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_mesh_normals", "pt_get_mesh_normals_info", "pt_mesh_shade"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert C.sizeof(P.MeshNormalsInfo) == 24 and [(n, getattr(P.MeshNormalsInfo, n).offset) for n, _ in P.MeshNormalsInfo._fields_] == \
        [("struct_size", 0), ("has_normals", 4), ("per_corner", 8), ("n_normals", 12), ("device_bytes", 16)]
    for name in ("set_mesh_normals", "mesh_normals_info", "mesh_shade"):
        assert callable(getattr(P.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 == P.ABI_VERSION
    assert C.sizeof(P.Mesh) == 32 and C.sizeof(P.MeshInfo) == 48 and C.sizeof(P.Config) == 56 and P.SCENE_EX_DTYPE.itemsize == 84
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+5\b", header)
    assert "typedef struct pt_mesh {              /* 32 bytes */" in header and "typedef struct pt_mesh_info {         /* 48 bytes */" in header


def test_kernel_argument_budget_and_mesh_row():
    """TraceParams grew by one pointer at its end and still fits the 4 KiB of kernel arguments; a mesh row still travels in its
    PolyEdges slot (the static_asserts of csrc/pt_trace.h, which the build compiles, say so: this reads them)."""
    src = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "pt_trace.h")).read()
    assert "static_assert(sizeof(TraceParams) <= 4096" in src and "static_assert(sizeof(MeshRow) == sizeof(PolyEdges)" in src
    tail = src[src.index("struct TraceParams {"):src.index("static_assert(sizeof(TraceParams) <= 4096")]
    assert tail.rstrip().endswith("const ptmesh::F4* mesh_normals;\n};".rstrip())


def test_null_handle_rules(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    n = np.float32([(0, 0, 1)])
    assert lib.pt_set_mesh_normals(None, 0, n.ctypes.data, 1, None) == -1
    assert lib.pt_last_error(None).decode() == "pt_set_mesh_normals: null handle"
    assert lib.pt_set_mesh_normals(None, 0, None, 0, None) == -1
    assert lib.pt_get_mesh_normals_info(None, 0, C.byref(P.MeshNormalsInfo(struct_size=24))) == -1
    o = np.zeros((1, 3), np.float32)
    out = np.zeros(3, np.float32)
    assert lib.pt_mesh_shade(None, o.ctypes.data, o.ctypes.data, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                             out.ctypes.data) == -1


def test_the_bindings_argument_checks(ptmi_lib):
    P = ptmi_lib
    v = np.float32([(0, 0, -2), (1, 0, -2), (0, 1, -2), (1, 1, -2.5)])
    t = np.uint32([(0, 1, 2), (1, 3, 2)])
    good = {"shape": "mesh", "material": "diffuse", "vertices": v, "triangles": t, "normals": np.float32([(0, 0, 1)] * 4)}
    table, meshes = P.scene_meshes([good])                      # the keys are known; the table and the meshes are as before
    assert table["shape"].tolist() == [4] and len(meshes) == 1
    flat = {"shape": "mesh", "material": "diffuse", "vertices": v, "triangles": t}
    got = P.mesh_normals([flat, {"shape": "sphere"}, dict(good, normal_indices=t), good])
    assert [(k, i is None) for k, _, i in got] == [(1, False), (2, True)]        # k counts mesh rows; the flat one has no entry
    with pytest.raises(ValueError, match="normal_indices without normals"):
        P.mesh_normals([dict(flat, normal_indices=t)])
    r = object.__new__(P.Renderer)                              # no handle: the checks below run before the library is called
    for normals, indices, match in [(np.zeros((4, 2), np.float32), None, "shape \\(N, 3\\)"), (np.zeros((0, 3), np.float32), None, "shape \\(N, 3\\)"),
                                    (np.zeros((4, 3)), t.ravel(), "shape \\(T, 3\\)"), (np.zeros((4, 3)), t.astype(np.float32), "shape \\(T, 3\\)"),
                                    (np.zeros((4, 3)), t.astype(np.int64) - 1, "shape \\(T, 3\\)"), (None, t, "indices without normals")]:
        with pytest.raises(ValueError, match=match):
            r.set_mesh_normals(0, normals, indices)
    for o, d in [(np.zeros((2, 2)), np.zeros((2, 2))), (np.zeros((2, 3)), np.zeros((3, 3)))]:
        with pytest.raises(ValueError, match="shape \\(n, 3\\)"):
            r.mesh_shade(o, d)


def test_vertex_normals(ptmi_lib):
    P = ptmi_lib
    # a planar grid: the plane's normal exactly
    v, t = MM.height_field(4, 1.0, (0.0, 0.5, -2.0), 0.0)
    n = P.vertex_normals(v, t)
    assert n.dtype == np.float32 and n.shape == (len(v), 3)
    assert np.array_equal(np.abs(n), np.tile(np.float32([0, 1, 0]), (len(v), 1)))
    assert len(set(np.sign(n[:, 1]).tolist())) == 1
    # a convex mesh: unit length, pointing away from the centroid
    v, t = MM.icosphere(2, 0.3, (0.1, 0.2, -1.0))
    n = P.vertex_normals(v, t).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-6)
    assert np.all(np.einsum("ij,ij->i", n, v - v.mean(axis=0)) > 0)
    # angle weights: on a sphere's mesh the vertex normal is close to radial
    assert np.max(np.abs(n - (v - np.array((0.1, 0.2, -1.0))) / 0.3)) < 0.02
    # a vertex no triangle uses gets zero; bad shapes are refused
    v2 = np.concatenate([v, [[9.0, 9.0, 9.0]]])
    assert np.all(P.vertex_normals(v2, t)[-1] == 0)
    with pytest.raises(ValueError):
        P.vertex_normals(v[:, :2], t)
    with pytest.raises(ValueError):
        P.vertex_normals(v, t + len(v))
