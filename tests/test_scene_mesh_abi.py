"""Triangle meshes in runtime scenes (pt_set_scene_meshes, pt_get_mesh_info, pt_mesh_intersect): the C-ABI, every validation message
in the stated order with a NULL handle, and the binding's own argument checks, without a GPU.  (pt_get_scene_ex / pt_get_scene with a
mesh row need a handle: tests/test_gpu_scene_meshes.py.)"""
import ctypes as C

import numpy as np
import pytest

VERTS = np.float32([(0, 0, -2), (1, 0, -2), (0, 1, -2), (1, 1, -2.5)])
TRIS = np.uint32([(0, 1, 2), (1, 3, 2)])


def test_entry_points_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_scene_meshes", "pt_get_mesh_info", "pt_mesh_intersect"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert P.SHAPE_MESH == 4 and P.MAX_MESH_TRIANGLES == 1 << 22 and (P.MESH_INTERSECT_BVH, P.MESH_INTERSECT_BRUTE) == (0, 1)
    assert C.sizeof(P.Mesh) == 32 and [(n, getattr(P.Mesh, n).offset) for n, _ in P.Mesh._fields_] == \
        [("struct_size", 0), ("n_vertices", 4), ("n_triangles", 8), ("vertices", 16), ("indices", 24)]
    assert C.sizeof(P.MeshInfo) == 48 and [(n, getattr(P.MeshInfo, n).offset) for n, _ in P.MeshInfo._fields_] == \
        [("struct_size", 0), ("object_index", 4), ("n_triangles", 8), ("n_nodes", 12), ("max_leaf", 16), ("depth", 20),
         ("device_bytes", 24), ("build_ms", 32), ("pad", 40)]
    for name in ("set_scene_meshes", "mesh_info", "mesh_intersect"):
        assert callable(getattr(P.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.Config) == 56 and C.sizeof(P.Stats) == 80 and P.SCENE_EX_DTYPE.itemsize == 84


def _table(P):
    return P.scene_meshes([
        {"shape": "sphere", "material": "diffuse", "centre": (0, 0, -3), "radius": 1, "colour": (0.5, 0.6, 0.7)},
        {"shape": "mesh", "material": "refractive", "colour": (0.9, 0.9, 0.9), "vertices": VERTS, "triangles": TRIS},
        {"shape": "triangle", "material": "emissive", "vertices": ((0, 0, -2), (1, 0, -2), (0, 1, -2)), "emission": (4, 5, 6)},
        {"shape": "mesh", "material": "emissive", "emission": (1, 2, 3), "vertices": VERTS, "triangles": TRIS[:1]}])[0]


class _Call:
    """One pt_set_scene_meshes(NULL, ...) over a table and meshes whose fields a test edits before the call."""

    def __init__(self, P):
        self.P, self.lib = P, P.load_library()
        self.table = _table(P)
        self.v = [VERTS.copy(), VERTS.copy()]
        self.t = [TRIS.copy(), TRIS[:1].copy()]
        self.size = [32, 32]
        self.nv = [4, 4]
        self.nt = [2, 1]
        self.null_v, self.null_t = [False, False], [False, False]
        self.n_meshes = 2
        self.no_meshes = False

    def message(self, n=None, stride=84, table=True):
        P = self.P
        arr = (P.Mesh * 2)()
        for k in range(2):
            arr[k] = P.Mesh(self.size[k], self.nv[k], self.nt[k], None if self.null_v[k] else self.v[k].ctypes.data,
                            None if self.null_t[k] else self.t[k].ctypes.data)
        rc = self.lib.pt_set_scene_meshes(None, self.table.ctypes.data if table else None, len(self.table) if n is None else n, stride,
                                          None if self.no_meshes else arr, self.n_meshes)
        assert rc == -1
        return self.lib.pt_last_error(None).decode()


def test_every_validation_message_in_the_stated_order(ptmi_lib):
    """With a NULL handle every check runs and the handle is refused last.  The call below collects faults from the LAST check
    to the first: each message shows that the earlier check wins over every later fault still in place."""
    P = ptmi_lib
    c = _Call(P)
    assert c.message() == "pt_set_scene_meshes: null handle"                     # 13: a valid call reaches the handle
    c.v[1][:] = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3)]                      # 12 collinear, in the second mesh (row 3)
    assert c.message() == "scene object 3, mesh 1, triangle 0: vertices are collinear"
    c.v[0][1] = (1e30, 0, 0)
    c.v[0][2] = (0, 1e30, 0)                                                     # 12 the cross product overflows: mesh 0 comes first
    assert c.message() == "scene object 1, mesh 0, triangle 0: vertex differences and their cross product must be finite"
    c.v[0][3] = (1, np.float32("nan"), 0)                                        # 11 before 12 on triangle 1; triangle 0 still fails 12 first
    assert c.message() == "scene object 1, mesh 0, triangle 0: vertex differences and their cross product must be finite"
    c.v[0][1], c.v[0][2] = (1, 0, -2), (0, 1, -2)
    assert c.message() == "scene object 1, mesh 0, triangle 1: vertices[3] must be finite (got nan)"
    c.t[0][1, 2] = 4                                                             # 10 before 11 on the same triangle
    assert c.message() == "scene object 1, mesh 0, triangle 1: indices[2] must be < n_vertices = 4 (got 4)"
    c.nv[1] = 0                                                                  # (a vertex count of 0: every index is out of range)
    c.t[0][1, 2] = 2
    c.v[0][3] = (1, 1, -2.5)
    assert c.message() == "scene object 3, mesh 1, triangle 0: indices[0] must be < n_vertices = 0 (got 0)"
    c.nt[0] = (1 << 22) + 1                                                      # 9: the total, before any triangle is read
    assert c.message() == "scene: 4194306 mesh triangles in all, 4194304 at most"
    c.nt[1] = 0                                                                  # 8 before 9
    assert c.message() == "mesh 1: n_triangles must be > 0"
    c.null_t[1] = True                                                           # 7 before 8
    assert c.message() == "mesh 1: null indices"
    c.null_v[1] = True
    assert c.message() == "mesh 1: null vertices"
    c.size[1] = 24                                                               # 6 before 7
    assert c.message() == "mesh 1: struct_size must be 32 (got 24)"
    c.null_v[0] = True                                                           # per mesh: mesh 0's 7 before mesh 1's 6
    assert c.message() == "mesh 0: null vertices"
    c.n_meshes = 1                                                               # 5 before 6
    assert c.message() == "scene: 2 object(s) of shape 4 (mesh) but n_meshes = 1"
    c.n_meshes, c.no_meshes = 2, True
    assert c.message() == "scene: null mesh table"
    c.table[2]["vertex"] = ((0, 0, 0), (1, 1, 1), (2, 2, 2))                      # 4, pt_set_scene_ex's rows: a polygon ...
    assert c.message() == "scene object 2: vertices are collinear"
    c.table[1]["colour"] = (1, -0.5, 1)                                          # ... and a mesh row's colour and material
    assert c.message() == "scene object 1: colour components must be >= 0 (got -0.5)"
    c.table[1]["colour"] = (1, np.float32("inf"), 1)
    assert c.message() == "scene object 1: colour must be finite (got inf)"
    c.table[1]["material"] = 7
    assert c.message().startswith("scene object 1: material must be 0 (diffuse), 1 (specular), 2 (refractive) or 3 (emissive) (got 7)")
    c.table[0]["shape"] = 5
    assert c.message() == "scene object 0: shape must be 0 (sphere), 1 (disc), 2 (triangle), 3 (parallelogram) or 4 (mesh) (got 5)"
    assert c.message(table=False) == "scene: null object table"                  # 3
    assert c.message(n=33, table=False) == "scene: object count must be 1..32 (got 33)"   # 2 before 3
    assert c.message(n=0) == "scene: object count must be 1..32 (got 0)"
    assert c.message(n=33, stride=48, table=False) == "scene: stride must be 84 (sizeof(pt_scene_object_ex)) (got 48)"   # 1 before 2


def test_a_mesh_row_ignores_its_geometric_fields(ptmi_lib):
    P = ptmi_lib
    c = _Call(P)
    nan, inf = np.float32("nan"), np.float32("inf")
    c.table[1]["centre"], c.table[1]["radius"], c.table[1]["normal"] = (nan, inf, 0), -inf, (nan, nan, nan)
    c.table[1]["vertex"] = nan
    assert c.message() == "pt_set_scene_meshes: null handle"


def test_null_handle_rules_and_the_other_setters(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    # (NULL, 0, stride, NULL, 0) is a valid call -- the built-in scene -- and reaches the handle
    assert lib.pt_set_scene_meshes(None, None, 0, 84, None, 0) == -1 and lib.pt_last_error(None).decode() == "pt_set_scene_meshes: null handle"
    # a table without a mesh row is checked as pt_set_scene_ex checks it, then refused for the handle
    plain = P.scene_array_ex([{"shape": "sphere", "material": "diffuse", "centre": (0, 0, -3), "radius": 1}])
    assert lib.pt_set_scene_meshes(None, plain.ctypes.data, 1, 84, None, 0) == -1
    assert lib.pt_last_error(None).decode() == "pt_set_scene_meshes: null handle"
    # pt_set_scene_ex and pt_set_scene still refuse shape 4
    t = _table(P)
    assert lib.pt_set_scene_ex(None, t.ctypes.data, len(t), 84) == -1
    assert lib.pt_last_error(None).decode() == "scene object 1: shape must be 0 (sphere), 1 (disc), 2 (triangle) or 3 (parallelogram) (got 4)"
    assert lib.pt_get_mesh_info(None, 0, C.byref(P.MeshInfo(struct_size=48))) == -1
    o = np.zeros((1, 3), np.float32)
    out = np.zeros(1, np.float32)
    assert lib.pt_mesh_intersect(None, o.ctypes.data, o.ctypes.data, 1, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -1


def test_scene_meshes_and_the_bindings_argument_checks(ptmi_lib):
    P = ptmi_lib
    table, meshes = P.scene_meshes([
        {"shape": "mesh", "material": "diffuse", "colour": (0.1, 0.2, 0.3), "vertices": VERTS.tolist(), "triangles": TRIS.tolist()},
        {"shape": "disc", "material": 1, "centre": (0, -1, -3), "radius": 2, "normal": (0, 1, 0)},
        {"shape": 4, "material": "emissive", "emission": (1, 2, 3), "vertices": VERTS, "triangles": TRIS[:1]}])
    assert table.dtype == P.SCENE_EX_DTYPE and table["shape"].tolist() == [4, 1, 4] and table["material"].tolist() == [0, 1, 3]
    assert np.array_equal(table["colour"][0], np.float32((0.1, 0.2, 0.3))) and np.array_equal(table["colour"][2], np.float32((1, 2, 3)))
    assert np.all(table["centre"][[0, 2]] == 0) and np.all(table["radius"][[0, 2]] == 0) and np.all(table["vertex"] == 0)
    assert len(meshes) == 2 and meshes[0][0].dtype == np.float32 and meshes[0][1].dtype == np.uint32
    assert meshes[0][0].shape == (4, 3) and meshes[0][1].shape == (2, 3) and meshes[1][1].shape == (1, 3)
    assert P.has_mesh([{"shape": "mesh"}]) and P.has_mesh([{"shape": 4}]) and not P.has_mesh([{"shape": "triangle"}]) and not P.has_mesh(table)
    good = {"shape": "mesh", "material": "diffuse", "vertices": VERTS, "triangles": TRIS}
    for key, value, match in [("vertices", VERTS[:, :2], "shape \\(V, 3\\)"), ("vertices", VERTS[:0], "shape \\(V, 3\\)"),
                              ("triangles", TRIS.ravel(), "shape \\(T, 3\\)"), ("triangles", TRIS[:0], "shape \\(T, 3\\)"),
                              ("triangles", TRIS.astype(np.float32), "unsigned 32-bit"), ("triangles", TRIS.astype(np.int64) - 1, "unsigned 32-bit"),
                              ("centre", (0, 0, 0), "unknown key"), ("radius", 1.0, "unknown key")]:
        with pytest.raises(ValueError, match=match):
            P.scene_meshes([dict(good, **{key: value})])
