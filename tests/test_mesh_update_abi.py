"""Animated meshes (pt_update_mesh_vertices / pt_get_mesh_update_info): the C-ABI, the validation order up to the NULL handle and
the binding's argument checks, without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_constants_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_update_mesh_vertices", "pt_get_mesh_update_info"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert (P.MESH_UPDATE_REFIT, P.MESH_UPDATE_REBUILD) == (0, 1) and (P.MESH_UPDATE_HOST_MEMORY, P.MESH_UPDATE_DEVICE_MEMORY) == (0, 1)
    assert P.MESH_UPDATE_MODES == {"refit": 0, "rebuild": 1}
    U, I = P.MeshUpdate, P.MeshUpdateInfo
    assert C.sizeof(U) == 40
    assert [(n, getattr(U, n).offset) for n, _ in U._fields_] == [("struct_size", 0), ("mode", 4), ("memory", 8), ("n_vertices", 12),
                                                                  ("vertices", 16), ("n_normals", 24), ("normals", 32)]
    assert C.sizeof(I) == 64
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("struct_size", 0), ("last_kind", 4), ("updates", 8), ("refits", 16), ("rebuilds", 24), ("fallbacks", 32),
        ("last_frames_ms", 40), ("last_tree_ms", 48), ("device_bytes", 56)]
    for name in ("update_mesh_vertices", "mesh_update_info"):
        assert callable(getattr(P.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.Config) == 56 and C.sizeof(P.Stats) == 80 and C.sizeof(P.SceneObject) == 48
    assert C.sizeof(P.Mesh) == 32 and C.sizeof(P.MeshInfo) == 48 and C.sizeof(P.MeshNormalsInfo) == 24
    assert C.sizeof(P.MeshBuildOptions) == 12 and C.sizeof(P.MeshBuildInfo) == 64
    assert C.sizeof(P.MeshTexture) == 56 and C.sizeof(P.MeshTextureInfo) == 40


def test_the_header_states_the_same_layout():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+5\b", text)
    assert "enum { PT_MESH_UPDATE_REFIT = 0, PT_MESH_UPDATE_REBUILD = 1 };" in text
    assert "enum { PT_MESH_UPDATE_HOST_MEMORY = 0, PT_MESH_UPDATE_DEVICE_MEMORY = 1 };" in text
    for decl in ("int pt_update_mesh_vertices(pt_handle h, uint32_t mesh, const pt_mesh_update* u);",
                 "int pt_get_mesh_update_info(pt_handle h, pt_mesh_update_info* out);"):
        assert decl in text
    body = text[text.index("typedef struct pt_mesh_update {"):text.index("} pt_mesh_update;")]
    order = [body.index(f) for f in ("struct_size;", "mode;", "memory;", "n_vertices;", "* vertices;", "n_normals;", "* normals;")]
    assert order == sorted(order)
    assert "KEEPS THE ATTACHED NORMALS AS THEY ARE" in text and "TOPOLOGY DOES NOT CHANGE" in text


def _rejected(P, update):
    lib = P.load_library()
    rc = lib.pt_update_mesh_vertices(None, 0, None if update is None else C.byref(update))
    assert rc == -1
    return lib.pt_last_error(None).decode()


def test_validation_order_with_a_null_handle(ptmi_lib):
    """With a NULL handle every check that needs no scene runs and the handle is refused last: each struct carries the fault under
    test and every later one."""
    P = ptmi_lib
    v = np.zeros((3, 3), np.float32)
    vp = v.ctypes.data

    def U(size=40, mode=0, memory=0, nv=3, vertices=vp, nn=0, normals=None):
        return P.MeshUpdate(size, mode, memory, nv, vertices, nn, normals)
    assert _rejected(P, None) == "pt_update_mesh_vertices: null update"
    assert _rejected(P, U(size=39, mode=7, memory=9, vertices=None, nn=4)) == "pt_update_mesh_vertices: struct_size must be 40 (got 39)"
    assert _rejected(P, U(mode=7, memory=9, vertices=None, nn=4)) == "pt_update_mesh_vertices: mode must be 0 (refit) or 1 (rebuild) (got 7)"
    assert _rejected(P, U(mode=-1, memory=9, vertices=None, nn=4)) == "pt_update_mesh_vertices: mode must be 0 (refit) or 1 (rebuild) (got -1)"
    assert _rejected(P, U(mode=1, memory=9, vertices=None, nn=4)) == "pt_update_mesh_vertices: memory must be 0 (host) or 1 (device) (got 9)"
    assert _rejected(P, U(mode=1, memory=1, vertices=None, nn=4)) == "pt_update_mesh_vertices: null vertices"
    assert _rejected(P, U(mode=1, memory=1, nn=4)) == "pt_update_mesh_vertices: null normals with n_normals = 4"
    assert _rejected(P, U(normals=vp)) == "pt_update_mesh_vertices: normals with n_normals = 0"
    for mode in (0, 1):
        for memory in (0, 1):
            assert _rejected(P, U(mode=mode, memory=memory)) == "pt_update_mesh_vertices: null handle"
            assert _rejected(P, U(mode=mode, memory=memory, nn=3, normals=vp)) == "pt_update_mesh_vertices: null handle"
    info = P.MeshUpdateInfo(struct_size=64)
    assert P.load_library().pt_get_mesh_update_info(None, C.byref(info)) == -1


class _NoDevice:
    """Renderer's methods on an object without a handle: the argument checks run before the library is reached."""
    handle = None
    _device = 0

    def _check(self, rc):
        raise AssertionError("the library was reached")


def test_binding_argument_checks(ptmi_lib):
    P = ptmi_lib
    r = _NoDevice()
    r._lib = None
    r._update_array = lambda what, a: P.Renderer._update_array(r, what, a)
    good = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="mode must be one of"):
        P.Renderer.update_mesh_vertices(r, 0, good, mode="fit")
    with pytest.raises(ValueError, match="vertices must be an array of shape"):
        P.Renderer.update_mesh_vertices(r, 0, np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="vertices must be an array of shape"):
        P.Renderer.update_mesh_vertices(r, 0, np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="normals must be an array of shape"):
        P.Renderer.update_mesh_vertices(r, 0, good, normals=np.zeros(3, np.float32))
    import torch
    with pytest.raises(ValueError, match="must be float32"):
        P.Renderer.update_mesh_vertices(r, 0, torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="must lie on the renderer's device"):
        P.Renderer.update_mesh_vertices(r, 0, torch.zeros((4, 3), dtype=torch.float32))      # a CPU tensor
