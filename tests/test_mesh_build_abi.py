"""Mesh trees built and refitted on the device (pt_set_mesh_build / pt_get_mesh_build_info / pt_mesh_tree): the C-ABI, the
validation order with a NULL handle, the binding's argument checks and the CLI's --mesh-builder, without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")


def test_entry_points_constants_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_mesh_build", "pt_get_mesh_build_info", "pt_mesh_tree"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert (P.MESH_BUILDER_HOST, P.MESH_BUILDER_DEVICE) == (0, 1) and (P.MESH_POSE_REBUILD, P.MESH_POSE_REFIT) == (0, 1)
    assert (P.MESH_LAST_NONE, P.MESH_LAST_HOST_BUILD, P.MESH_LAST_DEVICE_BUILD, P.MESH_LAST_REFIT) == (0, 1, 2, 3)
    assert P.MESH_BUILDERS == {"host": 0, "device": 1} and P.MESH_POSES == {"rebuild": 0, "refit": 1}
    O, I = P.MeshBuildOptions, P.MeshBuildInfo
    assert C.sizeof(O) == 12 and [(n, getattr(O, n).offset) for n, _ in O._fields_] == [("struct_size", 0), ("builder", 4), ("on_pose", 8)]
    assert C.sizeof(I) == 64
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("struct_size", 0), ("builder", 4), ("on_pose", 8), ("sort_on_device", 12), ("host_builds", 16), ("device_builds", 24),
        ("refits", 32), ("last_kind", 40), ("reserved", 44), ("last_ms", 48), ("device_bytes", 56)]
    D = P.MESH_NODE_DTYPE
    assert D.itemsize == 32 and [(n, D.fields[n][1]) for n in D.names] == [("lo", 0), ("hi", 12), ("skip", 24), ("leaf", 28)]
    for name in ("set_mesh_build", "mesh_build_info", "mesh_tree"):
        assert callable(getattr(P.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.Config) == 56 and C.sizeof(P.Stats) == 80 and C.sizeof(P.SceneObject) == 48
    assert C.sizeof(P.Mesh) == 32 and C.sizeof(P.MeshInfo) == 48 and C.sizeof(P.MeshNormalsInfo) == 24
    assert C.sizeof(P.MeshTexture) == 56 and C.sizeof(P.MeshTextureInfo) == 40
    assert P.SCENE_EX_DTYPE.itemsize == 84 and P.SCENE_DTYPE.itemsize == 48 and P.TRACE_DTYPE.itemsize == 20 and P.PATH_DTYPE.itemsize == 48


def test_the_header_states_the_same_layout():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+5\b", text)
    assert "enum { PT_MESH_BUILDER_HOST = 0, PT_MESH_BUILDER_DEVICE = 1 };" in text
    assert "enum { PT_MESH_POSE_REBUILD = 0, PT_MESH_POSE_REFIT = 1 };" in text
    for decl in ("int pt_set_mesh_build(pt_handle h, const pt_mesh_build_options* o);",
                 "int pt_get_mesh_build_info(pt_handle h, pt_mesh_build_info* out);",
                 "int pt_mesh_tree(pt_handle h, uint32_t mesh, pt_mesh_node* nodes, uint32_t node_capacity, uint32_t* orig, uint32_t orig_capacity);"):
        assert decl in text
    assert "TREE QUALITY IS BELOW SAH" in text and "DOES NOT\n * DEPEND ON THE TREE" in text


def _rejected(P, options):
    lib = P.load_library()
    rc = lib.pt_set_mesh_build(None, None if options is None else C.byref(options))
    assert rc == -1
    return lib.pt_last_error(None).decode()


def test_validation_order_with_a_null_handle(ptmi_lib):
    """With a NULL handle every check runs and the handle is refused last: each struct carries the fault under test and every
    later one."""
    P = ptmi_lib
    O = P.MeshBuildOptions
    assert _rejected(P, O(11, 7, 9)) == "pt_set_mesh_build: struct_size must be 12 (got 11)"
    assert _rejected(P, O(12, 7, 9)) == "pt_set_mesh_build: builder must be 0 (host) or 1 (device) (got 7)"
    assert _rejected(P, O(12, -1, 9)) == "pt_set_mesh_build: builder must be 0 (host) or 1 (device) (got -1)"
    assert _rejected(P, O(12, 1, 9)) == "pt_set_mesh_build: on_pose must be 0 (rebuild) or 1 (refit) (got 9)"
    assert _rejected(P, O(12, 0, 2)) == "pt_set_mesh_build: on_pose must be 0 (rebuild) or 1 (refit) (got 2)"
    for b in (0, 1):
        for p in (0, 1):
            assert _rejected(P, O(12, b, p)) == "pt_set_mesh_build: null handle"
    assert _rejected(P, None) == "pt_set_mesh_build: null handle"        # NULL options are the defaults: valid
    lib = P.load_library()
    info = P.MeshBuildInfo(struct_size=64)
    assert lib.pt_get_mesh_build_info(None, C.byref(info)) == -1
    assert lib.pt_mesh_tree(None, 0, None, 0, None, 0) == -1


class _NoDevice:
    """Renderer's methods on an object without a handle: the argument checks run before the library is reached."""
    handle = None

    def _check(self, rc):
        raise AssertionError("the library was reached")


def test_binding_argument_checks(ptmi_lib):
    P = ptmi_lib
    r = _NoDevice()
    r._lib = None
    with pytest.raises(ValueError, match="builder must be one of"):
        P.Renderer.set_mesh_build(r, builder="gpu")
    with pytest.raises(ValueError, match="on_pose must be one of"):
        P.Renderer.set_mesh_build(r, builder="device", on_pose="keep")
    with pytest.raises(ValueError, match="builder must be one of"):
        P.Renderer.set_mesh_build(r, builder=1)
    assert np.zeros(1, P.MESH_NODE_DTYPE)["lo"].shape == (1, 3)


def test_cli_mesh_builder_option(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--mesh-builder" in help_text
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    r = subprocess.run(base + ["--mesh-builder", "sah"], capture_output=True, text=True)
    assert r.returncode == 1 and "--mesh-builder must be one of host, device; got 'sah'" in r.stdout, r.stdout[-600:]
    assert "Could not attach" not in r.stdout                                  # refused before a device is attached
    for value in ("host", "device"):
        r = subprocess.run(base + ["--mesh-builder", value, "--compile-only"], capture_output=True, text=True)
        assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, r.stdout[-500:]
