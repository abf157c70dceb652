"""Which tree the device builder builds (pt_set_mesh_device_tree / pt_get_mesh_device_tree_info): the C-ABI, the validation order
with a NULL handle, the binding's argument check and the CLI's --mesh-device-tree, without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")


def test_entry_points_constants_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_mesh_device_tree", "pt_get_mesh_device_tree_info"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert (P.MESH_DEVICE_TREE_LINEAR, P.MESH_DEVICE_TREE_SAH) == (0, 1)
    assert P.MESH_DEVICE_TREES == {"linear": 0, "sah": 1}
    I = P.MeshDeviceTreeInfo
    assert C.sizeof(I) == 40
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("struct_size", 0), ("kind", 4), ("sah_builds", 8), ("last_levels", 16), ("reserved", 20), ("last_ms", 24), ("device_bytes", 32)]
    for name in ("set_mesh_device_tree", "mesh_device_tree_info"):
        assert callable(getattr(P.Renderer, name))
    # additive: the ABI version and the build options' structs and constants do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.MeshBuildOptions) == 12 and C.sizeof(P.MeshBuildInfo) == 64
    assert P.MESH_BUILDERS == {"host": 0, "device": 1}


def test_the_header_states_the_same_layout():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+5\b", text)
    for line in ("enum { PT_MESH_DEVICE_TREE_LINEAR = 0, PT_MESH_DEVICE_TREE_SAH = 1 };",
                 "int pt_set_mesh_device_tree(pt_handle h, int32_t kind);",
                 "typedef struct pt_mesh_device_tree_info { uint32_t struct_size; int32_t kind; uint64_t sah_builds;",
                 "uint32_t last_levels, reserved; double last_ms; uint64_t device_bytes; } pt_mesh_device_tree_info;   /* 40 bytes */",
                 "int pt_get_mesh_device_tree_info(pt_handle h, pt_mesh_device_tree_info* out);"):
        assert line in text, line
    # the linear tree's paragraph stands as it was, and the new block states the memory per triangle
    assert "enum { PT_MESH_BUILDER_HOST = 0, PT_MESH_BUILDER_DEVICE = 1 };" in text and "TREE QUALITY IS BELOW SAH" in text
    assert "BYTES PER TRIANGLE" in text


def test_validation_order_with_a_null_handle(ptmi_lib):
    """The kind is checked first, the handle last, and both report through pt_last_error(NULL)."""
    P = ptmi_lib
    lib = P.load_library()
    for bad in (2, -1, 7):
        assert lib.pt_set_mesh_device_tree(None, bad) == -1
        assert lib.pt_last_error(None).decode() == "pt_set_mesh_device_tree: kind must be 0 (linear) or 1 (sah) (got %d)" % bad
    for kind in (0, 1):
        assert lib.pt_set_mesh_device_tree(None, kind) == -1
        assert lib.pt_last_error(None).decode() == "pt_set_mesh_device_tree: null handle"
    info = P.MeshDeviceTreeInfo(struct_size=40)
    assert lib.pt_get_mesh_device_tree_info(None, C.byref(info)) == -1


class _NoDevice:
    """Renderer's methods on an object without a handle: the argument checks run before the library is reached."""
    handle = None
    _lib = None

    def _check(self, rc):
        raise AssertionError("the library was reached")


@pytest.mark.parametrize("kind", ["SAH", "lbvh", "", 1, None, b"sah"])
def test_binding_argument_check(ptmi_lib, kind):
    with pytest.raises(ValueError, match="kind must be one of"):
        ptmi_lib.Renderer.set_mesh_device_tree(_NoDevice(), kind)


def test_cli_mesh_device_tree_option(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--mesh-device-tree" in help_text and "--mesh-builder" in help_text
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    r = subprocess.run(base + ["--mesh-device-tree", "lbvh"], capture_output=True, text=True)
    assert r.returncode == 1 and "--mesh-device-tree must be one of linear, sah; got 'lbvh'" in r.stdout, r.stdout[-600:]
    assert "Could not attach" not in r.stdout                                  # refused before a device is attached
    for value in ("linear", "sah"):
        for builder in ("host", "device"):
            r = subprocess.run(base + ["--mesh-builder", builder, "--mesh-device-tree", value, "--compile-only"], capture_output=True, text=True)
            assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, r.stdout[-500:]
