"""The report of the trace-kernel instance in force (pt_get_trace_variant / Renderer.trace_variant): the entry point, the layout
stated in Python and in the header, the constants against ipu_path_trace_amd/csrc/ptmi_trace_variant.h, and the validation order
with a NULL handle, without a GPU.  What a launch reports is checked on the device, tests/test_gpu_trace_instances.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enumerators(text, name):
    """The enumerators of `enum class <name> : int { ... }` in ptmi_trace_variant.h, in order, with their values."""
    body = re.search(r"enum class %s : int \{([^}]*)\}" % name, text).group(1)
    out, value = [], -1
    for item in body.split(","):
        m = re.fullmatch(r"\s*(\w+)\s*(?:=\s*(\d+))?\s*", item)
        value = int(m.group(2)) if m.group(2) else value + 1
        out.append((m.group(1), value))
    return out


def test_entry_point_constants_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    assert hasattr(lib, "pt_get_trace_variant") and "pt_get_trace_variant" in P.EXPORTS
    L, I = P.TraceVariantLaunch, P.TraceVariantInfo
    assert C.sizeof(L) == 24 and [(n, getattr(L, n).offset) for n, _ in L._fields_] == [
        ("camera", 0), ("bounce", 4), ("geometry", 8), ("index", 12), ("launches", 16)]
    assert C.sizeof(I) == 80 and [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("struct_size", 0), ("reserved", 4), ("trace", 8), ("paths", 32), ("features", 56)]
    assert callable(P.Renderer.trace_variant)
    # the constants are the selector's own (ptmi_trace_variant.h), by name and by value
    text = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "ptmi_trace_variant.h")).read()
    for enum, prefix, names in (("Camera", "TRACE_CAMERA_", P.TRACE_CAMERAS), ("Bounce", "TRACE_BOUNCE_", P.TRACE_BOUNCES),
                                ("Geometry", "TRACE_GEOMETRY_", P.TRACE_GEOMETRIES)):
        found = _enumerators(text, enum)
        assert [n for n, _ in found] == list(names) and [v for _, v in found] == list(range(len(names)))
        assert [getattr(P, prefix + n) for n in names] == list(range(len(names)))
    assert re.search(r"kCameras = 3, kBounces = 4, kGeometries = 5;", text)
    assert re.search(r"kTraceInstances == 57 && kPathsInstances == 19 && kFeatureInstances == 5", text)
    assert (P.TRACE_INSTANCES, P.TRACE_PATHS_INSTANCES, P.TRACE_FEATURE_INSTANCES) == (57, 19, 5)
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(P.Config) == 56 and C.sizeof(P.Stats) == 80 and C.sizeof(P.SceneObject) == 48
    assert C.sizeof(P.Mesh) == 32 and C.sizeof(P.MeshInfo) == 48 and C.sizeof(P.MeshBuildInfo) == 64 and C.sizeof(P.MeshUpdateInfo) == 64
    assert P.SCENE_EX_DTYPE.itemsize == 84 and P.SCENE_DTYPE.itemsize == 48 and P.TRACE_DTYPE.itemsize == 20 and P.PATH_DTYPE.itemsize == 48


def test_the_header_states_the_same_layout_and_values():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+5\b", text)
    variant = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "ptmi_trace_variant.h")).read()
    for enum, prefix in (("Camera", "PT_TRACE_CAMERA_"), ("Bounce", "PT_TRACE_BOUNCE_"), ("Geometry", "PT_TRACE_GEOMETRY_")):
        assert "enum { %s };" % ", ".join("%s%s = %d" % (prefix, n, v) for n, v in _enumerators(variant, enum)) in text
    assert re.search(r"typedef struct pt_trace_variant_launch \{ /\* 24 bytes \*/\s*int32_t camera, bounce, geometry;[^\n]*\n"
                     r"\s*int32_t index;[^\n]*\n\s*uint64_t launches;[^\n]*\n\} pt_trace_variant_launch;", text)
    assert re.search(r"typedef struct pt_trace_variant_info \{ /\* 80 bytes \*/\s*uint32_t struct_size;[^\n]*\n\s*uint32_t reserved;\n"
                     r"\s*pt_trace_variant_launch trace, paths, features;\n\} pt_trace_variant_info;", text)
    assert "int pt_get_trace_variant(pt_handle h, pt_trace_variant_info* out);" in text
    assert "nothing that is launched changes" in text and "are -1 and its count is 0" in text


def _rejected(P, info):
    lib = P.load_library()
    assert lib.pt_get_trace_variant(None, None if info is None else C.byref(info)) == -1
    return lib.pt_last_error(None).decode()


def test_validation_order_with_a_null_handle(ptmi_lib):
    """With a NULL handle every check runs and the handle is refused last; a refused call writes nothing."""
    P = ptmi_lib
    assert _rejected(P, None) == "pt_get_trace_variant: null output"
    for size in (0, 8, 56, 79):                                     # too small: 56 is the struct without `features`
        info = P.TraceVariantInfo(struct_size=size, reserved=7)
        info.trace.index = 41
        assert _rejected(P, info) == "pt_get_trace_variant: struct_size must be 80 (got %d)" % size
        assert (info.struct_size, info.reserved, info.trace.index) == (size, 7, 41)
    assert _rejected(P, P.TraceVariantInfo(struct_size=81)) == "pt_get_trace_variant: struct_size must be 80 (got 81)"
    info = P.TraceVariantInfo(struct_size=80, reserved=7)
    info.paths.launches = 3
    assert _rejected(P, info) == "pt_get_trace_variant: null handle"
    assert (info.reserved, info.paths.launches) == (7, 3)


class _NoDevice:
    """Renderer.trace_variant on an object whose library call is a stand-in: the binding's own work, without a handle."""
    handle = None

    def __init__(self, P, fill):
        self._lib = self
        self._P, self._fill, self.seen = P, fill, None

    def pt_get_trace_variant(self, handle, ref):
        info = ref._obj
        self.seen = info.struct_size
        self._fill(info)
        return 0

    def _check(self, rc):
        assert rc == 0


def test_binding_returns_the_three_records(ptmi_lib):
    P = ptmi_lib

    def fill(info):
        info.trace = P.TraceVariantLaunch(2, 3, 4, 56, 9)
        info.paths = P.TraceVariantLaunch(1, 0, 1, 3, 2)
        info.features = P.TraceVariantLaunch(-1, -1, -1, -1, 0)
    r = _NoDevice(P, fill)
    out = P.Renderer.trace_variant(r)
    assert r.seen == 80
    assert out == {"trace": {"camera": 2, "bounce": 3, "geometry": 4, "index": 56, "launches": 9},
                   "paths": {"camera": 1, "bounce": 0, "geometry": 1, "index": 3, "launches": 2},
                   "features": {"camera": -1, "bounce": -1, "geometry": -1, "index": -1, "launches": 0}}
