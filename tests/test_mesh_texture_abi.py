"""Textures of meshes (pt_set_mesh_texture, pt_get_mesh_texture_info, pt_mesh_texel): the C-ABI without a GPU -- symbols, struct
layouts, that nothing pinned moved, the NULL-handle rules, the binding's argument checks and the budget of the TEX kernels' two
arguments.  (Everything that needs a handle: tests/test_gpu_mesh_texture.py; the validation's messages: tests/test_mesh_texture.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_and_layout(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    for sym in ("pt_set_mesh_texture", "pt_get_mesh_texture_info", "pt_mesh_texel"):
        assert hasattr(lib, sym) and sym in P.EXPORTS
    assert C.sizeof(P.MeshTexture) == 56 and [(n, getattr(P.MeshTexture, n).offset) for n, _ in P.MeshTexture._fields_] == \
        [("struct_size", 0), ("width", 4), ("height", 8), ("filter", 12), ("wrap", 16), ("bgr", 24), ("uvs", 32), ("n_uvs", 40), ("uv_indices", 48)]
    assert C.sizeof(P.MeshTextureInfo) == 40 and [(n, getattr(P.MeshTextureInfo, n).offset) for n, _ in P.MeshTextureInfo._fields_] == \
        [("struct_size", 0), ("has_texture", 4), ("per_corner", 8), ("width", 12), ("height", 16), ("filter", 20), ("wrap", 24), ("n_uvs", 28),
         ("device_bytes", 32)]
    for name in ("set_mesh_texture", "mesh_texture_info", "mesh_texel"):
        assert callable(getattr(P.Renderer, name))
    assert (P.TEX_FILTER_NEAREST, P.TEX_FILTER_BILINEAR, P.TEX_WRAP_REPEAT, P.TEX_WRAP_CLAMP, P.MESH_TEXTURE_MAX_SIZE) == (0, 1, 0, 1, 8192)
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 == P.ABI_VERSION
    assert C.sizeof(P.Mesh) == 32 and C.sizeof(P.MeshInfo) == 48 and C.sizeof(P.MeshNormalsInfo) == 24 and C.sizeof(P.Config) == 56
    assert P.SCENE_EX_DTYPE.itemsize == 84
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+5\b", header)
    assert "typedef struct pt_mesh {              /* 32 bytes */" in header and "typedef struct pt_mesh_info {         /* 48 bytes */" in header
    assert "typedef struct pt_mesh_normals_info {   /* 24 bytes */" in header
    assert re.search(r"#define\s+PT_MESH_TEXTURE_MAX_SIZE\s+8192\b", header)
    assert "enum { PT_TEX_FILTER_NEAREST = 0, PT_TEX_FILTER_BILINEAR = 1 };" in header
    assert "enum { PT_TEX_WRAP_REPEAT = 0, PT_TEX_WRAP_CLAMP = 1 };" in header
    # the limits the contract states
    section = header[header.index("Texture coordinates and an image texture for a mesh"):header.index("int pt_mesh_texel(")]
    for phrase in ("LINEAR FLOAT IMAGES ONLY", "ONE texture per mesh", "NO mip maps", "NOT in the emitter guide"):
        assert phrase in section


def test_kernel_argument_budget():
    """TraceParams did not change -- its last member is still the normals' pointer -- and the TEX kernels' two arguments together fit
    the 4 KiB of kernel arguments (the static_asserts of csrc/pt_trace.h, which the build compiles, say so: this reads them)."""
    src = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "pt_trace.h")).read()
    assert "static_assert(sizeof(TraceParams) <= 4096" in src
    assert "static_assert(sizeof(TraceParams) + sizeof(TexParams) <= 4096" in src
    tail = src[src.index("struct TraceParams {"):src.index("static_assert(sizeof(TraceParams) <= 4096")]
    assert tail.rstrip().endswith("const ptmesh::F4* mesh_normals;\n};".rstrip())
    assert "uint32_t textured;" in src[src.index("struct MeshRow {"):src.index("static_assert(sizeof(MeshRow) == sizeof(PolyEdges)")]
    # every TEX kernel takes the second argument, and no other kernel does: the kernels with it are the three _tex templates, which
    # fix the geometry to TEX, and pt_mesh_texel's; the templates without it refuse TEX (static_asserts the build compiles: this reads them)
    feat = open(os.path.join(ROOT, "ipu_path_trace_amd", "csrc", "pt_features.h")).read()
    kernels = re.findall(r"__global__[^;{]*?void (\w+)\(const TraceParams P(, const TexParams X)?", src + feat)
    assert len(kernels) >= 10
    tex = sorted(k for k, second in kernels if second)
    assert tex == ["features_kernel_tex", "mesh_texel_kernel", "trace_kernel_tex", "trace_paths_tex_kernel"], tex
    assert not [k for k, second in kernels if not second and "tex" in k]
    for kernel, text in (("trace_kernel", src), ("trace_paths_kernel", src), ("features_kernel", feat)):
        body = text[text.index("void %s(const TraceParams P" % kernel):]
        assert body[:body.index("\n}")].count("static_assert(GEOM != GEOM_TEX") == 1, kernel
    for kernel, text in (("trace_kernel_tex", src), ("trace_paths_tex_kernel", src), ("features_kernel_tex", feat)):
        body = text[text.index("void %s(const TraceParams P, const TexParams X" % kernel):]
        assert re.search(r"using F = VariantFlags<\w+, GEOM_TEX>;", body[:body.index("\n}")]), kernel
    assert "void features_kernel_tex(const TraceParams P, const TexParams X" in feat


def test_null_handle_rules(ptmi_lib):
    P = ptmi_lib
    lib = P.load_library()
    img = np.ones((1, 1, 3), np.float32)
    uv = np.zeros((3, 2), np.float32)
    t = P.MeshTexture(struct_size=56, width=1, height=1, filter=0, wrap=0, bgr=img.ctypes.data, uvs=uv.ctypes.data, n_uvs=3, uv_indices=None)
    assert lib.pt_set_mesh_texture(None, 0, C.byref(t)) == -1
    assert lib.pt_last_error(None).decode() == "pt_set_mesh_texture: null handle"
    assert lib.pt_set_mesh_texture(None, 0, None) == -1
    assert lib.pt_get_mesh_texture_info(None, 0, C.byref(P.MeshTextureInfo(struct_size=40))) == -1
    o = np.zeros((1, 3), np.float32)
    out = np.zeros(3, np.float32)
    assert lib.pt_mesh_texel(None, o.ctypes.data, o.ctypes.data, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                             out.ctypes.data) == -1


def test_the_bindings_argument_checks(ptmi_lib):
    P = ptmi_lib
    v = np.float32([(0, 0, -2), (1, 0, -2), (0, 1, -2), (1, 1, -2.5)])
    t = np.uint32([(0, 1, 2), (1, 3, 2)])
    img = np.ones((3, 5, 3), np.float32)
    uv = np.float32([(0, 0), (1, 0), (0, 1), (1, 1)])
    plain = {"shape": "mesh", "material": "diffuse", "vertices": v, "triangles": t}
    good = dict(plain, texture=img, uvs=uv)
    table, meshes = P.scene_meshes([dict(good, uv_indices=t, texture_filter="nearest", texture_wrap="clamp")])   # the keys are known
    assert table["shape"].tolist() == [4] and len(meshes) == 1
    got = P.mesh_textures([plain, {"shape": "sphere"}, dict(good, uv_indices=t, texture_filter="nearest"), good])
    assert [(k, i is None, f, w) for k, _, _, i, f, w in got] == [(1, False, "nearest", "repeat"), (2, True, "bilinear", "repeat")]
    with pytest.raises(ValueError, match="texture without uvs"):
        P.mesh_textures([dict(plain, texture=img)])
    for key, value in (("uvs", uv), ("uv_indices", t), ("texture_filter", "nearest"), ("texture_wrap", "clamp")):
        with pytest.raises(ValueError, match="%s without texture" % key):
            P.mesh_textures([dict(plain, **{key: value})])
    r = object.__new__(P.Renderer)                              # no handle: the checks below run before the library is called
    for image, uvs, indices, kw, match in [
            (np.ones((3, 5), np.float32), uv, None, {}, "shape \\(H, W, 3\\)"), (np.ones((3, 5, 4), np.float32), uv, None, {}, "shape \\(H, W, 3\\)"),
            (np.ones((0, 5, 3), np.float32), uv, None, {}, "shape \\(H, W, 3\\)"), (np.ones((1, 8193, 3), np.float32), uv, None, {}, "at most 8192 x 8192"),
            (img, None, None, {}, "needs uvs"), (img, np.zeros((4, 3)), None, {}, "shape \\(N, 2\\)"), (img, np.zeros((0, 2)), None, {}, "shape \\(N, 2\\)"),
            (img, uv, None, {"filter": "cubic"}, "filter must be one of"), (img, uv, None, {"wrap": "mirror"}, "wrap must be one of"),
            (img, uv, t.ravel(), {}, "shape \\(T, 3\\)"), (img, uv, t.astype(np.float32), {}, "shape \\(T, 3\\)"),
            (img, uv, t.astype(np.int64) - 1, {}, "shape \\(T, 3\\)"), (None, uv, None, {}, "without an image"), (None, None, t, {}, "without an image")]:
        with pytest.raises(ValueError, match=match):
            r.set_mesh_texture(0, image, uvs, indices, **kw)
    for o, d in [(np.zeros((2, 2)), np.zeros((2, 2))), (np.zeros((2, 3)), np.zeros((3, 3)))]:
        with pytest.raises(ValueError, match="shape \\(n, 3\\)"):
            r.mesh_texel(o, d)
