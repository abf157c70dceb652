"""Fixtures of the mesh-texture tests (pt_set_mesh_texture): the meshes of tests/mesh_normals_fixtures.py again, two or three per
scene, the FIRST always without a texture, so that a textured mesh's slots and its descriptor do not start at 0.  The image is a
non-square 5 x 3 of distinct values (a swapped width and height or a flipped t returns another texel), and the coordinates leave
the unit square on purpose, so that the wrap decides.

  nearest_repeat   a plain icosphere; height_field(8) with per-vertex uvs linear in x and z over [-1.3, 2.2], NEAREST, REPEAT
  nearest_clamp    the same meshes, uvs over [-0.5, 1.5], NEAREST, CLAMP
  bilinear_repeat  a plain height_field; the icosphere of the "odd" normals fixture (every second winding reversed) with PER-CORNER
                   uvs -- a seam: the triangles below the ring use a second set, shifted --, BILINEAR, REPEAT; one triangle with a
                   1 x 1 image
  bilinear_clamp   a plain height_field; the icosphere with per-vertex uvs, BILINEAR, CLAMP; one triangle with a constant 3 x 2
                   image, NEAREST

write() puts a fixture into the file tests/mesh_texture_main.cpp reads, read_dump() reads what that program wrote, and scene() gives
the same fixture to a Renderer."""
import os
import struct
import subprocess

import numpy as np

from tests import mesh_normals_fixtures as NF
from tests import scene_mesh_model as MM

MAGIC_IN, MAGIC_OUT = 0x5458544c, 0x5458544f
NAMES = ("nearest_repeat", "nearest_clamp", "bilinear_repeat", "bilinear_clamp")
NEAREST, BILINEAR, REPEAT, CLAMP = 0, 1, 0, 1

ROOT = NF.ROOT
FLAGS = NF.FLAGS


def build_program(directory):
    """tests/mesh_texture_main.cpp under ASan and UBSan (a stand-alone host program)."""
    exe = os.path.join(str(directory), "mesh_texture")
    build = subprocess.run(["g++"] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "mesh_texture_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def run_fixture(exe, directory, name, dump=True):
    """The program over fixture `name`; returns (stdout, path of the dump or None)."""
    path = os.path.join(str(directory), name + ".fixture")
    write(name, path)
    args = [exe, path]
    out = os.path.join(str(directory), name + ".dump") if dump else None
    if dump:
        args += ["--dump", out]
    run = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "MESH_TEXTURE_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    return run.stdout, out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def image_5x3():
    """(3, 5, 3) B,G,R: fifteen distinct texels, each channel distinct too; values between 0.1 and 1.9."""
    r, c = np.mgrid[0:3, 0:5]
    base = (5 * r + c).astype(np.float64)
    return _f32(np.stack([0.1 + 0.11 * base, 1.9 - 0.09 * base, 0.3 + 0.05 * ((7 * base) % 15)], axis=-1))


def image_constant(h, w, bgr=(0.25, 0.5, 0.75)):
    return _f32(np.broadcast_to(np.asarray(bgr, np.float32), (h, w, 3)))


def planar_uvs(v, lo, hi, axes=(0, 2)):
    """(V, 2): linear in two coordinates of the vertices, the mesh's box mapped onto [lo, hi]^2."""
    p = np.asarray(v, np.float64)[:, list(axes)]
    a, b = p.min(axis=0), p.max(axis=0)
    return _f32(lo + (hi - lo) * (p - a) / (b - a))


def spherical_uvs(v, centre, scale=1.0):
    """(V, 2): longitude and latitude of the vertex about `centre`, each in [0, 1], times scale."""
    p = np.asarray(v, np.float64) - np.asarray(centre, np.float64)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    s = np.arctan2(p[:, 2], p[:, 0]) / (2.0 * np.pi) + 0.5
    t = np.arccos(np.clip(p[:, 1], -1.0, 1.0)) / np.pi
    return _f32(scale * np.stack([s, t], axis=-1))


def meshes(name):
    """[(vertices, triangles, texture or None)] of a fixture, in row order; texture = dict(image, uvs, uv_indices or None, filter, wrap)."""
    fv, ft = MM.height_field(*NF.FIELD)
    fv = _f32(fv)
    sv, st, _ = NF.sphere_mesh()
    if name in ("nearest_repeat", "nearest_clamp"):
        rep = name == "nearest_repeat"
        uvs = planar_uvs(fv, -1.3, 2.2) if rep else planar_uvs(fv, -0.5, 1.5)
        tex = dict(image=image_5x3(), uvs=uvs, uv_indices=None, filter=NEAREST, wrap=REPEAT if rep else CLAMP)
        return [(sv, st, None), (fv, ft, tex)]
    tv, tt, _ = NF.zero_sum_triangle()
    tri_uvs = _f32([(-0.4, 0.2), (1.7, 0.1), (0.6, 2.3)])
    if name == "bilinear_repeat":
        ov, ot, _, _, _ = NF.odd_sphere()
        V = len(ov)
        upper = spherical_uvs(ov, NF.CENTRE, 3.0)
        low = ov[ot].astype(np.float64)[:, :, 1].mean(axis=1) < NF.CENTRE[1]
        uvs = np.concatenate([upper, _f32(upper + np.float32(0.37))])   # the seam: the lower triangles use the shifted set
        idx = ot.astype(np.uint32).copy()
        idx[low] += np.uint32(V)
        tex = dict(image=image_5x3(), uvs=uvs, uv_indices=idx, filter=BILINEAR, wrap=REPEAT)
        one = dict(image=image_constant(1, 1, (0.625, 1.5, 0.125)), uvs=tri_uvs, uv_indices=None, filter=BILINEAR, wrap=REPEAT)
        return [(fv, ft, None), (ov, ot, tex), (tv, tt, one)]
    if name == "bilinear_clamp":
        tex = dict(image=image_5x3(), uvs=_f32(spherical_uvs(sv, NF.CENTRE, 2.0) - np.float32(0.5)), uv_indices=None, filter=BILINEAR, wrap=CLAMP)
        const = dict(image=image_constant(2, 3), uvs=tri_uvs, uv_indices=None, filter=NEAREST, wrap=CLAMP)
        return [(fv, ft, None), (sv, st, tex), (tv, tt, const)]
    raise KeyError(name)


def scene(name, materials=None, colour=(0.8, 0.7, 0.5), textures=True):
    """The fixture as a list of dicts for Renderer.set_scene (textures=False: no mesh textured)."""
    ms = meshes(name)
    out = []
    for (v, t, tex), mat in zip(ms, materials or ("diffuse",) * len(ms)):
        o = {"shape": "mesh", "material": mat, "colour": colour, "vertices": v, "triangles": t}
        if textures and tex is not None:
            o["texture"] = tex["image"]
            o["uvs"] = tex["uvs"]
            if tex["uv_indices"] is not None:
                o["uv_indices"] = tex["uv_indices"]
            o["texture_filter"] = tex["filter"]
            o["texture_wrap"] = tex["wrap"]
        out.append(o)
    return out


def write(name, path):
    ms = meshes(name)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC_IN, len(ms)))
        for v, t, tex in ms:
            if tex is None:
                f.write(struct.pack("<8I", len(v), len(t), 0, 0, 0, 0, 0, 0))
            else:
                h, w = tex["image"].shape[:2]
                f.write(struct.pack("<8I", len(v), len(t), len(tex["uvs"]), 0 if tex["uv_indices"] is None else 1, w, h, tex["filter"], tex["wrap"]))
            f.write(_f32(v).tobytes())
            f.write(np.ascontiguousarray(t, np.uint32).tobytes())
            if tex is not None:
                f.write(_f32(tex["uvs"]).tobytes())
                if tex["uv_indices"] is not None:
                    f.write(np.ascontiguousarray(tex["uv_indices"], np.uint32).tobytes())
                f.write(_f32(tex["image"]).tobytes())


def write_pfm(path, bgr):
    """A little-endian three-channel .pfm of an (H, W, 3) B,G,R image with rows top to bottom: the file holds R,G,B, bottom row first."""
    bgr = np.asarray(bgr, np.float32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (bgr.shape[1], bgr.shape[0]))
        f.write(np.ascontiguousarray(bgr[::-1, :, ::-1], dtype="<f4").tobytes())


def read_dump(path):
    """What tests/mesh_texture_main.cpp --dump wrote: dict of origin, dir (n, 3), t, mesh (index among the meshes, -1), triangle,
    uv (n, 2), bgr (n, 3)."""
    raw = open(path, "rb").read()
    magic, n = struct.unpack_from("<II", raw, 0)
    assert magic == MAGIC_OUT
    off = 8
    out = {}
    for key, dt, w in (("origin", np.float32, 3), ("dir", np.float32, 3), ("t", np.float32, 1), ("mesh", np.int32, 1),
                       ("triangle", np.int32, 1), ("uv", np.float32, 2), ("bgr", np.float32, 3)):
        a = np.frombuffer(raw, dt, n * w, off).copy()
        off += 4 * n * w
        out[key] = a.reshape(n, w) if w > 1 else a
    assert off == len(raw)
    return out
