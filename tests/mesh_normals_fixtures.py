"""Fixtures of the vertex-normal tests (pt_set_mesh_normals): scenes of two or three meshes built from tests/scene_mesh_model.py's
icosphere and height_field, one of them always flat, so that a smooth mesh's slots and normals do not start at 0.

  sphere  icosphere(2) with the exact radial normals (v - centre) / radius, per vertex; a flat height_field(8)
  field   a flat icosphere(2); height_field(8) with angle-weighted vertex normals (ptmi.vertex_normals), per vertex
  odd     a flat height_field(8); the icosphere with every second triangle's winding reversed and per-corner indices that crease
          the closed ring of edges between its upper and lower triangles (a vertex there has one normal for each side);
          a single triangle whose three corner normals sum to (numerically) zero, for the fallback to the geometric normal

write() puts a fixture into the file tests/mesh_normals_main.cpp reads, read_dump() reads what that program wrote, and
scene() / attach() give the same fixture to a Renderer."""
import os
import struct
import subprocess

import numpy as np

from tests import scene_mesh_model as MM

CENTRE = (0.03, -0.02, -0.55)
RADIUS = 0.1
FIELD = (8, 0.7, (0.0, -0.19, -0.55), 0.04)
MAGIC_IN, MAGIC_OUT = 0x4e524d4c, 0x4e524d4f
NAMES = ("sphere", "field", "odd")


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc")]
# python -m pytest tests/test_mesh_normals.py -s prints the measurement: 2.28e-5 (see that file's docstring)
CLOSED_FORM_MEASURED = 2.3e-5
CLOSED_FORM_BOUND = 2.0 * CLOSED_FORM_MEASURED


def build_program(directory):
    """tests/mesh_normals_main.cpp under ASan and UBSan (a stand-alone host program)."""
    exe = os.path.join(str(directory), "mesh_normals")
    build = subprocess.run(["g++"] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "mesh_normals_main.cpp")], capture_output=True, text=True)
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
    if name == "sphere":
        args += ["--sphere", "0"] + [repr(float(c)) for c in CENTRE]
    if name == "odd":
        args += ["--fallback", "2"]
    run = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "MESH_NORMALS_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    return run.stdout, out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def sphere_mesh():
    v, t = MM.icosphere(2, RADIUS, CENTRE)
    v = _f32(v)
    normals = _f32((v.astype(np.float64) - np.asarray(CENTRE)) / RADIUS)
    return v, t, normals


def field_mesh():
    from ipu_path_trace_amd import ptmi
    v, t = MM.height_field(*FIELD)
    v = _f32(v)
    return v, t, ptmi.vertex_normals(v, t)


def odd_sphere():
    """The icosphere, windings of odd triangles reversed, creased along the closed ring of edges between the triangles whose
    centroid lies above centre.y and those below: per-corner indices into 2 V normals, the radial one at k and, at V + k, the one
    the triangles below use -- the radial one again, but tilted at the ring's vertices."""
    v, t, radial = sphere_mesh()
    t = t.copy()
    t[1::2] = t[1::2][:, [0, 2, 1]]
    V = len(v)
    low = v[t].astype(np.float64)[:, :, 1].mean(axis=1) < CENTRE[1]
    ring = np.zeros(V, bool)
    ring[np.intersect1d(t[low].ravel(), t[~low].ravel())] = True
    below = radial.copy()
    below[ring] = _f32(radial[ring].astype(np.float64) + np.array([0.0, -0.6, 0.0]))   # not unit on purpose: the library normalises
    normals = np.concatenate([radial, below])
    idx = t.astype(np.uint32).copy()
    idx[low] += np.uint32(V)
    return v, t, normals, idx, int(ring.sum())


def zero_sum_triangle():
    v = _f32([(-0.2, 0.05, -0.5), (-0.12, 0.06, -0.52), (-0.17, 0.13, -0.5)])
    t = np.array([(0, 1, 2)], np.uint32)
    s = np.sqrt(3.0) / 2.0
    normals = _f32([(1.0, 0.0, 0.0), (-0.5, s, 0.0), (-0.5, -s, 0.0)])
    return v, t, normals


def meshes(name):
    """[(vertices, triangles, normals or None, normal_indices or None)] of a fixture, in row order."""
    if name == "sphere":
        fv, ft = MM.height_field(*FIELD)
        return [sphere_mesh() + (None,), (_f32(fv), ft, None, None)]
    if name == "field":
        sv, st, _ = sphere_mesh()
        return [(sv, st, None, None), field_mesh() + (None,)]
    if name == "odd":
        fv, ft = MM.height_field(*FIELD)
        ov, ot, on, oi, _ = odd_sphere()
        return [(_f32(fv), ft, None, None), (ov, ot, on, oi), zero_sum_triangle() + (None,)]
    raise KeyError(name)


MATERIALS = {"sphere": ("refractive", "diffuse"), "field": ("specular", "diffuse"), "odd": ("diffuse", "specular", "diffuse")}


def scene(name, materials=None, normals=True):
    """The fixture as a list of dicts for Renderer.set_scene (normals=False: every mesh flat)."""
    out = []
    for (v, t, n, i), mat in zip(meshes(name), materials or MATERIALS[name]):
        o = {"shape": "mesh", "material": mat, "colour": (0.8, 0.7, 0.5), "vertices": v, "triangles": t}
        if normals and n is not None:
            o["normals"] = n
            if i is not None:
                o["normal_indices"] = i
        out.append(o)
    return out


def write(name, path):
    ms = meshes(name)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC_IN, len(ms)))
        for v, t, n, i in ms:
            f.write(struct.pack("<IIII", len(v), len(t), 0 if n is None else len(n), 0 if i is None else 1))
            f.write(_f32(v).tobytes())
            f.write(np.ascontiguousarray(t, np.uint32).tobytes())
            if n is not None:
                f.write(_f32(n).tobytes())
            if i is not None:
                f.write(np.ascontiguousarray(i, np.uint32).tobytes())


def read_dump(path):
    """What tests/mesh_normals_main.cpp --dump wrote: dict of origin, dir (n, 3), t, mesh (index among the meshes, -1), triangle,
    bary (n, 2), normal (n, 3)."""
    raw = open(path, "rb").read()
    magic, n = struct.unpack_from("<II", raw, 0)
    assert magic == MAGIC_OUT
    off = 8
    out = {}
    for key, dt, w in (("origin", np.float32, 3), ("dir", np.float32, 3), ("t", np.float32, 1), ("mesh", np.int32, 1),
                       ("triangle", np.int32, 1), ("bary", np.float32, 2), ("normal", np.float32, 3)):
        a = np.frombuffer(raw, dt, n * w, off).copy()
        off += 4 * n * w
        out[key] = a.reshape(n, w) if w > 1 else a
    assert off == len(raw)
    return out
