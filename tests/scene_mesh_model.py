"""The float64 model of a scene with meshes (pt_set_scene_meshes): it IS tests/scene_poly_model.py's model over the scene with every
mesh row expanded into its triangles, in index order, as PT_SHAPE_TRIANGLE rows of the mesh's material and colour -- what the header
says a mesh equals.  scene_poly_model.trace loops over the rows of a stored table of any length, so nothing of it changes; this file
adds the expansion, the meshes of the cases and their placement in front of each camera.

The model costs one Python loop trip per triangle and bounce, so the cases keep the meshes small -- an icosphere of 320 triangles
over a height field of 128, two meshes (the second one's tree and triangles do not start at 0 on the device), a parallelogram lamp
and a mirror sphere -- and take every third pixel at one sample.  The meshes are a fifth of a unit across and no face squarely faces a
posed camera ("Model and tests").  (scene_poly_model.trace records the object of every bounce as int8,
which wraps above 127 rows; it compares those records between its plain and perturbed runs only, together with lengths, outcomes and
choices, so a wrapped index still tells a changed hit from an unchanged one.)"""
import functools

import numpy as np

from ipu_path_trace_amd import ptmi
from tests import scene_model as M
from tests import scene_poly_model as PM

W, H = PM.W, PM.H
SAMPLE = 7
STRIDE = 3
CAMERAS = PM.CAMERAS
CASES = [("none", False), ("moved", True), ("lens", True), ("lens_moved", False)]      # (camera, samples_half)


def icosphere(k, radius, centre):
    """(vertices float64 (V, 3), triangles (20 x 4^k, 3)) of a subdivided icosahedron."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    p = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    p = [np.array(x, float) for x in p]
    for _ in range(k):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(p)
                p.append(0.5 * (p[a] + p[b]))
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(p)
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * radius + np.asarray(centre, float)
    return v, np.array(f, np.uint32)


def height_field(n, size, centre, bump, seed=5):
    """An n x n grid of two triangles per cell over a square of side `size` about `centre`, heights raised by up to `bump`."""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy"), -1).reshape(-1, 2)
    v = np.zeros((len(ij), 3))
    v[:, 0] = (ij[:, 0] / n - 0.5) * size + centre[0]
    v[:, 2] = (ij[:, 1] / n - 0.5) * size + centre[2]
    v[:, 1] = centre[1] + bump * rng.random(len(ij))
    t = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            t += [(a, a + 1, a + n + 1), (a + 1, a + n + 2, a + n + 1)]
    return v, np.array(t, np.uint32)


def _mesh(vt, material, colour):
    return {"shape": "mesh", "material": material, "colour": colour, "vertices": vt[0], "triangles": vt[1]}


# camera space: x right, y up, the view along -z
SCENE = [
    _mesh(icosphere(2, 0.1, (0.03, -0.02, -0.55)), "refractive", (0.9, 0.95, 0.9)),
    {"shape": "parallelogram", "material": "emissive", "colour": PM.EMISSION,
     "vertices": ((-0.08, 0.22, -0.62), (0.08, 0.23, -0.62), (-0.08, 0.2, -0.48))},
    _mesh(height_field(8, 0.7, (0.0, -0.19, -0.55), 0.04), "diffuse", (0.8, 0.7, 0.5)),
    {"shape": "sphere", "material": "specular", "centre": (-0.15, -0.1, -0.6), "radius": 0.05, "colour": (1.0, 1.0, 1.0)},
]


def world_scene(camera_name):
    """SCENE placed in front of the camera, as scene_poly_model.world_scene places its scenes: a camera-space point (x, y, z) is
    position + x r + y u - z f, rounded to the binary32 the library is given.  A list of dicts for Renderer.set_scene."""
    camera = CAMERAS[camera_name]
    pose = M._has_pose(camera)
    if pose:
        p, r, up, f = M.basis(camera)

    def points(c):
        c = np.asarray(c, np.float64)
        return np.float32(p + c[..., 0:1] * r + c[..., 1:2] * up - c[..., 2:3] * f) if pose else np.float32(c)
    out = []
    for o in SCENE:
        o = dict(o)
        if o["shape"] == "mesh":
            o["vertices"] = points(o["vertices"])
        elif "vertices" in o:
            o["vertices"] = tuple(tuple(float(x) for x in row) for row in points(o["vertices"]))
        else:
            o["centre"] = tuple(float(x) for x in points(o["centre"]))
        out.append(o)
    return out


def expand(objects):
    """Every mesh row replaced by its triangles in index order, as PT_SHAPE_TRIANGLE rows of the mesh's material and colour;
    also the map expanded row -> row of the mesh table."""
    rows, origin = [], []
    for i, o in enumerate(objects):
        if o["shape"] != "mesh":
            rows.append(o)
            origin.append(i)
            continue
        v = np.asarray(o["vertices"], np.float32)
        for tri in np.asarray(o["triangles"]):
            rows.append({"shape": "triangle", "material": o["material"], "colour": o["colour"],
                         "vertices": tuple(tuple(float(x) for x in v[k]) for k in tri)})
            origin.append(i)
    return rows, np.array(origin)


def stored(objects):
    """The expanded table as the library would store it (scene_poly_model.stored_scene_ex): the model's scene."""
    return PM.stored_scene_ex(expand(objects)[0])


def pixels():
    u, v = PM.all_pixels()
    return u[::STRIDE], v[::STRIDE]


@functools.lru_cache(maxsize=None)
def case(camera_name, samples_half):
    """The GPU test's inputs and the model's analysis of them: (u, v, sample, cam, plain, fragile, spread)."""
    u, v = pixels()
    ss = np.full(len(u), SAMPLE, np.uint32)
    cam = PM.oracle_cam(SAMPLE)[::STRIDE]
    plain, fragile, spread = PM.analyse(stored(world_scene(camera_name)), CAMERAS[camera_name], PM.case_options(samples_half),
                                        u, v, ss, cam, PM.ENV)
    return u, v, ss, cam, plain, fragile, spread
