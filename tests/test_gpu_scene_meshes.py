"""Triangle meshes in runtime scenes (pt_set_scene_meshes) on the GPU.

1. The pin: a mesh of ten triangles against the same triangles as ten PT_SHAPE_TRIANGLE rows -- pt_trace_paths records, production
   accumulators and feature buffers bit for bit (object_id through the obvious map).
2. The production kernels' mesh instances against pt_trace_paths on the same handle, bit for bit, on large meshes.
3. pt_trace_paths against the float64 model (tests/scene_mesh_model.py) at the project's rule 2 R (spread + 2e-6 scale), R = 0.68.
4. pt_mesh_intersect: the tree walk equals brute force equals the CPU program tests/mesh_bvh_main.cpp on its fixtures and rays.
5. Closed forms.   6. Unchanged behaviour.   7. The camera.   8. The guides.   9. NIF sharing, the memo and the denoiser.
(Meshes in the CLI are not built: DESIGN.md section 4.16.)
"""
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import scene_mesh_model as MM
from tests import scene_model as M
from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W, H = 64, 48
ENV = (0.75, 1.5, 3.0)
FIXTURES = ["icosphere2", "icosphere4", "grid", "doubled", "sliver", "single"]


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


# ---- the CPU program's fixtures, rays and results (a seed, not a file: the program makes them on the spot)

@pytest.fixture(scope="module")
def bvh_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_bvh") / "mesh_bvh")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "mesh_bvh_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


_dumps = {}


def _dump(exe, name):
    """(vertices, triangles, origins, directions, t, triangle) of a fixture, as the CPU program made and traced them."""
    if name not in _dumps:
        path = os.path.join(os.path.dirname(exe), name + ".bin")
        subprocess.run([exe, "--dump", name, path], check=True, timeout=120)
        raw = np.fromfile(path, np.uint32)
        os.remove(path)
        assert raw[0] == 0x4d455348
        nv, nt, nr = int(raw[1]), int(raw[2]), int(raw[3])
        parts, at = [], 4
        for count, dtype in ((3 * nv, F32), (3 * nt, np.uint32), (3 * nr, F32), (3 * nr, F32), (nr, F32), (nr, np.int32)):
            parts.append(raw[at:at + count].view(dtype))
            at += count
        assert at == len(raw)
        _dumps[name] = (parts[0].reshape(-1, 3), parts[1].reshape(-1, 3), parts[2].reshape(-1, 3), parts[3].reshape(-1, 3), parts[4], parts[5])
    return _dumps[name]


def _scaled(v, scale, centre):
    """The fixture's vertices blown up about their mean to `scale` times their size and moved to `centre` (binary32 on the host)."""
    v = np.asarray(v, np.float64)
    return F32((v - v.mean(0)) * scale + np.asarray(centre, np.float64))


def _mesh(v, t, material, colour=(1.0, 1.0, 1.0)):
    return {"shape": "mesh", "material": material, "colour": colour, "vertices": v, "triangles": t}


def _tri(v, material, colour=(1.0, 1.0, 1.0)):
    return {"shape": "triangle", "material": material, "colour": colour, "vertices": tuple(map(tuple, v))}


def _sph(c, r, material, colour=(1.0, 1.0, 1.0)):
    return {"shape": "sphere", "material": material, "centre": c, "radius": r, "colour": colour}


def _dsc(c, n, r, material, colour=(1.0, 1.0, 1.0)):
    return {"shape": "disc", "material": material, "centre": c, "normal": n, "radius": r, "colour": colour}


def _nif(r):
    r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())


def _renderer(P, scene, camera="none", half=False, spp=1, ipb=0, const=True, depth=PM.DEPTH, roulette=PM.ROULETTE, seed=PM.SEED):
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT, iterations_per_batch=ipb)
    if const:
        r.set_constant_env(ENV)
    else:
        _nif(r)
    r.init_render_settings(seed=seed, samples_per_step=spp, aa_noise_scale=PM.AA_SCALE)
    r.set_scene(scene)
    if PM.CAMERAS[camera] is not None:
        r.set_camera(**PM.CAMERAS[camera])
    return r


def _step(P, r):
    rec = P.worklist(W, H)
    r.setup(rec)
    r.path_trace()
    return rec, r.read_results(rec)


def _radiance(p, emission, env=F32(ENV)):
    want = np.zeros((len(p), 3), F32)
    for code, col in ((1, env), (2, F32(emission))):
        m = p["escaped"] == code
        want[m] = col[None, :] * p["throughput"][m]
    return want


# ---- 1. the pin

# an open box of ten triangles (no front face), a fifth of a unit across, turned so that no wall squarely faces a camera
def _box():
    c = np.array([0.02, -0.05, -0.55])
    h = 0.1
    ang = 0.37
    rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.21), -np.sin(0.21)], [0, np.sin(0.21), np.cos(0.21)]])
    corners = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], float) * h
    v = F32(corners @ rot.T + c)
    quads = [(0, 1, 3, 2), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]       # back, bottom, top, left, right
    t = np.uint32([tri for a, b, c_, d in quads for tri in ((a, b, c_), (a, c_, d))])
    return v, t


LAMP = (6.0, 4.5, 3.0)
PIN_CASES = [("none", False, "diffuse", True), ("moved", True, "specular", True), ("lens", False, "refractive", False),
             ("lens_moved", True, "emissive", True), ("moved", False, "refractive", True), ("none", True, "diffuse", False),
             ("lens_moved", False, "specular", False), ("lens", True, "diffuse", True)]


def _pin_scenes(material):
    v, t = _box()
    colour = LAMP if material == "emissive" else (0.8, 0.6, 0.4)
    # (the lamp sits exactly on the camera's horizontal plane: on the image's middle row its normal.y is -0 in both feature kernels)
    before = [_sph((0.05, 0.0, -0.5), 0.03, "emissive", LAMP)]
    after = [_dsc((0.0, -0.2, -0.55), (0.1, 1.0, 0.05), 0.6, "diffuse", (0.7, 0.7, 0.7)), _sph((-0.04, -0.09, -0.5), 0.04, "refractive", (0.9, 0.9, 0.9))]
    mesh = before + [_mesh(v, t, material, colour)] + after
    rows = before + [_tri(v[list(tri)], material, colour) for tri in t] + after
    return mesh, rows, len(t)


@pytest.mark.parametrize("camera,half,material,const", PIN_CASES, ids=["%s-%s-%s-%s" % (c, "half" if h else "float", m, "const" if e else "nif")
                                                                     for c, h, m, e in PIN_CASES])
def test_a_mesh_equals_its_triangles_as_rows(ptmi_lib, camera, half, material, const):
    P = ptmi_lib
    mesh, rows, k = _pin_scenes(material)
    out = []
    for scene in (mesh, rows):
        r = _renderer(P, scene, camera, half, spp=2, ipb=1, const=const)
        try:
            rec, st = _step(P, r)
            paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 1, np.uint32))
            out.append((rec.copy(), st.as_dict(), paths, r.feature_buffers(), r.scene_ex()))
        finally:
            r.close()
    (rec_m, st_m, p_m, f_m, s_m), (rec_t, st_t, p_t, f_t, s_t) = out
    assert s_m["shape"].tolist() == [0, 4, 1, 0] and len(s_t) == k + 3
    assert p_m.tobytes() == p_t.tobytes()                                           # pt_trace_paths records
    assert rec_m.tobytes() == rec_t.tobytes()                                       # production accumulators, lengths and counts
    for key in ("paths", "segments", "escaped"):
        assert st_m[key] == st_t[key]
    ids = f_t["object_id"].copy()
    ids[(ids >= 1) & (ids <= k)] = 1
    ids[ids > k] -= k - 1
    assert np.array_equal(f_m["object_id"], ids)
    for key in ("depth", "normal", "albedo"):
        bad = np.argwhere(_bits(f_m[key]) != _bits(f_t[key]))
        for at in bad[:5]:
            px = tuple(at[:2])
            print("feature %s differs at pixel %s: object %d / %d, mesh %r rows %r" % (
                key, px, f_m["object_id"][px], f_t["object_id"][px], f_m[key][px].tolist(), f_t[key][px].tolist()))
        assert len(bad) == 0
    # not vacuous: the mesh is seen, hit at depth and paths of every outcome exist
    assert np.count_nonzero(f_m["object_id"] == 1) > 20 and p_m["length"].max() >= 3
    assert set(np.unique(p_m["escaped"]).tolist()) >= {1, 2}


# ---- 2. production kernels against pt_trace_paths on large meshes

def _big_scene(exe):
    sv, st_ = _dump(exe, "icosphere4")[:2]
    gv, gt = _dump(exe, "grid")[:2]
    ball = _scaled(sv, 1.1, (0.03, -0.03, -0.55))          # 0.22 across
    floor = _scaled(gv, 0.8, (0.0, -0.19, -0.55))
    lamp = {"shape": "parallelogram", "material": "emissive", "colour": LAMP,
            "vertices": ((-0.08, 0.22, -0.62), (0.08, 0.23, -0.62), (-0.08, 0.2, -0.48))}
    return [_mesh(ball, st_, "refractive", (0.9, 0.95, 0.9)), lamp, _mesh(floor, gt, "diffuse", (0.8, 0.7, 0.5)),
            _sph((-0.15, -0.1, -0.6), 0.05, "specular")]


@pytest.mark.parametrize("camera,half,const", [("none", False, True), ("moved", True, False), ("lens", True, True), ("lens_moved", False, True)])
def test_production_kernels_equal_trace_paths(ptmi_lib, bvh_program, camera, half, const):
    P = ptmi_lib
    spp = 5
    r = _renderer(P, _big_scene(bvh_program), camera, half, spp=spp, ipb=2, const=const)
    try:
        info = [r.mesh_info(k) for k in range(2)]
        assert [i["object_index"] for i in info] == [0, 2] and [i["n_triangles"] for i in info] == [5120, 2048]
        assert all(i["max_leaf"] <= 4 and i["n_nodes"] <= 2 * i["n_triangles"] - 1 and i["pad"] > 0 for i in info)
        seen = set()
        for step in range(3):
            rec, st = _step(P, r)
            assert st.first_sample == step * spp and st.trace_launches >= 3                       # 5 = 2 + 2 + 1: ragged
            paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
            assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
            assert st.paths == spp * W * H and st.segments == sum(int(p["length"].sum()) for p in paths)
            assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
            if const:
                terms = np.stack([_radiance(p, LAMP).astype(np.float64) for p in paths])
                got = np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64)
                assert np.all(np.abs(got - terms.sum(0)) <= 5 * 2.0 ** -24 * np.abs(terms).sum(0))  # any order of summation
            for p in paths:
                seen |= set(np.unique(p["escaped"]).tolist())
        # one sample per step on the same handle: the accumulators are the records' radiance bit for bit
        r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
        rec, st = _step(P, r)
        p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
        assert np.array_equal(rec["pathLength"], p["length"])
        if const:
            assert np.array_equal(_bits(np.stack([rec["r"], rec["g"], rec["b"]], -1)), _bits(_radiance(p, LAMP)))
    finally:
        r.close()
    assert seen >= {0, 1, 2} and p["length"].max() >= 4


# ---- 3. pt_trace_paths against the float64 model

@pytest.mark.parametrize("camera,half", MM.CASES, ids=["%s-%s" % (c, "half" if h else "float") for c, h in MM.CASES])
def test_trace_paths_against_the_float64_model(oracle, ptmi_lib, camera, half):
    """Largest ratio measured on an MI355X over the four cases: see profiles/r22_meshes.txt."""
    P = ptmi_lib
    uu, vv, ss, cam, plain, fragile, spread = MM.case(camera, half)
    objs = MM.world_scene(camera)
    r = P.Renderer(PM.W, PM.H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT)
    try:
        r.set_constant_env(PM.ENV)
        r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
        r.set_scene(objs)
        if PM.CAMERAS[camera] is not None:
            r.set_camera(**PM.CAMERAS[camera])
        info = [r.mesh_info(k) for k in range(2)]
        p = r.trace_paths(uu, vv, ss)
    finally:
        r.close()
    assert [i["n_triangles"] for i in info] == [320, 128] and [i["object_index"] for i in info] == [0, 2]
    assert np.array_equal(p["cam"], cam)                    # the model ran on the camera rays the library forms
    same, ratio = PM.compare(p, plain, fragile, spread)
    ok = ~fragile
    print("mesh model / %s / %s: fragile %.2f %%, largest ratio %.3f of %.3f allowed; mismatching outcomes %d" % (
        camera, "half" if half else "float", 100 * fragile.mean(), ratio, M.GPU_FACTOR,
        np.count_nonzero((p["length"] != plain["length"])[ok] | (p["escaped"] != plain["escaped"])[ok])))
    assert fragile.mean() <= M.FRAGILE_CAP
    assert same
    assert ratio <= M.GPU_FACTOR
    assert set(np.unique(p["escaped"]).tolist()) == {0, 1, 2} and p["length"].max() >= 4


# ---- 4. pt_mesh_intersect

@pytest.mark.parametrize("name", FIXTURES)
def test_mesh_intersect_walk_equals_brute_force_equals_the_cpu(ptmi_lib, bvh_program, name):
    P = ptmi_lib
    v, t, o, d, cpu_t, cpu_tri = _dump(bvh_program, name)
    assert len(o) >= 1 << 16
    r = P.Renderer(W, H)
    try:
        r.set_scene([_mesh(v, t, "diffuse")])
        walk = r.mesh_intersect(o, d)
        brute = r.mesh_intersect(o, d, brute=True)
        # under a pose the hook still answers in world space, and the render's trees come back afterwards
        r.set_camera(**PM.CAMERAS["moved"])
        posed = r.mesh_intersect(o[:4096], d[:4096])
        info = r.mesh_info(0)
    finally:
        r.close()
    assert info["n_triangles"] == len(t) and info["object_index"] == 0
    differ = (_bits(walk[0]) != _bits(brute[0])) | (walk[1] != brute[1]) | (walk[2] != brute[2])
    print("%s: %d rays, %d hits, %d differ between walk and brute force, %d between device and CPU" % (
        name, len(o), np.count_nonzero(walk[1] >= 0), differ.sum(),
        np.count_nonzero((_bits(walk[0]) != _bits(cpu_t)) | (walk[2] != cpu_tri))))
    assert not differ.any()
    assert np.array_equal(_bits(walk[0]), _bits(cpu_t)) and np.array_equal(walk[2], cpu_tri)
    assert np.array_equal(walk[1], np.where(cpu_tri >= 0, 0, -1))
    assert np.all(walk[0][cpu_tri < 0] == 0)
    assert all(np.array_equal(a[:4096], b) for a, b in zip(walk, posed))
    if name == "doubled":
        assert np.all(walk[2][walk[2] >= 0] % 2 == 0)                                # the lower index wins everywhere


def test_mesh_intersect_among_other_objects_and_its_errors(ptmi_lib, bvh_program):
    P = ptmi_lib
    v, t, o, d, cpu_t, cpu_tri = _dump(bvh_program, "icosphere2")
    o, d = o[:8192], d[:8192]
    r = P.Renderer(W, H)
    try:
        with pytest.raises(P.PtError, match="holds no mesh"):
            r.mesh_intersect(o, d)
        with pytest.raises(P.PtError, match="mesh 0 of 0"):
            r.mesh_info(0)
        # a sphere declared BEFORE the mesh that encloses it hides it; declared after, an equal distance never beats the mesh
        r.set_scene([_sph((0.37, -0.21, -2.9), 0.11, "diffuse"), _mesh(v, t, "diffuse")])
        t1, obj1, tri1 = r.mesh_intersect(o, d)
        b1 = r.mesh_intersect(o, d, brute=True)
        r.set_scene([_mesh(v, t, "diffuse"), _mesh(v, t, "specular")])                # the same mesh twice: declaration order, strict <
        t2, obj2, tri2 = r.mesh_intersect(o, d)
        assert r.mesh_info(1)["object_index"] == 1
        with pytest.raises(P.PtError, match="mesh 2 of 2"):
            r.mesh_info(2)
        assert r.mesh_intersect(o[:0], d[:0])[0].shape == (0,)
    finally:
        r.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((t1, obj1, tri1), b1))
    outside = np.linalg.norm(o - np.float32((0.37, -0.21, -2.9)), axis=1) > 0.12
    assert np.all(obj1[outside & (obj1 >= 0)] == 0) and np.all(tri1[obj1 == 0] == -1) and np.count_nonzero(obj1 == 1) > 0
    hit = cpu_tri[:8192] >= 0
    assert np.all(obj2[hit] == 0) and np.array_equal(tri2, cpu_tri[:8192]) and np.array_equal(_bits(t2), _bits(cpu_t[:8192]))


# ---- 5. closed forms

def _render(P, scene, const, spp, depth=8, roulette=8, steps=1):
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette, sample_precision=P.SAMPLES_FLOAT, iterations_per_batch=4)
    try:
        r.set_constant_env(const)
        r.init_render_settings(seed=5, samples_per_step=spp)
        r.set_scene(scene)
        rec = P.worklist(W, H)
        r.setup(rec)
        r.path_trace()
        st = r.read_results(rec).as_dict()
        r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)[0].copy()
        return rec, film, st
    finally:
        r.close()


def test_closed_emissive_and_mirror_spheres_around_the_camera(ptmi_lib, bvh_program):
    P = ptmi_lib
    v, t = _dump(bvh_program, "icosphere2")[:2]
    around = _scaled(v, 20.0, (0.0, 0.0, 0.0))                                        # radius 2 about the camera
    E, spp = (0.5, 1.0, 2.0), 4
    rec, film, st = _render(P, [_mesh(around, t, "emissive", E)], ENV, spp)
    assert np.all(film == F32(E[::-1]))                                               # its emission exactly ...
    assert np.all(rec["pathLength"] == spp) and st["escaped"] == 0 and st["segments"] == st["paths"]   # ... with length 1
    rec, film, st = _render(P, [_mesh(around, t, "specular")], ENV, spp, depth=6, roulette=6)
    assert st["escaped"] == 0 and np.all(film == 0)                                   # a closed mirror's inside never escapes
    assert np.all(rec["pathLength"] == 6 * spp)


def _flat_grid(n, half_size, z):
    """A flat square of n x n cells, two triangles each, in the plane z: 2 n^2 triangles, a tree several levels deep."""
    ij = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy"), -1).reshape(-1, 2)
    v = np.zeros((len(ij), 3), F32)
    v[:, 0] = (ij[:, 0] / n - 0.5) * 2 * half_size
    v[:, 1] = (ij[:, 1] / n - 0.5) * 2 * half_size
    v[:, 2] = z
    t = [tri for j in range(n) for i in range(n) for a in [j * (n + 1) + i] for tri in ((a, a + 1, a + n + 1), (a + 1, a + n + 2, a + n + 1))]
    return v, np.uint32(t)


def test_furnace_on_a_mesh_that_fills_the_view(ptmi_lib):
    """The polygon furnace on a mesh with a real tree: a flat diffuse square of 16 x 16 x 2 = 512 triangles that fills the view under
    a constant L gives c L / 2 (E[cos theta] = 1/2 and every bounce leaves the plane; the statistic of
    test_gpu_scene_polygons.py::test_furnace_on_a_parallelogram).  Every interior edge and vertex is shared: a hole between
    neighbouring triangles would show as a path of length 1.  (A CLOSED diffuse box seen from inside never sees the sky: the test
    below is about it.)"""
    P = ptmi_lib
    spp = 20
    c, L = np.array([0.8, 0.5, 0.25]), 2.0
    v, t = _flat_grid(16, 2.0, -1.0)
    r = P.Renderer(W, H)
    try:
        r.set_scene([_mesh(v, t, "diffuse", tuple(c))])
        info = r.mesh_info(0)
    finally:
        r.close()
    assert info["n_triangles"] == 512 and info["depth"] >= 7 and info["n_nodes"] >= 255
    rec, film, st = _render(P, [_mesh(v, t, "diffuse", tuple(c))], (L, L, L), spp)
    n = W * H * spp
    assert n >= 50000 and st["paths"] == n
    mean = film.astype(np.float64).mean(axis=0)[::-1]
    sigma = c * L * np.sqrt((1.0 / 3.0 - 0.25) / n)
    print("furnace: mean / (c L / 2) = %s, 5 sigma = %s of it" % (mean / (c * L / 2), 5 * sigma / (c * L / 2)))
    assert np.all(np.abs(mean - c * L / 2) < 5 * sigma), (mean, c * L / 2, sigma)
    assert st["escaped"] == st["paths"] and np.all(rec["pathLength"] == 2 * spp)


@pytest.mark.parametrize("material", ["specular", "diffuse"])
def test_a_closed_box_leaks_exactly_what_its_triangles_as_rows_leak(ptmi_lib, material):
    """Moeller-Trumbore is not watertight: along the edges between the faces of a closed unit box about the camera a few rays pass
    between two triangles that each reject them by a rounding of a + b (include/ptmi.h says so).  That is a property of the pinned
    triangle test and its epsilon, not of the tree, the pad or the walk: the same twelve triangles as PT_SHAPE_TRIANGLE rows let the
    IDENTICAL paths out -- records, accumulators and counts bit for bit."""
    P = ptmi_lib
    corners = F32([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.uint32([tri for a, b, c_, d in quads for tri in ((a, b, c_), (a, c_, d))])
    scenes = ([_mesh(corners, t, material, (0.8, 0.5, 0.25))], [_tri(corners[list(tri)], material, (0.8, 0.5, 0.25)) for tri in t])
    out = []
    for scene in scenes:
        r = _renderer(P, scene, "none", spp=2, ipb=1, depth=6, roulette=6)
        try:
            rec, st = _step(P, r)
            p = np.concatenate([r.trace_paths(rec["u"], rec["v"], np.full(len(rec), k, np.uint32)) for k in range(2)])
            out.append((rec.tobytes(), st.as_dict(), p))
        finally:
            r.close()
    (rec_m, st_m, p_m), (rec_t, st_t, p_t) = out
    leaked = np.count_nonzero(p_m["escaped"] == 1)
    print("closed %s box: %d of %d paths leave it, as a mesh and as rows alike" % (material, leaked, len(p_m)))
    assert p_m.tobytes() == p_t.tobytes() and rec_m == rec_t
    assert all(st_m[k] == st_t[k] for k in ("paths", "segments", "escaped")) and st_m["escaped"] == leaked
    # (measured on an MI355X: 8 of 6144 mirror paths and 22 of 6144 diffuse paths of six bounces; no bound is set on the count --
    # what is asserted is that the tree adds nothing to it and takes nothing away)


# ---- 6. unchanged behaviour

def _everything(P, setter, camera="lens_moved"):
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE, iterations_per_batch=2)
    try:
        _nif(r)
        r.init_render_settings(seed=PM.SEED, samples_per_step=3)
        setter(r)
        if camera:
            r.set_camera(**PM.CAMERAS[camera])
        rec = P.worklist(W, H)
        r.setup(rec)
        out = []
        for _ in range(2):
            r.path_trace()
            st = r.read_results(rec)
            out.append((rec.tobytes(), st.paths, st.segments, st.escaped))
        out.append(r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 4, np.uint32)).tobytes())
        return out
    finally:
        r.close()


def test_a_table_without_a_mesh_is_set_scene_ex_and_restore_is_the_builtin_scene(ptmi_lib, bvh_program):
    P = ptmi_lib
    table = P.scene_array_ex(PM.world_scene("cornell", "lens_moved"))
    assert P.has_polygon(table)
    assert _everything(P, lambda r: r.set_scene_meshes(table, [])) == _everything(P, lambda r: r.set_scene(table))
    builtin = _everything(P, lambda r: None)
    v, t = _dump(bvh_program, "icosphere2")[:2]

    def set_then_restore(r):
        r.set_scene([_mesh(_scaled(v, 2.0, (0, 0, -0.6)), t, "diffuse")])
        assert r.scene_ex()["shape"].tolist() == [4]
        lib = P.load_library()
        assert lib.pt_set_scene_meshes(r.handle, None, 0, 84, None, 0) == 0           # (NULL, 0, stride, NULL, 0)
        assert len(r.scene_ex()) == 6
        with pytest.raises(P.PtError, match="holds no mesh"):
            r.mesh_intersect(np.zeros((1, 3), F32), np.zeros((1, 3), F32))
    assert _everything(P, set_then_restore) == builtin


def test_getters_and_a_rejected_table_keeps_the_mesh_scene(ptmi_lib, bvh_program):
    P = ptmi_lib
    v, t = _dump(bvh_program, "icosphere2")[:2]
    scene = [_sph((0.2, 0, -0.6), 0.05, "specular"), _mesh(_scaled(v, 1.5, (0, 0, -0.6)), t, "diffuse", (0.2, 0.4, 0.6))]
    r = _renderer(P, scene)
    try:
        s = r.scene_ex()
        assert s["shape"].tolist() == [0, 4] and s["material"].tolist() == [1, 0]
        assert np.array_equal(s["colour"][1], F32((0.2, 0.4, 0.6)))
        assert np.all(s["centre"][1] == 0) and s["radius"][1] == 0 and np.all(s["normal"][1] == 0) and np.all(s["vertex"][1] == 0)
        with pytest.raises(P.PtError, match="holds a mesh: use pt_get_scene_ex"):
            r.scene()
        rec, st = _step(P, r)
        before = rec.tobytes()
        bad = [scene[0], _mesh(F32([(0, 0, 0), (1, 1, 1), (2, 2, 2)]), np.uint32([(0, 1, 2)]), "diffuse")]
        with pytest.raises(P.PtError, match="scene object 1, mesh 0, triangle 0: vertices are collinear"):
            r.set_scene(bad)
        with pytest.raises(P.PtError, match="shape must be 0 \\(sphere\\), 1 \\(disc\\), 2 \\(triangle\\) or 3 \\(parallelogram\\) \\(got 4\\)"):
            r._check(r._lib.pt_set_scene_ex(r.handle, s.ctypes.data, len(s), 84))
        assert r.scene_ex().tobytes() == s.tobytes() and r.mesh_info(0)["n_triangles"] == len(t)
        rec2, st2 = _step(P, r)                                                    # ... and still renders: the next sample
        p = r.trace_paths(rec2["u"], rec2["v"], np.full(len(rec2), st2.first_sample, np.uint32))
        assert st2.first_sample == 1 and np.array_equal(rec2["pathLength"], p["length"]) and rec2.tobytes() != before
    finally:
        r.close()


# ---- 7. the camera

def test_meshes_follow_a_new_pose(ptmi_lib, bvh_program):
    P = ptmi_lib
    scene = _big_scene(bvh_program)
    r = _renderer(P, scene, "none", spp=2, ipb=1)
    try:
        rec, st = _step(P, r)
        first = [r.mesh_info(k) for k in range(2)]
        r.set_camera(**PM.CAMERAS["moved"])
        assert [r.mesh_info(k)["build_ms"] for k in range(2)] == [i["build_ms"] for i in first]     # stale until something traces
        rec, st = _step(P, r)
        second = [r.mesh_info(k) for k in range(2)]
        paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 3, np.uint32))
        feats = r.feature_buffers()
        assert [r.mesh_info(k)["build_ms"] for k in range(2)] == [i["build_ms"] for i in second]    # built once for this pose
    finally:
        r.close()
    assert all(a["build_ms"] != b["build_ms"] and a["build_ms"] > 0 and b["build_ms"] > 0 for a, b in zip(first, second))
    assert all(a["device_bytes"] == b["device_bytes"] and a["n_triangles"] == b["n_triangles"] for a, b in zip(first, second))
    fresh = _renderer(P, scene, "moved", spp=2, ipb=1)
    try:
        _step(P, fresh)                                                                            # samples 0, 1
        rec_f, _ = _step(P, fresh)                                                                 # samples 2, 3: the posed step above
        paths_f = fresh.trace_paths(rec_f["u"], rec_f["v"], np.full(len(rec_f), 3, np.uint32))
        feats_f = fresh.feature_buffers()
    finally:
        fresh.close()
    assert paths.tobytes() == paths_f.tobytes() and rec.tobytes() == rec_f.tobytes()
    assert all(feats[k].tobytes() == feats_f[k].tobytes() for k in feats)
    assert np.count_nonzero(feats["object_id"] == 0) > 20 and np.count_nonzero(feats["object_id"] == 2) > 20


# ---- 8. the guides

def test_guides_at_zero_are_the_unguided_bits_and_an_emissive_mesh_is_not_listed(ptmi_lib, bvh_program):
    P = ptmi_lib
    v, t = _dump(bvh_program, "icosphere2")[:2]
    gv, gt = _dump(bvh_program, "grid")[:2]
    scene = [_mesh(_scaled(gv, 0.8, (0.0, -0.19, -0.55)), gt, "diffuse", (0.8, 0.7, 0.5)),
             _mesh(_scaled(v, 0.4, (0.0, 0.1, -0.55)), t, "emissive", LAMP), _sph((0.12, -0.1, -0.5), 0.04, "emissive", LAMP)]

    def run(setup, spp=2, steps=2):
        r = _renderer(P, scene, "moved", spp=spp, ipb=1)
        try:
            setup(r)
            rec = P.worklist(W, H)
            r.setup(rec)
            for _ in range(steps):
                r.path_trace()
                r.read_results(rec)
                r.film_accumulate()
            info = r.light_guide_info()
            film = r.gather_hdr(W * H, P.HDR_FILM)[0].copy()
            return rec.tobytes(), film, info
        finally:
            r.close()

    sky = np.full((16, 32, 3), 0.1, F32)
    sky[3, 5] = 50.0
    plain = run(lambda r: None)
    zero = run(lambda r: (r.set_env_guide(sky, rows=8, cols=16, alpha=0.0), r.set_light_guide(beta=0.0)))
    assert zero[0] == plain[0] and np.array_equal(zero[1], plain[1])
    for polygons in (False, True):
        info = run(lambda r: r.set_light_guide(beta=0.5, polygons=polygons))[2]
        assert info["active"] and info["n_lights"] == 1 and info["object_index"].tolist() == [2]    # the sphere; never the mesh
    # the light-guided mesh instance estimates the same image: the image means agree within 5 combined standard errors of the
    # step means (the statistic of test_gpu_scene_polygons.py), and it is pt_trace_paths' guided twin bit for bit
    steps, spp = 12, 16
    films = {}
    for beta in (0.0, 0.5):
        r = _renderer(P, scene, "moved", spp=spp)
        try:
            if beta:
                r.set_light_guide(beta)
            means = []
            for _ in range(steps):
                rec, st = _step(P, r)
                means.append(np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64).mean(axis=0) / spp)
            films[beta] = np.array(means)
            if beta:
                r.init_render_settings(seed=PM.SEED + 1, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
                rec, st = _step(P, r)
                p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
                assert np.array_equal(rec["pathLength"], p["length"]) and st.escaped == np.count_nonzero(p["escaped"] == 1)
                got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
                assert np.array_equal(_bits(got), _bits(_radiance(p, LAMP))) and np.count_nonzero(p["escaped"] == 2) > 30
        finally:
            r.close()
    off, on = films[0.0], films[0.5]
    se = np.sqrt(off.var(axis=0, ddof=1) / steps + on.var(axis=0, ddof=1) / steps)
    z = (on.mean(axis=0) - off.mean(axis=0)) / se
    print("light guide on a mesh scene: off %s on %s, difference / combined se %s" % (off.mean(axis=0), on.mean(axis=0), z))
    assert np.all(np.abs(z) <= 5.0) and not np.array_equal(off, on)


# ---- 9. NIF sharing, the memo and the denoiser

def test_sharing_memo_and_denoiser_on_a_mesh_scene(ptmi_lib, bvh_program):
    P = ptmi_lib
    scene = _big_scene(bvh_program)

    def run(setup):
        r = _renderer(P, scene, "moved", True, spp=3, ipb=2, const=False)
        try:
            setup(r)
            rec = P.worklist(W, H)
            r.setup(rec)
            out = []
            for _ in range(2):
                r.path_trace()
                r.read_results(rec)
                r.film_accumulate()
                out.append(rec.tobytes())
            return out, r.denoise(source="film")
        finally:
            r.close()

    off, dn = run(lambda r: r.set_nif_sharing("off"))
    assert run(lambda r: r.set_nif_sharing("step"))[0] == off
    assert run(lambda r: r.set_nif_sharing("batch"))[0] == off
    assert run(lambda r: r.set_nif_memo(1 << 24))[0] == off
    assert dn.shape == (H, W, 3) and np.all(np.isfinite(dn)) and dn.max() > 0
