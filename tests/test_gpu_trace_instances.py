"""Every instance of the trace, trace-paths and feature kernels (ipu_path_trace_amd/csrc/ptmi_trace_variant.h: 57 + 19 + 5) is
launched on the device, REPORTED as the instance that ran (pt_get_trace_variant) and pinned to its twins, bit for bit.  A constant
environment, SAMPLES_FLOAT, one sample per step, 64 x 48 pixels, path length 8 and roulette depth 2 as the other scene tests; one
Renderer per geometry level, cameras and guides switched on it, the sample cursor rewound before every step.

A. The inert ladder.  A visible scene of spheres and a disc (diffuse, mirror, glass, one emissive sphere) holds an opaque diffuse
   "vault" sphere that no ray starts inside.  The geometry levels above SPHERES append, as the last objects and strictly inside
   the vault, a diffuse triangle (POLY), a two-triangle mesh (MESH), with vertex normals (SMOOTH), with a 2 x 2 texture (TEX), and
   a black emissive triangle, which pt_set_light_guide_ex lists (the PLAMPS instances run) but which has no mass, so nothing is
   ever drawn from it.  No ray reaches them.  Every instance must then compute what the lowest instance with the same arithmetic
   computes: accumulators, pathLength and (paths, segments, escaped) of one step, the pt_trace_paths records over the same (u, v,
   sample), and the feature buffers, whose object_id never names a hidden object.

   Two rungs of that ladder cannot be taken with their weight at zero, BY DESIGN, and the tests below state both as facts:
   * pt_set_light_guide(0) launches no emitter-guided instance (ptmi_context.h, fill_light_params: beta = 0 leaves lights.n at 0,
     "the other instances' arithmetic exactly"), so the LIGHT_GUIDE and LIGHT_GUIDE_PLAMPS instances run here with beta = 0.5.
     Their weight divides by a mixture density, which no other instance forms, so they are compared with the nearest level that
     shares that code: (camera, LIGHT_GUIDE, SPHERES) of the visible scene -- the hidden polygon lamp and the geometry levels
     are still inert.  PLAIN and ENV_GUIDE (alpha = 0) are compared with (camera, PLAIN, SPHERES).
   * The default pose given explicitly is recognised as the identity and launches the BUILTIN instances (fill_trace_params), so
     the POSE instances run under a pure translation by T, whose components and all the scene's coordinates are multiples of
     1 / 64, over the scene moved by T: the camera-space table R^T (c - T) is then the built-in camera's table exactly, and the
     POSE runs are compared with the BUILTIN runs as the BUILTIN ones are.  LENS is a thin lens under a moved pose and is
     compared with its own (LENS, ., SPHERES).

B. The live matrix.  One scene per geometry level with the level's feature in view (a parallelogram lamp and a triangle; an
   icosphere over a grid floor; the icosphere glass with vertex normals; the floor under an 8 x 8 texture), all emitters
   untextured and of one colour c, the guides live (alpha = 0.5 over a one-bright-texel sky, beta = 0.5 with and without
   polygons, and once per level both guides together), the cameras built-in, moved and moved with a lens.  For each of the 57
   triples every pixel's accumulator equals, as binary32 bits, the reconstruction from that pixel's pt_trace_paths record: env x
   throughput where it escaped, c x throughput where it ended on an emitter (the single product shade_hit forms), 0 where it died.

The pt_trace_paths records are the kernel's own twin, not an independent model: the float64 models of tests/scene_*_model.py and
tests/light_guide*_model.py check those records feature by feature, and extending them to the combinations is out of scope here.
All comparisons are exact; the liveness counts are conditions, not measurements."""
import numpy as np
import pytest

from tests import mesh_normals_fixtures as NF
from tests import mesh_texture_fixtures as F
from tests import scene_mesh_model as MM
from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 64, 48
ENV = (0.75, 1.5, 3.0)
LAMP = (6.0, 4.5, 3.0)            # c: the one emission colour of a scene
BETA = 0.5

BUILTIN, POSE, LENS = 0, 1, 2
PLAIN, ENV_GUIDE, LIGHT_GUIDE, PLAMPS = 0, 1, 2, 3
SPHERES, POLY, MESH, SMOOTH, TEX = 0, 1, 2, 3, 4
CAMERA_NAMES = ("BUILTIN", "POSE", "LENS")
BOUNCE_NAMES = ("PLAIN", "ENV_GUIDE", "LIGHT_GUIDE", "LIGHT_GUIDE_PLAMPS")
GEOMETRY_NAMES = ("SPHERES", "POLY", "MESH", "SMOOTH", "TEX")
# The dense numbering as ptmi_trace_variant.h states it in words -- geometry major, then bounce, then camera, the pair
# (LIGHT_GUIDE_PLAMPS, SPHERES) left out -- written as an enumeration, not with the header's formula.
PAIRS = [(b, g) for g in range(5) for b in range(4) if not (b == PLAMPS and g == SPHERES)]
TRIPLES = [(c, b, g) for b, g in PAIRS for c in range(3)]
INDEX = {t: i for i, t in enumerate(TRIPLES)}
PATHS_INDEX = {p: i for i, p in enumerate(PAIRS)}
assert len(TRIPLES) == 57 and len(PAIRS) == 19


def _id(t):
    return "%s-%s-%s" % (CAMERA_NAMES[t[0]], BOUNCE_NAMES[t[1]], GEOMETRY_NAMES[t[2]])


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _sky():
    sky = np.full((16, 32, 3), 0.1, F32)
    sky[3, 5] = 50.0
    return sky


def _renderer(P):
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE, sample_precision=P.SAMPLES_FLOAT)
    r.set_constant_env(ENV)
    r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
    return r


def _rewind(r):
    """The sample cursor back to 0: a new seed resets it."""
    r.init_render_settings(seed=PM.SEED + 1, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
    r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)


def _set_bounce(r, bounce, alpha, beta=BETA):
    r.set_light_guide(None)
    r.set_env_guide(None)
    if bounce == ENV_GUIDE:
        r.set_env_guide(_sky(), rows=8, cols=16, alpha=alpha)
    elif bounce >= LIGHT_GUIDE:
        r.set_light_guide(beta, polygons=bounce == PLAMPS)


def _run(P, r):
    """One step from sample 0 and the records of its paths, with what pt_get_trace_variant said before and after."""
    _rewind(r)
    before = r.trace_variant()
    rec = P.worklist(W, H)
    r.setup(rec)
    r.path_trace()
    st = r.read_results(rec)
    paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
    return {"rec": rec, "stats": (st.paths, st.segments, st.escaped), "first_sample": st.first_sample, "trace_launches": st.trace_launches,
            "paths": paths, "before": before, "after": r.trace_variant()}


def _assert_reported(run, triple):
    """The launch took exactly this instance: the coordinates, the dense index of each family and the counts."""
    c, b, g = triple
    t, p = run["after"]["trace"], run["after"]["paths"]
    assert (t["camera"], t["bounce"], t["geometry"], t["index"]) == (c, b, g, INDEX[triple]), (t, _id(triple))
    assert (p["camera"], p["bounce"], p["geometry"], p["index"]) == (c, b, g, PATHS_INDEX[(b, g)]), (p, _id(triple))
    assert run["trace_launches"] >= 1 and run["first_sample"] == 0
    assert t["launches"] == run["before"]["trace"]["launches"] + run["trace_launches"]
    assert p["launches"] == run["before"]["paths"]["launches"] + 1


def _rgb(rec):
    return np.stack([rec["r"], rec["g"], rec["b"]], -1)


# ---- A. the inert ladder

T = (0.25, -0.125, 0.5)                                   # the POSE rung: a pure translation, multiples of 1 / 64
VAULT = (-27 / 64, 22 / 64, -53 / 64)
VISIBLE = [
    {"shape": "disc", "material": "diffuse", "centre": (1 / 64, -16 / 64, -48 / 64), "radius": 1.0, "normal": (1 / 16, 1.0, 1 / 8), "colour": (0.75, 0.75, 0.5)},
    {"shape": "sphere", "material": "diffuse", "centre": (-24 / 64, -2 / 64, -56 / 64), "radius": 12 / 64, "colour": (0.75, 0.5, 0.25)},
    {"shape": "sphere", "material": "specular", "centre": (22 / 64, -2 / 64, -50 / 64), "radius": 10 / 64, "colour": (1.0, 1.0, 1.0)},
    {"shape": "sphere", "material": "refractive", "centre": (2 / 64, -7 / 64, -35 / 64), "radius": 7 / 64, "colour": (0.875, 1.0, 0.875)},
    {"shape": "sphere", "material": "emissive", "centre": (4 / 64, 30 / 64, -46 / 64), "radius": 8 / 64, "colour": LAMP},
    {"shape": "sphere", "material": "diffuse", "centre": VAULT, "radius": 9 / 64, "colour": (0.5, 0.625, 0.75)}]
VAULT_INDEX, LAMP_INDEX = 5, 4
LADDER_CAMERAS = {BUILTIN: None, POSE: dict(position=T, look_at=(T[0], T[1], T[2] - 1.0), up=(0.0, 1.0, 0.0)), LENS: PM.CAMERAS["lens_moved"]}


def _in_vault(offsets):
    """Points at the vault's centre plus offsets given in units of 1 / 64, all of them well inside its radius of 9 / 64."""
    o = np.asarray(offsets, np.float64) / 64.0
    assert np.linalg.norm(o, axis=-1).max() < 5 / 64
    return F32(np.asarray(VAULT) + o)


HIDDEN_TRIANGLE = {"shape": "triangle", "material": "diffuse", "colour": (0.5, 0.5, 0.5), "vertices": _in_vault([(-3, -2, 1), (3, -1, -1), (1, 3, 2)])}
HIDDEN_LAMP = {"shape": "triangle", "material": "emissive", "colour": (0.0, 0.0, 0.0), "vertices": _in_vault([(-1, 1, -3), (2, -1, -3), (1, 3, -2)])}
HIDDEN_MESH = {"shape": "mesh", "material": "diffuse", "colour": (0.5, 0.75, 0.5), "vertices": _in_vault([(-2, -2, -1), (2, -2, 1), (2, 2, -1), (-2, 2, 2)]),
               "triangles": np.uint32([(0, 1, 2), (0, 2, 3)])}
HIDDEN_NORMALS = F32([(0.1, 0.2, 1.0), (-0.2, 0.1, 1.0), (0.3, -0.1, 1.0), (0.0, 0.25, 1.0)])
HIDDEN_IMAGE = F32(np.arange(1, 13).reshape(2, 2, 3) / 8.0)
HIDDEN_UVS = F32([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])


def _moved(o, t):
    o = dict(o)
    for key in ("centre", "vertices"):
        if key in o:
            was = np.asarray(o[key], F32)
            o[key] = F32(was + F32(t))
            assert np.array_equal(o[key].astype(np.float64) - np.asarray(t), was.astype(np.float64))   # exact: back by subtraction
    return o


def _ladder_scene(g, shifted=False):
    """The visible scene and, from POLY on, the level's hidden objects as the last ones; shifted: everything moved by T."""
    scene = [dict(o) for o in VISIBLE]
    if g == POLY:
        scene.append(dict(HIDDEN_TRIANGLE))
    if g >= MESH:
        m = dict(HIDDEN_MESH)
        if g >= SMOOTH:
            m["normals"] = HIDDEN_NORMALS
        if g == TEX:
            m.update(texture=HIDDEN_IMAGE, uvs=HIDDEN_UVS, texture_filter="nearest", texture_wrap="repeat")
        scene.append(m)
    if g >= POLY:
        scene.append(dict(HIDDEN_LAMP))
    return [_moved(o, T) for o in scene] if shifted else scene


@pytest.fixture(scope="module")
def ladder(ptmi_lib):
    """Every run of A: runs[(camera, bounce, geometry)], features[(camera, geometry)], lights[...] (the emitter table in force)."""
    P = ptmi_lib
    out = {"runs": {}, "features": {}, "lights": {}, "first": None}
    for g in range(5):
        r = _renderer(P)
        try:
            if g == 0:
                out["first"] = r.trace_variant()                        # before any launch
            for c in range(3):
                r.set_scene(_ladder_scene(g, shifted=c == POSE))
                r.set_camera(None) if LADDER_CAMERAS[c] is None else r.set_camera(**LADDER_CAMERAS[c])
                _set_bounce(r, PLAIN, alpha=0.0)
                before = r.trace_variant()["features"]
                out["features"][(c, g)] = (r.feature_buffers(), before, r.trace_variant()["features"])
                for b in range(4):
                    if (b, g) not in PATHS_INDEX:
                        continue
                    _set_bounce(r, b, alpha=0.0)
                    if b >= LIGHT_GUIDE:
                        out["lights"][(c, b, g)] = r.light_guide_info()
                    out["runs"][(c, b, g)] = _run(P, r)
        finally:
            r.close()
    return out


def test_nothing_is_reported_before_a_launch(ladder):
    never = {"camera": -1, "bounce": -1, "geometry": -1, "index": -1, "launches": 0}
    assert ladder["first"] == {"trace": never, "paths": never, "features": never}


def test_a_light_guide_at_zero_and_the_default_pose_launch_the_lower_instances(ptmi_lib):
    """The two rungs that are not there by design (module docstring): beta = 0 is the PLAIN (or ENV_GUIDE) instance, the identity
    pose the BUILTIN one -- which is why A takes them with beta = 0.5 and a translation."""
    P = ptmi_lib
    r = _renderer(P)
    try:
        r.set_scene(_ladder_scene(POLY))
        r.set_camera(position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
        for polygons in (False, True):
            r.set_light_guide(0.0, polygons=polygons)
            assert r.light_guide_info()["set"]
            _assert_reported(_run(P, r), (BUILTIN, PLAIN, POLY))
        r.set_env_guide(_sky(), rows=8, cols=16, alpha=0.0)
        _assert_reported(_run(P, r), (BUILTIN, ENV_GUIDE, POLY))
    finally:
        r.close()


@pytest.mark.parametrize("triple", TRIPLES, ids=_id)
def test_inert_ladder(ladder, triple):
    c, b, g = triple
    run = ladder["runs"][triple]
    _assert_reported(run, triple)
    rung = LIGHT_GUIDE if b >= LIGHT_GUIDE else PLAIN                   # the lowest bounce with this arithmetic
    base = ladder["runs"][(LENS if c == LENS else BUILTIN, rung, SPHERES)]
    assert run["rec"].tobytes() == base["rec"].tobytes(), "accumulators / pathLength of %s differ from %s" % (_id(triple), _id((LENS if c == LENS else BUILTIN, rung, SPHERES)))
    assert run["stats"] == base["stats"]
    twin = ladder["runs"][(c, rung, SPHERES)]                           # the records: across the instances of one camera
    assert run["paths"].tobytes() == twin["paths"].tobytes()
    assert np.array_equal(run["rec"]["pathLength"], run["paths"]["length"])
    if b >= LIGHT_GUIDE:
        info = ladder["lights"][triple]
        assert info["active"] and info["beta"] == BETA
        if b == PLAMPS:     # the table lists the hidden polygon, with no mass: the sphere is drawn every time
            assert info["object_index"].tolist() == [LAMP_INDEX, len(_ladder_scene(g)) - 1] and info["probability"].tolist() == [1.0, 0.0]
        else:
            assert info["object_index"].tolist() == [LAMP_INDEX]


@pytest.mark.parametrize("camera", range(3), ids=CAMERA_NAMES)
def test_inert_ladder_is_not_vacuous(ladder, camera):
    """The yardsticks see every material, the vault and the lamp, and the live emitter guide is another image."""
    plain, guided = ladder["runs"][(camera, PLAIN, SPHERES)], ladder["runs"][(camera, LIGHT_GUIDE, SPHERES)]
    for run in (plain, guided):
        p = run["paths"]
        assert np.count_nonzero(p["escaped"] == 1) >= 100 and np.count_nonzero(p["escaped"] == 2) >= 20 and p["length"].max() >= 4
    assert plain["rec"].tobytes() != guided["rec"].tobytes() and plain["paths"].tobytes() != guided["paths"].tobytes()
    ids = ladder["features"][(camera, SPHERES)][0]["object_id"]
    assert all(np.count_nonzero(ids == k) >= 20 for k in range(len(VISIBLE))), np.bincount(ids[ids >= 0].ravel(), minlength=len(VISIBLE))


@pytest.mark.parametrize("geometry", range(5), ids=GEOMETRY_NAMES)
@pytest.mark.parametrize("camera", range(3), ids=CAMERA_NAMES)
def test_inert_ladder_features(ladder, camera, geometry):
    feats, before, after = ladder["features"][(camera, geometry)]
    assert (after["geometry"], after["index"], after["bounce"]) == (geometry, geometry, PLAIN) and after["launches"] == before["launches"] + 1
    assert after["camera"] == (BUILTIN if camera == BUILTIN else POSE)          # the feature kernels trace through a pinhole
    base = ladder["features"][(camera, SPHERES)][0]
    assert all(feats[k].tobytes() == base[k].tobytes() for k in base)
    assert feats["object_id"].max() < len(VISIBLE) and feats["object_id"].min() == -1      # never a hidden object
    if camera == POSE:      # the translation: the built-in camera's first hits
        other = ladder["features"][(BUILTIN, SPHERES)][0]
        assert feats["object_id"].tobytes() == other["object_id"].tobytes() and feats["depth"].tobytes() == other["depth"].tobytes()


def test_every_instance_was_launched_and_reported(ladder):
    """The coverage fact: all 57 trace, 19 trace-paths and 5 feature instances ran, by the library's own report."""
    runs = ladder["runs"].values()
    assert sorted(run["after"]["trace"]["index"] for run in runs) == list(range(57))
    assert sorted({run["after"]["paths"]["index"] for run in runs}) == list(range(19))
    assert sorted({after["index"] for _, _, after in ladder["features"].values()}) == list(range(5))
    assert len({(run["after"]["trace"]["camera"], run["after"]["trace"]["bounce"], run["after"]["trace"]["geometry"]) for run in runs}) == 57


# ---- B. the live matrix

FLOOR_INDEX = 0
LIVE_CAMERAS = {BUILTIN: None, POSE: PM.CAMERAS["moved"], LENS: PM.CAMERAS["lens_moved"]}
BALL = {"shape": "sphere", "material": "diffuse", "centre": (-0.2, -0.05, -0.6), "radius": 0.07, "colour": (0.75, 0.5, 0.25)}
MIRROR = {"shape": "sphere", "material": "specular", "centre": (0.22, -0.05, -0.65), "radius": 0.07, "colour": (1.0, 1.0, 1.0)}
GLASS = {"shape": "sphere", "material": "refractive", "centre": (-0.08, -0.08, -0.38), "radius": 0.05, "colour": (0.9, 1.0, 0.9)}
SPHERE_LAMP = {"shape": "sphere", "material": "emissive", "centre": (0.25, 0.22, -0.5), "radius": 0.1, "colour": LAMP}
POLY_LAMP = {"shape": "parallelogram", "material": "emissive", "colour": LAMP, "vertices": ((-0.08, 0.22, -0.62), (0.08, 0.23, -0.62), (-0.08, 0.2, -0.48))}
BACKDROP = {"shape": "triangle", "material": "diffuse", "colour": (0.5, 0.75, 0.75), "vertices": ((-0.35, -0.19, -0.8), (0.35, -0.19, -0.85), (0.0, 0.3, -0.9))}
DISC_FLOOR = {"shape": "disc", "material": "diffuse", "centre": (0.0, -0.19, -0.55), "radius": 0.5, "normal": (0.0, 1.0, 0.0), "colour": (0.8, 0.7, 0.5)}


def _live_scene(g):
    """Row 0 is the floor (a disc, from MESH on the grid mesh, at TEX textured); the sphere lamp is in every scene (pt_set_light_guide
    draws from spheres and discs alone), the parallelogram lamp from POLY on."""
    if g <= POLY:
        scene = [DISC_FLOOR, BALL, MIRROR, GLASS, SPHERE_LAMP]
        return [dict(o) for o in scene + ([POLY_LAMP, BACKDROP] if g == POLY else [])]
    fv, ft = MM.height_field(*NF.FIELD)
    floor = {"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": F32(fv), "triangles": ft}
    sv, st, sn = NF.sphere_mesh()
    ico = {"shape": "mesh", "material": "diffuse", "colour": (0.5, 0.6, 0.9), "vertices": sv, "triangles": st}
    if g >= SMOOTH:
        ico.update(material="refractive", colour=(0.9, 0.95, 1.0), normals=sn)
    if g == TEX:
        image = F32(0.25 + np.random.default_rng(8).random((8, 8, 3)))
        floor.update(texture=image, uvs=F.planar_uvs(fv, -0.7, 1.6), texture_filter="bilinear", texture_wrap="repeat")
    return [floor, ico] + [dict(o) for o in (BALL, MIRROR, GLASS, SPHERE_LAMP, POLY_LAMP, BACKDROP)]


@pytest.fixture(scope="module")
def matrix(ptmi_lib):
    """Every run of B: runs[(camera, bounce, geometry)], both[geometry] (the two guides together, moved pose), features, lights."""
    P = ptmi_lib
    out = {"runs": {}, "both": {}, "features": {}, "lights": {}}
    for g in range(5):
        r = _renderer(P)
        try:
            r.set_scene(_live_scene(g))
            for c in range(3):
                r.set_camera(None) if LIVE_CAMERAS[c] is None else r.set_camera(**LIVE_CAMERAS[c])
                _set_bounce(r, PLAIN, alpha=0.0)
                out["features"][(c, g)] = r.feature_buffers()
                for b in range(4):
                    if (b, g) not in PATHS_INDEX:
                        continue
                    _set_bounce(r, b, alpha=0.5)
                    if b >= LIGHT_GUIDE:
                        out["lights"][(c, b, g)] = r.light_guide_info()
                    out["runs"][(c, b, g)] = _run(P, r)
                if c == POSE:     # both guides: the emitter-guided instance takes its environment branch, rotated into the camera's frame
                    b = PLAMPS if g >= POLY else LIGHT_GUIDE
                    r.set_light_guide(None)
                    r.set_env_guide(_sky(), rows=8, cols=16, alpha=0.45)
                    r.set_light_guide(0.45, polygons=b == PLAMPS)
                    out["both"][g] = (b, _run(P, r))
        finally:
            r.close()
    return out


def _assert_twin(run, lamp_in_view=True):
    """The accumulators are the reconstruction from the step's own path records, bit for bit; and the run is live."""
    rec, p = run["rec"], run["paths"]
    assert np.array_equal(rec["pathLength"], p["length"])
    assert run["stats"] == (W * H, int(p["length"].sum()), np.count_nonzero(p["escaped"] == 1))
    want = np.zeros((len(p), 3), F32)
    esc, em = p["escaped"] == 1, p["escaped"] == 2
    want[esc] = F32(ENV)[None, :] * p["throughput"][esc]
    want[em] = F32(LAMP)[None, :] * p["throughput"][em]
    wrong = (_bits(_rgb(rec)) != _bits(want)).any(axis=1)
    print("escaped %d, on an emitter %d, died %d, longest %d; %d accumulators differ from their record" % (
        esc.sum(), em.sum(), len(p) - esc.sum() - em.sum(), p["length"].max(), wrong.sum()))
    assert not wrong.any(), np.flatnonzero(wrong)[:8]
    assert set(np.unique(p["escaped"]).tolist()) <= {0, 1, 2}
    assert esc.sum() >= 100 and p["length"].max() >= 4
    if lamp_in_view:
        assert em.sum() >= 20


@pytest.mark.parametrize("triple", TRIPLES, ids=_id)
def test_live_matrix(matrix, triple):
    c, b, g = triple
    run = matrix["runs"][triple]
    _assert_reported(run, triple)
    _assert_twin(run)
    if b != PLAIN:      # the guide is live: another image than the unguided run of the same scene and camera
        plain = matrix["runs"][(c, PLAIN, g)]
        assert run["rec"].tobytes() != plain["rec"].tobytes() and run["paths"].tobytes() != plain["paths"].tobytes()
    if b >= LIGHT_GUIDE:
        info, scene = matrix["lights"][triple], _live_scene(g)
        assert info["active"] and info["beta"] == BETA and np.all(info["probability"] > 0)
        shapes = [scene[k]["shape"] for k in info["object_index"]]
        assert shapes == (["sphere", "parallelogram"] if b == PLAMPS else ["sphere"])
    ids = matrix["features"][(c, g)]["object_id"]
    assert np.count_nonzero(ids == FLOOR_INDEX) >= 100                  # at TEX: first hits on the textured mesh
    if g >= MESH:
        assert np.count_nonzero(ids == 1) >= 20                         # the icosphere
    if g >= POLY:
        assert np.count_nonzero(ids == len(_live_scene(g)) - 1) >= 20   # the triangle behind, the last row


@pytest.mark.parametrize("geometry", range(5), ids=GEOMETRY_NAMES)
def test_live_matrix_with_both_guides(matrix, geometry):
    b, run = matrix["both"][geometry]
    _assert_reported(run, (POSE, b, geometry))
    _assert_twin(run)
    for other in (PLAIN, ENV_GUIDE, b):
        assert run["rec"].tobytes() != matrix["runs"][(POSE, other, geometry)]["rec"].tobytes()


def test_the_texture_and_the_normals_are_live(matrix):
    """The levels' own code changes the image: TEX against SMOOTH (the same scene without the texture), SMOOTH against MESH."""
    for c in range(3):
        tex, smooth, mesh = (matrix["runs"][(c, PLAIN, g)] for g in (TEX, SMOOTH, MESH))
        assert tex["rec"].tobytes() != smooth["rec"].tobytes() and smooth["rec"].tobytes() != mesh["rec"].tobytes()
        albedo = [matrix["features"][(c, g)]["albedo"] for g in (TEX, SMOOTH)]
        floor = matrix["features"][(c, TEX)]["object_id"] == FLOOR_INDEX
        assert np.count_nonzero((_bits(albedo[0][floor]) != _bits(albedo[1][floor])).any(axis=1)) > 0.9 * floor.sum()
