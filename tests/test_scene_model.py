"""The float64 path model of tests/scene_model.py on the CPU: its Philox against the oracle's, its calibration against the oracle on
the built-in scene (the ratio R the GPU tolerance is made of), the cap on fragile paths over the very cases the GPU test uses,
closed-form known answers of the model itself, and mutations of the model that the tolerance must still tell apart."""
import numpy as np
import pytest

from ipu_path_trace_amd import ptmi
from tests import scene_model as M


def _central(n=1):
    """Inputs of n paths whose camera ray is the view axis."""
    z = np.zeros(n, np.uint16)
    return z, z, np.arange(n, dtype=np.uint32), np.zeros((n, 2), np.float32)


def test_philox_equals_the_oracle(oracle):
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64)
    ctr[0], key[0] = 0, 0
    ctr[1], key[1] = 0xFFFFFFFF, 0xFFFFFFFF
    for c, k in zip(ctr, key):
        got = M.philox(c[0], c[1], c[2], c[3], k[0], k[1])
        assert [int(x) for x in got] == [int(x) for x in oracle.philox(c, k)]
    # ... and vectorised with one key, as the model calls it
    got = np.stack(M.philox(ctr[:, 0], ctr[:, 1], ctr[:, 2], 0x5054, 9, 5), -1)
    for c, g in zip(ctr[:50], got[:50]):
        assert [int(x) for x in g] == [int(x) for x in oracle.philox([c[0], c[1], c[2], 0x5054], [9, 5])]


# ---- calibration on the built-in scene: the oracle is the binary32 statement the GPU matches bit for bit there

CALIBRATION = {"depth4_half": dict(max_path_length=4, samples_half=True),
               "depth8_float_roulette1": dict(max_path_length=8, samples_half=False, roulette_depth=1),
               "depth8_ri1.33": dict(max_path_length=8, refractive_index=1.33)}


@pytest.mark.parametrize("name", list(CALIBRATION))
def test_model_against_the_oracle_on_the_builtin_scene(oracle, name):
    O = oracle
    kw = dict(roulette_depth=3, refractive_index=1.5, samples_half=True, seed=77)
    kw.update(CALIBRATION[name])
    W, H, n = 200, 150, 4096
    rng = np.random.default_rng(2024)
    u = rng.integers(0, W, n).astype(np.uint16)
    v = rng.integers(0, H, n).astype(np.uint16)
    s = rng.integers(0, 100000, n).astype(np.uint32)
    cfg = O.make_config(width=W, height=H, max_path_length=kw["max_path_length"], roulette_depth=kw["roulette_depth"],
                        refractive_index=kw["refractive_index"], seed=kw["seed"],
                        sample_precision=O.SAMPLES_HALF if kw["samples_half"] else O.SAMPLES_FLOAT)
    ref = [O.trace_path(cfg, int(a), int(b), int(c)) for a, b, c in zip(u, v, s)]
    got = {k: np.array([list(getattr(p, k)) for p in ref], dtype=np.float32) for k in ("dir", "uv", "throughput", "cam")}
    got["length"] = np.array([p.length for p in ref], np.uint32)
    got["escaped"] = np.array([p.escaped for p in ref], np.uint32)
    plain, fragile, spread = M.analyse(ptmi.builtin_scene(), None, M.options(**kw), u, v, s, got["cam"])
    same, ratio = M.compare(got, plain, fragile, spread)
    print("calibration %s: fragile %.2f %%, largest ratio %.3f (R = %.3f)" % (name, 100 * fragile.mean(), ratio, M.R))
    assert fragile.mean() <= M.FRAGILE_CAP
    assert same                                     # length and escaped agree exactly on every non-fragile path
    assert ratio <= M.R
    assert got["length"].max() >= 4 and np.count_nonzero(got["escaped"] == 0) > 50 and np.count_nonzero(got["escaped"] == 1) > 1000


# ---- the cap on what may be left out, over the GPU test's own cases

@pytest.mark.parametrize("scene,camera,half", M.CASES_B, ids=["%s-%s-%s" % (s, c, "half" if h else "float") for s, c, h in M.CASES_B])
def test_fragile_share_of_the_gpu_cases(oracle, scene, camera, half):
    uu, vv, ss, cam, plain, fragile, spread = M.case_b(scene, camera, half)
    print("%s / %s: fragile %.2f %%" % (scene, camera, 100 * fragile.mean()))
    assert fragile.mean() <= M.FRAGILE_CAP
    outcomes, length = M.EXPECT[scene]
    assert set(np.unique(plain["escaped"]).tolist()) == outcomes
    assert plain["length"].max() >= length
    # the model against itself is inside the tolerance by construction
    assert M.compare(plain, plain, fragile, spread) == (True, 0.0)


def test_crowd_reaches_its_objects(oracle):
    """Object 31 is nearest for a region of pixels, object 0 the farthest; at least 20 objects are first hits under every camera."""
    scene = M.SCENES["crowd"]
    depth = [-o["centre"][2] - (o["radius"] if o["shape"] == M.SPHERE else 0.0) for o in scene]
    assert max(depth) == depth[0] and min(depth) == depth[31]
    assert scene[0]["shape"] == M.DISC and scene[1]["shape"] == M.SPHERE
    assert sum(1 for o in scene if o["material"] == M.EMISSIVE) == 3
    assert len({o["colour"] for o in scene if o["material"] == M.EMISSIVE}) == 1
    assert any(o["shape"] == M.DISC and o["normal"][2] < 0 for o in scene)                      # faces away from the camera
    for cam in M.CAMERAS:
        first = M.case_b("crowd", cam, M.CASES_B[[c[:2] for c in M.CASES_B].index(("crowd", cam))][2])[4]["hits"][:, 0]
        seen = set(np.unique(first).tolist()) - {-1}
        assert len(seen) >= 20 and {0, 31} <= seen, (cam, sorted(seen))
        assert np.count_nonzero(first == 31) > 50
        assert 20 not in seen                        # object 20 ties object 1 exactly everywhere: the earlier one wins


# ---- closed-form known answers of the model itself

GLASS = (0.9, 0.8, 0.7)


def test_central_ray_through_a_glass_sphere():
    scene = M.stored_scene([M._sph((0.0, 0.0, -4.0), 1.0, M.REFRACTIVE, GLASS)])
    u, v, s, cam = _central(400)
    p = M.trace(scene, None, M.options(roulette_depth=8), u, v, s, cam)
    through = np.all(p["choice"][:, :2] == 3, axis=1) & (p["length"] == 3)       # refracted in and out, then the environment
    assert np.count_nonzero(through) > 300                                      # (normal incidence: 4 % reflect per face)
    assert np.max(np.abs(p["dir"][through] - (0, 0, -1))) < 1e-12
    np.testing.assert_allclose(p["throughput"][through], np.tile(1.15 ** 2 * scene[0]["colour"].astype(np.float64) ** 2, (through.sum(), 1)), rtol=1e-12)
    mirrored = p["choice"][:, 0] == 4                                           # the other branch of the first face: no tint
    assert mirrored.any() and np.all(p["length"][mirrored] == 2)
    np.testing.assert_allclose(p["throughput"][mirrored], 1.15, rtol=1e-12)
    assert np.max(np.abs(p["dir"][mirrored] - (0, 0, 1))) < 1e-12


def test_off_axis_ray_follows_snell_twice():
    """A ray at impact parameter b on a sphere of radius r and index n is turned by 2 (i - t) towards the axis, sin i = b / r,
    sin t = sin i / n."""
    n_glass = float(np.float16(1.5))
    c, rad = np.array([0.0, 0.0, -5.0]), 1.0
    scene = M.stored_scene([M._sph(tuple(c), rad, M.REFRACTIVE, GLASS)])
    camx = np.float32(np.float16(0.125))
    cam = np.tile(np.float32([camx, 0.0]), (400, 1))
    u, v, s, _ = _central(400)
    p = M.trace(scene, None, M.options(roulette_depth=8), u, v, s, cam)
    through = np.all(p["choice"][:, :2] == 3, axis=1) & (p["length"] == 3)
    assert np.count_nonzero(through) > 250
    d = np.array([float(camx), 0.0, -1.0])
    d /= np.linalg.norm(d)
    b = np.linalg.norm(np.cross(c, d))
    i = np.arcsin(b / rad)
    t = np.arcsin(np.sin(i) / n_glass)
    # the ray d = (sin phi, 0, -cos phi) passes the centre on its +x side, so the sphere turns it towards -x: phi - 2 (i - t)
    phi = np.arctan2(d[0], -d[2]) - 2 * (i - t)
    want = np.array([np.sin(phi), 0.0, -np.cos(phi)])
    assert np.max(np.abs(p["dir"][through] - want)) < 1e-12


def test_disc_seen_from_behind_reflects_about_minus_n():
    nrm = np.array([0.3, -0.2, -1.0])                       # faces away from a camera that looks along -z
    scene = M.stored_scene([M._dsc((0.0, 0.0, -3.0), tuple(nrm), 2.0, M.SPECULAR)])
    u, v, s, _ = _central(1)
    cam = np.float32([[0.25, -0.125]])
    p = M.trace(scene, None, M.options(), u, v, s, cam)
    d = np.array([0.25, -0.125, -1.0])
    d /= np.linalg.norm(d)
    n32 = scene[0]["normal"].astype(np.float64)
    assert d @ n32 > 0
    want = d - 2 * (d @ -n32) * -n32                       # (the stored normal is unit to binary32 only: the result is normalised)
    want /= np.linalg.norm(want)
    assert p["hits"][0, 0] == 0 and p["length"][0] == 2 and p["escaped"][0] == 1
    assert np.max(np.abs(p["dir"][0] - want)) < 1e-12 and p["dir"][0, 2] > 0


def test_ray_from_inside_a_diffuse_shell_hits_the_far_root():
    """The camera is inside a diffuse sphere: the axis meets it at its far root, z = -sqrt(9 - 0.25), the bounce is about the
    outward normal (nothing flips a diffuse normal), so the next segment leaves the sphere and ends on the emitting shell."""
    scene = M.stored_scene([M._sph((0.5, 0.0, 0.0), 3.0, M.DIFFUSE, (0.5, 0.5, 0.5)), M._sph((0.0, 0.0, 0.0), 50.0, M.EMISSIVE, (1, 1, 1))])
    u, v, s, cam = _central(64)
    p = M.trace(scene, None, M.options(max_path_length=4), u, v, s, cam)
    assert np.all(p["hits"][:, 0] == 0) and np.all(p["hits"][:, 1] == 1) and np.all(p["length"] == 2) and np.all(p["escaped"] == 2)
    assert np.all(M.trace(scene, None, M.options(max_path_length=4), u, v, s, cam, rng=np.random.default_rng(1))["hits"][:, 0] == 0)
    best, t = M._nearest(scene, np.zeros((1, 3)), np.array([[0.0, 0.0, -1.0]]), None)
    assert best[0] == 0 and abs(t[0] - np.sqrt(3.0 ** 2 - 0.5 ** 2)) < 1e-12
    best, t = M._nearest(scene, np.zeros((1, 3)), np.array([[0.0, 0.0, -1.0]]), "no_far_root")
    assert best[0] == -1                                       # (the shell is met at its far root too)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_nearer_of_two_overlapping_spheres_wins_whatever_the_order(order):
    objs = [M._sph((0.0, 0.0, -4.0), 1.0, M.DIFFUSE, (0.2, 0.3, 0.4)), M._sph((0.3, 0.0, -3.4), 1.0, M.DIFFUSE, (0.9, 0.8, 0.7))]
    scene = M.stored_scene([objs[k] for k in order])
    u, v, s, cam = _central(8)
    p = M.trace(scene, None, M.options(), u, v, s, cam)
    assert np.all(p["hits"][:, 0] == order.index(1))        # the sphere whose surface is at z = -2.446..., not the one at z = -3
    # ... and an exact tie goes to the earlier one
    tie = M.stored_scene([objs[0], dict(objs[0], colour=(1, 1, 1))])
    assert np.all(M.trace(tie, None, M.options(), u, v, s, cam)["hits"][:, 0] == 0)


def test_roulette_survival_fraction():
    scene = M.stored_scene([M._sph((0.0, 0.0, 0.0), 10.0, M.SPECULAR)])      # a mirror shell: every path lives until roulette ends it
    n = 20000
    z = np.zeros(n, np.uint16)
    s = np.arange(n, dtype=np.uint32)
    p = M.trace(scene, None, M.options(max_path_length=3, roulette_depth=1, stop_prob=0.5, samples_half=False), z, z, s,
                np.zeros((n, 2), np.float32))
    survived = np.count_nonzero(p["length"] >= 2) / n         # length 1: stopped by the roulette of depth 1
    assert abs(survived - 0.5) < 5 * np.sqrt(0.25 / n), survived
    second = np.count_nonzero(p["hits"][:, 2] >= 0) / max(np.count_nonzero(p["length"] >= 2), 1)
    assert abs(second - 0.5) < 5 * np.sqrt(0.25 / (n / 2)), second


# ---- the tolerance still discriminates

MUTATION_CASES = {"skip_last": ("single_refractive_sphere", "none"), "prefer_later": ("crowd", "none"), "no_far_root": ("inside", "none"),
                  "one_sided_disc": ("crowd", "none"), "no_index_flip": ("inside", "none"), "tint_on_mirror": ("inside", "none")}


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_mutations_of_the_model_fail_at_the_gpu_tolerance(oracle, mutation):
    """Each mutation, run plainly, against the unmutated model at the factor 2 R the GPU test allows: at least one case fails."""
    assert set(MUTATION_CASES) == set(M.MUTATIONS)
    first = MUTATION_CASES[mutation]
    order = sorted(M.CASES_B, key=lambda c: c[:2] != first)          # the case expected to show it first, then all the others
    failed = None
    for scene, camera, half in order:
        uu, vv, ss, cam, plain, fragile, spread = M.case_b(scene, camera, half)
        stored = M.stored_scene(M.world_scene(scene, camera))
        mutant = M.trace(stored, M.CAMERAS[camera], M.case_options(half), uu, vv, ss, cam, M.ENV, mutation=mutation)
        same, ratio = M.compare(mutant, plain, fragile, spread)
        if not same or ratio > M.GPU_FACTOR:
            failed = (scene, camera, same, ratio)
            break
    print("mutation %s: %s" % (mutation, failed))
    assert failed is not None
