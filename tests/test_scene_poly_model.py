"""The float64 polygon model (tests/scene_poly_model.py) on the CPU: it is scene_model on spheres and discs, its intersection
gives the known answers, the mutations a polygon tracer can get wrong fail the GPU test's comparison rule, and the GPU cases'
own inputs leave at most the project's cap of fragile paths."""
import numpy as np
import pytest

from tests import scene_model as M
from tests import scene_poly_model as PM


def _cam(u, v, w, h, seed=3):
    """Half-exact camera rays near the pixel centres (the model takes them as an input; the GPU tests take the library's)."""
    rng = np.random.default_rng(seed)
    c = u + rng.normal(0, 0.3, len(u))
    r = v + rng.normal(0, 0.3, len(u))
    return np.stack([(2.0 * c - w) / w, -((2.0 * r - h) / h) * (h / w)], -1).astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("scene", ["crowd", "inside", "single_specular_disc", "single_refractive_sphere"])
@pytest.mark.parametrize("camera", ["none", "lens_moved"])
def test_model_equals_scene_model_on_spheres_and_discs(ptmi_lib, scene, camera):
    u, v = M.all_pixels()
    u, v = u[::3], v[::3]
    ss = np.full(len(u), 5, np.uint32)
    cam = _cam(u, v, M.W, M.H)
    objs = M.world_scene(scene, camera)
    old, new = M.stored_scene(objs), PM.stored_scene_ex(objs)
    assert not new["vertex"].any() and all(np.array_equal(old[k], new[k]) for k in old.dtype.names)
    opt = M.case_options(scene == "crowd")
    a = M.analyse(old, M.CAMERAS[camera], opt, u, v, ss, cam, M.ENV)
    b = PM.analyse(new, M.CAMERAS[camera], opt, u, v, ss, cam, M.ENV)
    for key in a[0]:                                        # the plain run: float64 equality, every output
        assert np.array_equal(a[0][key], b[0][key]), key
    assert np.array_equal(a[1], b[1])                       # ... and the perturbed runs draw the same numbers
    for key in a[2]:
        assert np.array_equal(a[2][key], b[2][key]), key


V0, V1, V2 = np.array([1.0, 0.5, -3.0]), np.array([3.0, 0.75, -3.5]), np.array([1.5, 2.5, -2.75])
E1, E2 = V1 - V0, V2 - V0


def _hit(shape, a, b, origin=(0.2, 0.1, 0.3), flip=False, **kw):
    """Shoot from `origin` (or from the other side of the plane) at the point v0 + a e1 + b e2."""
    o = np.array(origin, np.float64)
    if flip:
        o = V0 + 2 * E1 + 2 * E2 + (V0 + 2 * E1 + 2 * E2 - o)      # behind the plane (the origin reflected through a far point)
    target = V0 + a * E1 + b * E2
    d = target - o
    dist = np.linalg.norm(d)
    t = PM.poly_hit(shape, V0, E1, E2, o[None], (d / dist)[None], **kw)[0]
    return t, dist


def test_known_answers_of_the_intersection():
    T, P = PM.TRIANGLE, PM.PARALLELOGRAM
    for shape in (T, P):
        t, dist = _hit(shape, 1 / 3, 1 / 3)                        # the centroid
        assert abs(t - dist) < 1e-12
        for a, b, inside in ((1e-6, 0.4, True), (-1e-6, 0.4, False),          # the edge a = 0
                             (0.4, 1e-6, True), (0.4, -1e-6, False)):         # the edge b = 0
            t, dist = _hit(shape, a, b)
            assert (abs(t - dist) < 1e-12) if inside else t == 0.0, (shape, a, b)
    for a, b, inside in ((0.5 - 1e-6, 0.5, True), (0.5 + 1e-6, 0.5, False)):   # the triangle's third edge a + b = 1
        t, dist = _hit(T, a, b)
        assert (abs(t - dist) < 1e-12) if inside else t == 0.0
    for a, b, inside in ((1 - 1e-6, 0.5, True), (1 + 1e-6, 0.5, False), (0.5, 1 - 1e-6, True), (0.5, 1 + 1e-6, False)):
        t, dist = _hit(P, a, b)                                    # the parallelogram's far edges a = 1 and b = 1
        assert (abs(t - dist) < 1e-12) if inside else t == 0.0
    t, dist = _hit(P, 0.7, 0.8)                                    # the far half: a parallelogram's, not the triangle's
    assert abs(t - dist) < 1e-12 and _hit(T, 0.7, 0.8)[0] == 0.0
    t, dist = _hit(P, 0.999999, 0.999999)                          # up to the fourth corner v1 + v2 - v0
    assert abs(t - dist) < 1e-12
    for shape in (T, P):                                           # the back face: two-sided, the same distance rule
        t, dist = _hit(shape, 0.3, 0.3, flip=True)
        assert abs(t - dist) < 1e-12
    # a ray in the plane: det == 0 exactly, a miss whatever a and b would be
    o = (V0 + 0.3 * E1 + 0.3 * E2 - 2 * E1)[None]
    for shape in (T, P):
        assert PM.poly_hit(shape, V0, E1, E2, o, (E1 / np.linalg.norm(E1))[None])[0] == 0.0
    ex, ez = np.array([2.0, 0.0, 0.0]), np.array([0.0, 0.0, -2.0])     # ... and with exact arithmetic: an axis-aligned floor
    assert PM.poly_hit(P, np.zeros(3), ex, ez, np.array([[-1.0, 0.0, -1.0]]), np.array([[1.0, 0.0, 0.0]]))[0] == 0.0
    # a hit closer than eps is a miss, one just beyond it a hit
    n = np.cross(E1, E2) / np.linalg.norm(np.cross(E1, E2))
    target = V0 + 0.3 * E1 + 0.3 * E2
    for shape in (T, P):
        assert PM.poly_hit(shape, V0, E1, E2, (target + 0.5e-5 * n)[None], (-n)[None])[0] == 0.0
        assert abs(PM.poly_hit(shape, V0, E1, E2, (target + 2e-5 * n)[None], (-n)[None])[0] - 2e-5) < 1e-12
        assert PM.poly_hit(shape, V0, E1, E2, (target - 1.0 * n)[None], (-n)[None])[0] == 0.0       # behind the ray


def test_nearest_takes_polygons_in_declaration_order():
    far = dict(shape=PM.PARALLELOGRAM, material=0, vertices=((-1, -1, -3), (1, -1, -3), (-1, 1, -3)))
    near = dict(shape=PM.TRIANGLE, material=0, vertices=((-1, -1, -2), (3, -1, -2), (-1, 3, -2)))
    same = dict(shape=PM.PARALLELOGRAM, material=0, vertices=((-1, -1, -2), (1, -1, -2), (-1, 1, -2)))
    o, d = np.zeros((1, 3)), np.array([[0.0, 0.0, -1.0]])
    best, t = PM._nearest(PM.stored_scene_ex([far, near, same]), o, d, None)
    assert best[0] == 1 and t[0] == 2.0                            # the nearer one, and of an exact tie the earlier
    best, t = PM._nearest(PM.stored_scene_ex([far, M._sph((0, 0, -2.5), 0.25, 0)]), o, d, None)
    assert best[0] == 1 and t[0] == 2.25


# The mutations run over the cases' own scenes and pixels; each must break the rule the GPU test applies to the kernels.
_MUTATION_CASES = {"no_normal_flip": ("mixed32", "none"), "no_sum_test": ("cornell", "none"), "swap_edges_in_t": ("triangle", "none"),
                   "no_eps": ("cornell", "moved")}


@pytest.mark.parametrize("mutation", PM.MUTATIONS)
def test_mutations_fail_the_comparison_rule(ptmi_lib, mutation):
    scene_name, camera = _MUTATION_CASES[mutation]
    u, v = PM.all_pixels()
    ss = np.full(len(u), 7, np.uint32)
    cam = _cam(u, v, PM.W, PM.H)
    scene = PM.stored_scene_ex(PM.world_scene(scene_name, camera))
    opt = PM.case_options(True)
    plain, fragile, spread = PM.analyse(scene, PM.CAMERAS[camera], opt, u, v, ss, cam, PM.ENV)
    same, ratio = PM.compare(plain, plain, fragile, spread)
    assert same and ratio == 0.0                                   # the rule accepts the model itself
    wrong = PM.trace(scene, PM.CAMERAS[camera], opt, u, v, ss, cam, PM.ENV, mutation=mutation)
    same, ratio = PM.compare(wrong, plain, fragile, spread)
    print("%s on %s / %s: outcomes equal %s, ratio %.3g (allowed %.3f)" % (mutation, scene_name, camera, same, ratio, M.GPU_FACTOR))
    assert not (same and ratio <= M.GPU_FACTOR)


@pytest.mark.parametrize("scene,camera,half", PM.CASES_B, ids=["%s-%s-%s" % (s, c, "half" if h else "float") for s, c, h in PM.CASES_B])
def test_fragile_share_of_the_gpu_cases(oracle, ptmi_lib, scene, camera, half):
    """Test B's own inputs: the model alone keeps the share of paths it cannot vouch for under the project's cap, and the cases
    are not vacuous."""
    uu, vv, ss, cam, plain, fragile, spread = PM.case_b(scene, camera, half)
    print("%s / %s: fragile %.2f %% of %d paths" % (scene, camera, 100 * fragile.mean(), len(uu)))
    assert fragile.mean() <= M.FRAGILE_CAP
    hit = set(np.unique(plain["hits"]).tolist()) - {-1}
    if scene == "cornell":
        assert hit == set(range(11)) and set(np.unique(plain["escaped"]).tolist()) == {0, 1, 2} and plain["length"].max() == PM.DEPTH
        assert np.any(plain["choice"] >= PM.FLIPPED)               # a polygon is met from behind somewhere along a path
    elif scene == "mixed32":
        assert len(hit) >= 24 and {0, 2, 6, 31} <= hit and set(np.unique(plain["escaped"]).tolist()) == {0, 1, 2}
        first = plain["hits"][:, 0]
        assert np.any((first == 2) & (plain["choice"][:, 0] >= PM.FLIPPED))     # the polygon the camera sees from behind
    else:
        assert hit == {0} and np.count_nonzero(plain["hits"][:, 0] == 0) > 300 and np.count_nonzero(plain["hits"][:, 0] < 0) > 300
