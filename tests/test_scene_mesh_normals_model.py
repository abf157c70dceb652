"""The float64 model of mesh scenes with vertex normals (tests/scene_mesh_normals_model.py) on the CPU: without normals it is
scene_poly_model's model exactly, with them it differs and takes every rule, and the cases used on the device leave at most the
project's cap of fragile paths."""
import numpy as np
import pytest

from tests import scene_mesh_model as MM
from tests import scene_mesh_normals_model as NM
from tests import scene_model as M
from tests import scene_poly_model as PM


def _inputs():
    u, v = MM.pixels()
    return u, v, np.full(len(u), NM.SAMPLE, np.uint32), PM.oracle_cam(NM.SAMPLE)[::NM.STRIDE]


def test_without_normals_the_model_is_scene_poly_models(oracle):
    u, v, ss, cam = _inputs()
    objs = MM.world_scene("lens_moved")
    scene, opt = MM.stored(objs), PM.case_options(True)
    normals = NM.corner_normals(objs)
    assert not normals[0].any() and normals[0].shape == (450,)
    for seed in (None, 3):
        rng = (lambda: None) if seed is None else (lambda: np.random.default_rng(seed))
        want = PM.trace(scene, PM.CAMERAS["lens_moved"], opt, u, v, ss, cam, PM.ENV, rng=rng())
        got = NM.trace(scene, normals, PM.CAMERAS["lens_moved"], opt, u, v, ss, cam, PM.ENV, rng=rng())
        assert all(np.array_equal(got[k], want[k]) for k in want)


def test_corner_normals_are_unit_as_the_library_makes_them_and_follow_the_indices():
    objs = NM.world_scene("moved", "diffuse", True)
    smooth, corner = NM.corner_normals(objs)
    assert smooth.tolist() == [True] * 320 + [False] * 130
    ball = objs[0]
    n = NM.unit32(ball["normals"])
    assert n.dtype == np.float32 and np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0) < 2e-7)
    assert np.array_equal(corner[:320], n.astype(np.float64)[ball["normal_indices"]])
    assert np.count_nonzero(ball["normal_indices"] >= len(ball["vertices"])) > 100       # the creased half
    plainball = NM.world_scene("moved", "diffuse", False)[0]
    assert np.array_equal(NM.corner_normals([plainball])[1], NM.unit32(plainball["normals"]).astype(np.float64)[plainball["triangles"]])


@pytest.mark.parametrize("camera,half,material,odd", NM.CASES)
def test_fragile_share_of_the_device_cases_stays_under_the_cap(oracle, camera, half, material, odd):
    u, v, ss, cam, plain, fragile, spread = NM.case(camera, half, material, odd)
    flags = {name: int(np.count_nonzero(plain["choice"] & bit)) for name, bit in (("fallback", NM.FALLBACK), ("dropped", NM.DROPPED), ("guarded", NM.GUARDED))}
    print("%s / %s / %s%s: %d paths, fragile %.2f %%, bounces %s" % (camera, "half" if half else "float", material, " / odd" if odd else "",
                                                                    len(u), 100 * fragile.mean(), flags))
    assert len(u) == 1024 and fragile.mean() <= M.FRAGILE_CAP
    same, ratio = PM.compare(plain, plain, fragile, spread)
    assert same and ratio == 0.0
    assert set(np.unique(plain["escaped"]).tolist()) == {0, 1, 2} and plain["length"].max() >= 4
    # the normals matter to the model: the same scene flat gives other paths
    objs = NM.world_scene(camera, material, odd)
    flat = PM.trace(MM.stored(objs), PM.CAMERAS[camera], PM.case_options(half), u, v, ss, cam, PM.ENV)
    changed = np.any(np.abs(flat["dir"] - plain["dir"]) > 1e-3, axis=1) | (flat["length"] != plain["length"])
    assert changed.mean() > 0.05
    assert not PM.compare(flat, plain, fragile, spread)[0]                          # and the rule tells a flat render from a smooth one


def test_the_comparison_notices_a_rule_left_out(oracle):
    """Each mutation of the shading normal, taken for the device's result, fails the rule on a case that exercises it: a wrong
    orientation on reversed windings, a missing side test, a missing mirror guard."""
    inputs = {}
    for mutation in NM.MUTATIONS:
        caught = []
        for camera, half, material, odd in NM.CASES:
            u, v, ss, cam, plain, fragile, spread = NM.case(camera, half, material, odd)
            objs = NM.world_scene(camera, material, odd)
            key = (camera, material, odd)
            if key not in inputs:
                inputs[key] = (MM.stored(objs), NM.corner_normals(objs))
            got = NM.trace(*inputs[key], PM.CAMERAS[camera], PM.case_options(half), u, v, ss, cam, PM.ENV, mutation=mutation)
            same, ratio = PM.compare(got, plain, fragile, spread)
            caught.append(not same or ratio > M.GPU_FACTOR)
        print("%s: caught in %d of %d cases" % (mutation, sum(caught), len(caught)))
        assert any(caught)
        if mutation == "no_orientation":
            assert all(c for c, case in zip(caught, NM.CASES) if case[3])           # every case with reversed windings


def test_the_cases_take_every_rule(oracle):
    """Rule 4 (the side test) and rule 6 (the mirror's guard) are taken by well-conditioned paths of the cases, so the device is
    compared on them; rule 2's fallback needs dot(m, m) <= 1e-12, which no unit normals of a sphere give: tests/mesh_normals_main.cpp
    and pt_mesh_shade cover it."""
    dropped = guarded = 0
    for c in NM.CASES:
        plain, fragile = NM.case(*c)[4:6]
        dropped += np.count_nonzero(np.any(plain["choice"] & NM.DROPPED, axis=1) & ~fragile)
        guarded += np.count_nonzero(np.any(plain["choice"] & NM.GUARDED, axis=1) & ~fragile)
    print("well-conditioned paths with a dropped shading normal %d, with a guarded mirror vector %d" % (dropped, guarded))
    assert dropped > 0 and guarded > 0
