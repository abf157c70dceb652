"""The float64 model of mesh scenes with textures (tests/scene_mesh_texture_model.py) on the CPU: without textures it is
scene_mesh_normals_model's model exactly, perturbed runs included; with them the throughput differs; the cases used on the device
leave at most the project's cap of fragile paths; and a lookup that leaves the texture out, does not turn t upside down, or exchanges
s and t fails the comparison."""
import numpy as np
import pytest

from tests import mesh_texture_fixtures as F
from tests import scene_mesh_model as MM
from tests import scene_mesh_normals_model as NM
from tests import scene_mesh_texture_model as TM
from tests import scene_model as M
from tests import scene_poly_model as PM


def _inputs():
    u, v = MM.pixels()
    return u, v, np.full(len(u), TM.SAMPLE, np.uint32), PM.oracle_cam(TM.SAMPLE)[::TM.STRIDE]


def test_without_textures_the_model_is_scene_mesh_normals_models(oracle):
    u, v, ss, cam = _inputs()
    for camera, material, odd in (("lens_moved", "refractive", True), ("none", "diffuse", False)):
        objs = TM.world_scene(camera, material, odd, textures=False)
        scene, opt = MM.stored(objs), PM.case_options(True)
        normals, textures = NM.corner_normals(objs), TM.corner_uvs(objs)
        assert normals[0].any() and not textures[0].any() and textures[0].shape == (450,) and textures[3] == []
        for seed in (None, 3):
            rng = (lambda: None) if seed is None else (lambda: np.random.default_rng(seed))
            want = NM.trace(scene, normals, PM.CAMERAS[camera], opt, u, v, ss, cam, PM.ENV, rng=rng())
            got = TM.trace(scene, normals, textures, PM.CAMERAS[camera], opt, u, v, ss, cam, PM.ENV, rng=rng())
            assert all(np.array_equal(got[k], want[k]) for k in want)


def test_corner_uvs_follow_the_indices_and_no_camera_moves_them():
    objs = TM.world_scene("moved", "diffuse", True)
    textured, uv, image, images = TM.corner_uvs(objs)
    assert textured.tolist() == [True] * 320 + [False] + [True] * 128 + [False]
    assert image.tolist() == [0] * 320 + [-1] + [1] * 128 + [-1] and [w for _, w in images] == [TM.REPEAT, TM.CLAMP]
    ball = objs[0]
    assert np.array_equal(uv[:320], np.asarray(ball["uvs"], np.float64)[ball["uv_indices"]])
    assert np.count_nonzero(ball["uv_indices"] >= len(ball["vertices"])) > 100           # the shifted half: a seam
    assert uv[:320].max() > 1.5 and uv[321:449].min() < -0.4 and uv[321:449].max() > 1.4   # the wraps decide
    other = TM.world_scene("none", "diffuse", True)
    assert all(np.array_equal(a["uvs"], b["uvs"]) for a, b in zip((objs[0], objs[2]), (other[0], other[2])))
    plainball = TM.world_scene("moved", "diffuse", False)[0]
    assert np.array_equal(TM.corner_uvs([plainball])[1], np.asarray(plainball["uvs"], np.float64)[plainball["triangles"]])


def test_the_bilinear_lookup_in_float64():
    """Texel centres return their texel; (0, 0) is the bottom-left corner; the wraps; a constant image."""
    img = F.image_5x3().astype(np.float64)
    s, t = (np.arange(5) + 0.5) / 5, 1.0 - (np.arange(3) + 0.5) / 3
    for wrap in (TM.REPEAT, TM.CLAMP):
        for r in range(3):
            assert np.allclose(TM.bilinear(img, wrap, s, np.full(5, t[r])), img[r], rtol=0, atol=1e-12)
        assert np.allclose(TM.bilinear(np.full((2, 3, 3), 0.25), wrap, np.array([-3.3, 0.2, 7.9]), np.array([0.4, -1.1, 2.5])), 0.25)
    assert np.allclose(TM.bilinear(img, TM.CLAMP, np.array([-2.0, 9.0]), np.array([-2.0, 9.0])), [img[2, 0], img[0, 4]])
    assert np.allclose(TM.bilinear(img, TM.REPEAT, np.array([0.0, 1.0, 2.3]), np.array([0.5, 0.5, 1.5])),
                       [(img[1, 4] + img[1, 0]) / 2] * 2 + [TM.bilinear(img, TM.REPEAT, np.array([0.3]), np.array([0.5]))[0]])


@pytest.mark.parametrize("camera,half,material,odd", TM.CASES)
def test_fragile_share_of_the_device_cases_stays_under_the_cap(oracle, camera, half, material, odd):
    u, v, ss, cam, plain, fragile, spread = TM.case(camera, half, material, odd)
    print("%s / %s / %s%s: %d paths, fragile %.2f %%" % (camera, "half" if half else "float", material, " / odd" if odd else "", len(u), 100 * fragile.mean()))
    assert len(u) == 1024 and fragile.mean() <= M.FRAGILE_CAP
    same, ratio = PM.compare(plain, plain, fragile, spread)
    assert same and ratio == 0.0
    assert set(np.unique(plain["escaped"]).tolist()) == {0, 1, 2} and plain["length"].max() >= 4
    # the texture changes no decision of a path, and it does change what the paths carry
    objs = TM.world_scene(camera, material, odd, textures=False)
    bare = NM.trace(MM.stored(objs), NM.corner_normals(objs), PM.CAMERAS[camera], PM.case_options(half), u, v, ss, cam, PM.ENV)
    assert all(np.array_equal(bare[k], plain[k]) for k in ("length", "escaped", "hits", "choice", "dir"))
    changed = np.any(np.abs(bare["throughput"] - plain["throughput"]) > 1e-3, axis=1)
    assert changed.mean() > 0.2


def test_the_comparison_notices_a_wrong_lookup(oracle):
    """Each mutation, taken for the device's result, fails the rule in EVERY case: the texture left out, t not turned upside down,
    s and t exchanged."""
    inputs = {}
    for mutation in TM.MUTATIONS:
        caught = []
        for camera, half, material, odd in TM.CASES:
            u, v, ss, cam, plain, fragile, spread = TM.case(camera, half, material, odd)
            key = (camera, material, odd)
            if key not in inputs:
                objs = TM.world_scene(camera, material, odd)
                inputs[key] = (MM.stored(objs), NM.corner_normals(objs), TM.corner_uvs(objs))
            got = TM.trace(*inputs[key], PM.CAMERAS[camera], PM.case_options(half), u, v, ss, cam, PM.ENV, mutation=mutation)
            same, ratio = PM.compare(got, plain, fragile, spread)
            caught.append(not same or ratio > M.GPU_FACTOR)
        print("%s: caught in %d of %d cases" % (mutation, sum(caught), len(caught)))
        assert all(caught)


def test_glass_is_tinted_on_a_refracted_ray_only(oracle):
    """Where the texel multiplies inside a path: a glass ball's texel reaches the throughput of a path whose ray was refracted there
    and of no path that was only mirrored by it (choice 3 against 4)."""
    camera, half, material, odd = [c for c in TM.CASES if c[2] == "refractive"][0]
    u, v, ss, cam, plain, fragile, spread = TM.case(camera, half, material, odd)
    objs = TM.world_scene(camera, material, odd)
    for o in (objs[2],):                                             # the field plain: only the ball's texture is left
        for key in ("texture", "uvs", "texture_filter", "texture_wrap"):
            o.pop(key)
    args = (PM.CAMERAS[camera], PM.case_options(half), u, v, ss, cam, PM.ENV)
    with_ball = TM.trace(MM.stored(objs), NM.corner_normals(objs), TM.corner_uvs(objs), *args)
    bare_objs = TM.world_scene(camera, material, odd, textures=False)
    bare = NM.trace(MM.stored(bare_objs), NM.corner_normals(bare_objs), *args)
    on_ball = (with_ball["hits"] >= 0) & (with_ball["hits"] < 320)
    refracted = np.any(on_ball & ((with_ball["choice"] & 7) == 3), axis=1)
    mirrored_only = np.any(on_ball, axis=1) & ~refracted
    live = with_ball["escaped"] != 0
    differs = np.any(with_ball["throughput"] != bare["throughput"], axis=1)
    assert (refracted & live).sum() > 20 and (mirrored_only & live).sum() > 5
    assert differs[refracted & live].all() and not differs[mirrored_only & live].any()
