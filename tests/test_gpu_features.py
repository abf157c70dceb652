"""First-hit feature buffers (pt_feature_buffers) on the device; cases and yardsticks in tests/features_model.py.

1. object_id against the production trace kernels, exactly: every object made an emitter of radiance (i + 1, 0.5, 0.25) under the
   constant environment (0, 0.5, 0.25), aa_noise_scale 0, one sample -- each pixel's r names the object the trace kernel hit.
   The same ray and the same nearest_hit_primary: no tolerance, no excluded pixel.
2. depth and normal against the float64 model at four times what binary32 alone costs on these very cases
   (tests/features_model.py: `python -m tests.features_model` gave depth 9.82e-06 relative and normal 1.09e-04 per component, so
   DEPTH_TOL = 3.93e-05 and NORMAL_TOL = 4.36e-04), over the pixels whose index agrees and whose hit is not grazing
   (disc / b^2 >= 1e-4 for a sphere, |dot(n, d)| >= 1e-4 for a disc); at most 5 % of a case's hit pixels may be left out.
3. the cache follows pt_set_scene, pt_set_camera and the field of view, and is stable otherwise.
"""
import functools

import numpy as np
import pytest

from tests import features_model as FM
from tests import scene_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
_ID = ["%s-%s-%dx%d" % c for c in FM.CASES]


@functools.lru_cache(maxsize=None)
def _rays(W, H):
    return FM.camera_rays(W, H)


@functools.lru_cache(maxsize=None)
def _model(scene, camera, W, H):
    return FM.model64(FM.stored(scene, camera), FM.camera_of(scene, camera), _rays(W, H))


def _renderer(P, scene, camera, W, H, lens=False, recolour=False):
    r = P.Renderer(W, H, max_path_length=4, roulette_depth=2)
    r.set_constant_env((0.0, 0.5, 0.25))
    r.init_render_settings(seed=3, samples_per_step=1, aa_noise_scale=0.0, fov_degrees=FM.FOV_DEGREES)
    objs = FM.objects_of(scene, camera)
    if objs is not None:
        r.set_scene(objs)
    if recolour:
        t = r.scene()
        t["material"] = P.MATERIAL_EMISSIVE
        t["colour"] = np.stack([np.arange(len(t)) + 1.0, np.full(len(t), 0.5), np.full(len(t), 0.25)], -1)
        r.set_scene(t)
    pose = FM.camera_of(scene, camera)
    if pose is not None:
        r.set_camera(**dict(pose, **(FM.LENS if lens else {})))
    return r


@pytest.mark.parametrize("scene,camera,W,H", FM.CASES, ids=_ID)
def test_object_id_equals_the_production_kernels(ptmi_lib, scene, camera, W, H):
    P = ptmi_lib
    r = _renderer(P, scene, camera, W, H, recolour=True)
    try:
        rec = P.worklist(W, H)
        r.setup(rec)
        r.path_trace()                                   # the lens off
        r.read_results(rec)
        if camera == "posed_lens":
            r.set_camera(**dict(FM.camera_of(scene, camera), **FM.LENS))       # on the handle, and ignored by the features
        f = r.feature_buffers()
    finally:
        r.close()
    n = 6 if scene == "builtin" else 32
    assert np.all(rec["r"] == np.round(rec["r"])) and rec["r"].max() <= n
    traced = rec["r"].astype(np.int32).reshape(H, W) - 1               # env r = 0 -> -1
    assert np.array_equal(f["object_id"], traced)
    assert np.all(rec["g"] == F32(0.5)) and np.all(rec["b"] == F32(0.25))
    hit = np.unique(traced[traced >= 0])
    assert (traced < 0).sum() > 0.1 * W * H and len(hit) >= (4 if scene == "builtin" else 15)       # not vacuous
    assert np.all(f["albedo"] == 1)                                    # every object an emitter


@pytest.mark.parametrize("scene,camera,W,H", FM.CASES, ids=_ID)
def test_depth_normal_and_conventions_against_the_model(oracle, ptmi_lib, scene, camera, W, H):
    P = ptmi_lib
    ids, depth, nrm, ray, good = _model(scene, camera, W, H)
    r = _renderer(P, scene, camera, W, H, lens=camera == "posed_lens")
    try:
        stored = r.scene()
        u, v = FM.pixels(W, H)
        cam = r.trace_paths(u, v, np.zeros(len(u), np.uint32))["cam"]
        f = r.feature_buffers()
    finally:
        r.close()
    assert stored.tobytes() == FM.stored(scene, camera).tobytes() and np.array_equal(cam, _rays(W, H))     # the model's inputs
    gid, gd, gn, ga = f["object_id"].ravel(), f["depth"].ravel(), f["normal"].reshape(-1, 3), f["albedo"].reshape(-1, 3)
    dd, dn, excluded = FM.compare(gid, gd, gn, ids, depth, nrm, good)
    print("%s / %s / %d x %d: depth %.3g of %.3g, normal %.3g of %.3g, excluded %.3f, index mismatches %d" % (
        scene, camera, W, H, dd, FM.DEPTH_TOL, dn, FM.NORMAL_TOL, excluded, (gid != ids).sum()))
    assert excluded <= FM.EXCLUDED_CAP
    assert dd <= FM.DEPTH_TOL and dn <= FM.NORMAL_TOL
    # conventions: a miss is id -1, depth 0, normal 0, albedo 1; a hit has a unit normal that faces the ray
    miss = gid < 0
    assert miss.any() and np.all(gd[miss] == 0) and np.all(gn[miss] == 0) and np.all(ga[miss] == 1)
    hit = ~miss
    assert np.all(gd[hit] > 0)
    length = np.linalg.norm(gn[hit].astype(np.float64), axis=-1)
    assert np.max(np.abs(length - 1.0)) <= 4 * 2.0 ** -23
    facing = np.sum(gn[hit].astype(np.float64) * ray[hit], -1)
    print("largest dot(n, ray) %.3g" % facing.max())
    assert np.all(facing <= 0)
    # albedo: the colour of diffuse and refractive objects as B, G, R; 1 for mirrors and emitters
    mat, col = stored["material"][gid[hit]], stored["colour"][gid[hit]]
    tinted = (mat == P.MATERIAL_DIFFUSE) | (mat == P.MATERIAL_REFRACTIVE)
    assert tinted.any() and (~tinted).any()
    assert np.array_equal(ga[hit][tinted], col[tinted][:, ::-1]) and np.all(ga[hit][~tinted] == 1)


def test_the_cache_follows_scene_camera_and_fov(ptmi_lib):
    P = ptmi_lib
    W, H = 33, 17
    r = P.Renderer(W, H)
    try:
        with pytest.raises(P.PtError) as e:
            r.feature_buffers()
        assert e.value.code == -5                                      # PT_ERR_NOT_READY: no render settings yet
        r.init_render_settings(aa_noise_scale=0.3, fov_degrees=90.0)    # no worklist, no environment: not needed
        a = r.feature_buffers()
        b = r.feature_buffers()
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        r.init_render_settings(aa_noise_scale=0.0, fov_degrees=60.0)
        narrow = r.feature_buffers()
        assert (narrow["object_id"] >= 0).sum() > (a["object_id"] >= 0).sum()
        r.init_render_settings(aa_noise_scale=0.9, fov_degrees=90.0)    # the AA scale does not enter
        assert all(a[k].tobytes() == r.feature_buffers()[k].tobytes() for k in a)
        r.set_scene([M._sph((0.0, 0.0, -3.0), 1.0, M.DIFFUSE, (0.2, 0.4, 0.8))])
        one = r.feature_buffers()
        assert set(np.unique(one["object_id"])) == {-1, 0}
        centre = one["object_id"] == 0
        assert np.all(one["albedo"][centre] == F32([0.8, 0.4, 0.2]))
        r.set_camera(position=(0.0, 0.0, 6.0), look_at=(0.0, 0.0, -3.0))
        far = r.feature_buffers()
        assert 0 < (far["object_id"] == 0).sum() < centre.sum() and far["depth"].max() > 7.9
        assert far["depth"].tobytes() == r.feature_buffers()["depth"].tobytes()
        r.set_camera(None)
        r.set_scene(None)
        assert all(a[k].tobytes() == r.feature_buffers()[k].tobytes() for k in a)
    finally:
        r.close()
