"""The runtime camera on the GPU (pt_set_camera): the default camera is today's bits, pose geometry through pt_trace_paths
against float64 numpy, a yaw against the matching azimuth, the rotation reaching the NIF, closed forms from a moved and rotated
camera, sharing and the memo under a camera, the thin lens (focal plane, defocus circle, lens samples, weight) and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
META = nif_assets.URBAN_ALLEY_META
L_SKY = (0.75, 1.5, 3.0)        # few mantissa bits: L x 1 and sums of powers of two of them are exact

MOVED = dict(position=(1.5, 0.7, 2.0), look_at=(0.2, -0.3, -3.0), up=(0.1, 1.0, 0.2))
ALONG_Y = dict(position=(0.5, -4.0, 0.3), look_at=(0.5, -1.0, 0.3), up=(0.0, 0.0, 1.0))   # looks along +y, z is up


def _set_camera(r, camera):
    if camera is None:
        return
    if camera == "null":
        r.set_camera(None)
    else:
        r.set_camera(**camera)


def _render(P, W, H, camera=None, scene=None, const=None, spp=4, steps=1, depth=8, roulette=3, precision=0, memo=0, mode="off",
            camera_after=None, seed=1, aa=0.3, before=None):
    """`steps` steps with the film resident; returns (records of the last step, film bytes, stats of every step).
    `before` is a camera set (and replaced) ahead of `camera`; `camera_after` replaces `camera` half way."""
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette, sample_precision=precision, iterations_per_batch=2)
    try:
        if const is not None:
            r.set_constant_env(const)
        else:
            r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
        r.init_render_settings(seed=seed, samples_per_step=spp, aa_noise_scale=aa)
        if scene is not None:
            r.set_scene(scene)
        _set_camera(r, before)
        _set_camera(r, camera)
        r.set_nif_sharing(mode)
        if memo:
            r.set_nif_memo(memo)
        rec = P.worklist(W, H)
        r.setup(rec)
        stats = []
        for s in range(steps):
            if camera_after is not None and s == steps // 2:
                _set_camera(r, camera_after)
            r.path_trace()
            stats.append(r.read_results(rec).as_dict())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)[0].copy()
        return rec, film, stats
    finally:
        r.close()


def _paths(P, W, H, camera=None, scene=None, const=L_SKY, n=4096, depth=8, roulette=8, seed=7, precision=0, aa=0.3, before=None,
           azimuth_degrees=0.0, pixels=None):
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette, sample_precision=precision)
    try:
        r.set_constant_env(const)
        r.init_render_settings(seed=3, samples_per_step=1, aa_noise_scale=aa, env_rotation_degrees=azimuth_degrees)
        if scene is not None:
            r.set_scene(scene)
        _set_camera(r, before)
        _set_camera(r, camera)
        if pixels is not None:
            u, v = pixels
            s = np.zeros(len(u), np.uint32)
        else:
            rng = np.random.default_rng(seed)
            u = rng.integers(0, W, n).astype(np.uint16)
            v = rng.integers(0, H, n).astype(np.uint16)
            s = rng.integers(0, 1000, n).astype(np.uint32)
        return r.trace_paths(u, v, s)
    finally:
        r.close()


def _sphere(centre, radius, material, colour=(1, 1, 1)):
    return {"shape": "sphere", "centre": tuple(float(x) for x in centre), "radius": radius, "material": material, "colour": colour}


def _basis(camera):
    """float64 frame of include/ptmi.h: f = normalise(look_at - position), r = normalise(cross(f, up)), u = cross(r, f)."""
    p = np.array(np.float32(camera["position"]), dtype=np.float64)
    f = np.array(np.float32(camera["look_at"]), dtype=np.float64) - p
    f /= np.linalg.norm(f)
    r = np.cross(f, np.array(np.float32(camera["up"]), dtype=np.float64))
    r /= np.linalg.norm(r)
    return p, r, np.cross(r, f), f


def _to_world(camera, d):
    """Camera-space (x, y, z) -> world x r + y u - z f."""
    _, r, u, f = _basis(camera)
    return d[..., 0:1] * r + d[..., 1:2] * u - d[..., 2:3] * f


def _to_camera(camera, d):
    _, r, u, f = _basis(camera)
    return np.stack([d @ r, d @ u, -(d @ f)], -1)


def _cam_dirs(p):
    d = np.stack([p["cam"][:, 0].astype(np.float64), p["cam"][:, 1].astype(np.float64), -np.ones(len(p))], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _pixel_dirs(W, H):
    """Camera-space directions through the pixel centres (fov 90: tan = 1), [H, W, 3]."""
    px = (2 * (np.arange(W) + 0.0) - W) / W
    py = -((2 * (np.arange(H) + 0.0) - H) / H) * (H / W)
    d = np.stack(np.broadcast_arrays(px[None, :], py[:, None], -np.ones((H, W))), -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _behind(camera, dist=5.0, radius=0.5):
    """A scene whose only object is behind the camera: every camera ray escapes."""
    p, _, _, f = _basis(camera)
    return [_sphere(p - dist * f, radius, "diffuse")]


DEFAULT = dict(position=(0, 0, 0), look_at=(0, 0, -1), up=(0, 1, 0))


# ---- 1. the default camera is today's bits

def test_default_camera_is_todays_bits(ptmi_lib):
    P = ptmi_lib
    variants = (dict(camera=DEFAULT), dict(before=MOVED, camera="null"), dict(camera=dict(lens_radius=0.0, focus_distance=7.25)),
                dict(camera=dict(position=(0, 0, 0), look_at=(0, 0, -5), up=(0, 3, 0))))   # the same frame from other values
    for kw in ({}, {"const": (0.6, 0.9, 1.3)}):
        rec0, film0, st0 = _render(P, 96, 72, spp=6, steps=2, **kw)
        for var in variants:
            rec1, film1, st1 = _render(P, 96, 72, spp=6, steps=2, **kw, **var)
            assert rec0.tobytes() == rec1.tobytes() and film0.tobytes() == film1.tobytes(), var
            for a, b in zip(st0, st1):
                assert (a["paths"], a["segments"], a["escaped"]) == (b["paths"], b["segments"], b["escaped"]), var
        _, film2, _ = _render(P, 96, 72, spp=6, steps=2, camera=MOVED, **kw)
        assert film2.tobytes() != film0.tobytes()                      # (a moved camera is another image)
    base = _paths(P, 96, 72, roulette=3).tobytes()
    for var in variants:
        assert _paths(P, 96, 72, roulette=3, **var).tobytes() == base, var
    assert _paths(P, 96, 72, roulette=3, camera=MOVED).tobytes() != base


def test_rejected_camera_leaves_the_previous_one(ptmi_lib):
    P = ptmi_lib
    r = P.Renderer(32, 32)
    try:
        assert r.camera().as_dict() == P.default_camera().as_dict()
        r.set_camera(lens_radius=0.125, focus_distance=3.0, **MOVED)
        moved = r.camera().as_dict()
        assert moved["lens_radius"] == 0.125 and moved["focus_distance"] == 3.0
        assert np.array_equal(np.float32(moved["position"]), np.float32(MOVED["position"]))
        bad = (("position", dict(position=(0, float("nan"), 0))),
               ("look_at", dict(position=(1, 2, 3), look_at=(1, 2, 3))),
               ("up", dict(up=(0, 0, 0))),
               ("up", dict(position=(0, 0, 0), look_at=(0, 0, -2), up=(0, 0, 5))),
               ("up", dict(position=(0, 0, 0), look_at=(0, 0, -1), up=(0, 5e-4, 1))),     # |cross| = 5e-4 < 1e-3
               ("lens_radius", dict(lens_radius=-0.5)),
               ("focus_distance", dict(lens_radius=0.5, focus_distance=0.0)),
               ("focus_distance", dict(lens_radius=0.5, focus_distance=float("inf"))))
        for field, kw in bad:
            with pytest.raises(P.PtError) as e:
                r.set_camera(**kw)
            assert e.value.code == -1 and "camera" in str(e.value) and field in str(e.value), (field, str(e.value))
            assert r.camera().as_dict() == moved
        wrong = P.make_camera()
        wrong.struct_size = 44
        with pytest.raises(P.PtError) as e:
            r.set_camera(wrong)
        assert e.value.code == -1 and "struct_size" in str(e.value)
        assert r.camera().as_dict() == moved
        r.set_camera(position=(0, 0, 0), look_at=(0, 0, -1), up=(0, 2e-3, 1))   # |cross| = 2e-3: accepted
        r.set_camera(None)
        assert r.camera().as_dict() == P.default_camera().as_dict()
    finally:
        r.close()
    # ... and the rejected one is not what renders
    W, H = 64, 48
    r = P.Renderer(W, H, roulette_depth=8)
    try:
        r.set_constant_env(L_SKY)
        r.init_render_settings(seed=3, samples_per_step=1)
        r.set_camera(**MOVED)
        with pytest.raises(P.PtError):
            r.set_camera(position=(9, 9, 9), look_at=(9, 9, 9))
        u, v = np.arange(256, dtype=np.uint16) % W, np.arange(256, dtype=np.uint16) % H
        got = r.trace_paths(u, v, np.zeros(256, np.uint32))
    finally:
        r.close()
    assert got.tobytes() == _paths(P, W, H, camera=MOVED, pixels=(u, v)).tobytes()


# ---- 2. pose geometry against float64 numpy

GEOMETRY_CAM_CENTRE, GEOMETRY_RADIUS = np.array([0.3, -0.2, 3.5]), 1.2   # the sphere in camera space: 0.3 r - 0.2 u + 3.5 f


def _world_sphere(camera):
    p, r, u, f = _basis(camera)
    c = p + GEOMETRY_CAM_CENTRE[0] * r + GEOMETRY_CAM_CENTRE[1] * u + GEOMETRY_CAM_CENTRE[2] * f
    return np.float32(c).astype(np.float64)   # what the library is given


def _classify(camera, d_world, c, rad):
    p = _basis(camera)[0]
    oc = c - p
    tc = d_world @ oc
    dist = np.sqrt(np.maximum(oc @ oc - tc * tc, 0))
    return tc, dist, (dist < rad) & (tc > 0), np.abs(dist - rad) > 1e-4


@pytest.mark.parametrize("camera", [MOVED, ALONG_Y], ids=["moved", "along_y_z_up"])
def test_pose_geometry_through_trace_paths(ptmi_lib, camera):
    P = ptmi_lib
    W, H = 200, 150
    c, rad = _world_sphere(camera), GEOMETRY_RADIUS
    pos = _basis(camera)[0]
    # the float64 computation alone, over the pixel centres: both sides well populated, few rays near the silhouette
    dw = _to_world(camera, _pixel_dirs(W, H).reshape(-1, 3))
    _, _, hit, keep = _classify(camera, dw, c, rad)
    assert np.count_nonzero(~keep) < 0.05 * len(keep)
    assert np.count_nonzero(hit & keep) > 200 and np.count_nonzero(~hit & keep) > 200
    if camera is ALONG_Y:
        assert np.allclose(_basis(camera)[3], (0, 1, 0)) and np.allclose(_basis(camera)[2], (0, 0, 1))

    p = _paths(P, W, H, camera=camera, scene=[_sphere(c, rad, "specular")])
    d = _to_world(camera, _cam_dirs(p))                       # R normalise(camx, camy, -1)
    tc, dist, hit, keep = _classify(camera, d, c, rad)
    assert np.count_nonzero(~keep) < 0.05 * len(keep)
    assert np.count_nonzero(hit & keep) > 200 and np.count_nonzero(~hit & keep) > 200
    assert np.array_equal((p["length"] >= 2)[keep], hit[keep])
    miss = ~hit & keep
    assert np.all(p["length"][miss] == 1) and np.all(p["escaped"][miss] == 1)
    assert np.max(np.abs(p["dir"][miss] - d[miss])) < 1e-5
    # uv is PreProcessEscapedRays of the world direction
    th, ph = np.arccos(d[miss][:, 1]), np.arctan2(d[miss][:, 2], d[miss][:, 0])
    ph = np.where(ph < 0, ph + 2 * np.pi, ph)
    assert np.max(np.abs(p["uv"][miss][:, 0] - th / np.pi)) < 1e-5
    dv = np.abs(p["uv"][miss][:, 1] - ph / (2 * np.pi))
    assert np.max(np.minimum(dv, 1 - dv)) < 1e-5
    # reflections away from grazing bounce once and escape, reflected about the world-space normal
    cos_in = np.sqrt(np.maximum(1 - (dist / rad) ** 2, 0))
    h = hit & (cos_in > 0.3)
    assert np.count_nonzero(h) > 200
    assert np.all(p["escaped"][h] == 1) and np.all(p["length"][h] == 2)
    t = tc[h] - np.sqrt(rad * rad - dist[h] ** 2)
    x = pos + d[h] * t[:, None]
    nrm = (x - c) / rad
    refl = d[h] - 2 * np.sum(d[h] * nrm, -1, keepdims=True) * nrm
    assert np.max(np.abs(p["dir"][h] - refl)) < 1e-5
    assert np.all(p["throughput"][h] == 1.0)
    # an emitter reports the world direction of the ray that hit it
    p = _paths(P, W, H, camera=camera, scene=[_sphere(c, rad, "emissive", (3, 3, 3))])
    d = _to_world(camera, _cam_dirs(p))
    _, _, hit, keep = _classify(camera, d, c, rad)
    assert np.array_equal((p["escaped"] == 2)[keep], hit[keep])
    assert np.max(np.abs(p["dir"][hit & keep] - d[hit & keep])) < 1e-5


# ---- 3. a yaw about +y is the azimuth

def _basis32(camera):
    """The library's frame in binary32, every intermediate rounded (csrc/ptmi_camera.h)."""
    f32 = np.float32

    def normalise(v):
        d = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
        return np.array([f32(x / np.sqrt(d)) for x in v], dtype=f32)

    def cross(a, b):
        return np.array([f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])),
                         f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))], dtype=f32)

    p, la, up = (np.array(camera[k], dtype=f32) for k in ("position", "look_at", "up"))
    f = normalise(la - p)
    r = normalise(cross(f, up))
    return r, cross(r, f), f


YAW_DEGREES = (90.0, 30.0, 45.0, 60.0, 120.0, 200.0, 300.0, 37.0, 73.0, 151.0, 233.0, 340.0)


def test_yaw_equals_azimuth(ptmi_lib):
    """dir_to_uv: phi = atan2(z, x) + azimuth.  A camera whose view direction is (sin a, 0, -cos a) adds a to the phi of every
    ray, which is what azimuth = a does to the default camera; theta = acos(y) is untouched.  u is bit-identical where the world
    y equals the camera y bit for bit, i.e. where the binary32 frame has r.y = f.y = 0 and u.y = 1 exactly (x * 0 + y * 1 - z * 0
    is y); where u.y rounds one or two ulps off 1, y moves by <= 3 * 2^-24 |y| and u = acos(y) / pi by < 1e-6 (|y| < 0.6 at
    fov 90).  Which yaws are exact is decided here on the CPU, from the frame alone."""
    P = ptmi_lib
    W, H = 128, 96
    far_up = [_sphere((0.0, 50.0, 0.0), 0.1, "diffuse")]          # out of every view: all rays are primary misses
    exact = []
    for deg in YAW_DEGREES:
        a = P.rotation_to_radians_f32(deg)
        cam = dict(position=(0, 0, 0), look_at=(np.sin(a), 0.0, -np.cos(a)), up=(0, 1, 0))
        r, u, f = _basis32(cam)
        assert r[1] == 0 and f[1] == 0 and abs(float(u[1]) - 1) <= 2.0 ** -22
        is_exact = bool(u[1] == np.float32(1))
        exact.append(is_exact)
        yawed = _paths(P, W, H, camera=cam, scene=far_up)
        rotated = _paths(P, W, H, scene=far_up, azimuth_degrees=deg)
        assert np.all(yawed["length"] == 1) and np.all(rotated["length"] == 1) and np.all(yawed["escaped"] == 1)
        assert np.array_equal(yawed["cam"], rotated["cam"])
        du = np.abs(yawed["uv"][:, 0].astype(np.float64) - rotated["uv"][:, 0])
        print("yaw %g: frame exact %s, max |du| %.3g" % (deg, is_exact, du.max()))
        if is_exact:
            assert np.array_equal(yawed["uv"][:, 0], rotated["uv"][:, 0]), deg
        assert du.max() < 1e-6, deg
        dv = np.abs(yawed["uv"][:, 1].astype(np.float64) - rotated["uv"][:, 1])
        assert np.max(np.minimum(dv, 1 - dv)) < 1e-5, deg
        assert np.max(np.abs(yawed["dir"][:, 1] - rotated["dir"][:, 1])) < 1e-6
    assert exact[0] and sum(exact[1:]) >= 3            # more than the right angle is compared bit for bit


# ---- 4. the rotation reaches the NIF

def test_rotation_reaches_the_nif(ptmi_lib):
    P = ptmi_lib
    W, H = 64, 48
    out = {}
    for name, camera in (("default", DEFAULT), ("moved", MOVED), ("along_y", ALONG_Y)):
        rec = P.worklist(W, H)                                   # fresh accumulators: one sample per pixel
        r = P.Renderer(W, H, max_path_length=6)
        try:
            r.init_nif_weights(nif_assets.synthetic_nif(), 12, META["max"], nif_assets.folded_mean())
            r.init_render_settings(seed=5, samples_per_step=1, aa_noise_scale=0.0)
            r.set_scene(_behind(camera))
            r.set_camera(**camera)
            r.setup(rec)
            r.path_trace()
            st = r.read_results(rec)
            assert st.escaped == st.paths == W * H
            p = r.trace_paths(rec["u"], rec["v"], np.full(W * H, st.first_sample, np.uint32))
            assert np.all(p["escaped"] == 1) and np.all(p["length"] == 1)
            bgr = r.nif_infer(p["uv"][:, 0], p["uv"][:, 1])
        finally:
            r.close()
        d = _to_world(camera, _cam_dirs(p))
        assert np.max(np.abs(p["dir"] - d)) < 1e-5
        for k, ch in enumerate("bgr"):
            np.testing.assert_allclose(rec[ch], bgr[:, k], rtol=2e-2, atol=1e-6)
        out[name] = np.stack([rec["r"], rec["g"], rec["b"]], -1).copy()
    assert not np.allclose(out["default"], out["moved"], rtol=0.1) and not np.allclose(out["moved"], out["along_y"], rtol=0.1)


# ---- 5. closed forms from a moved, rotated camera

def _silhouette_mask(camera, W, H, centre, radius, margin):
    """Pixels whose camera ray passes at least `margin` (radians, about) inside the sphere's silhouette."""
    c = np.arange(W) + 0.5
    r = np.arange(H) + 0.5
    px = (2 * c - W) / W
    py = -((2 * r - H) / H) * (H / W)
    d = np.stack(np.broadcast_arrays(px[None, :], py[:, None], -np.ones((H, W))), -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = _to_world(camera, d)
    oc = np.array(centre, dtype=np.float64) - _basis(camera)[0]
    ang = np.arccos(np.clip(d @ (oc / np.linalg.norm(oc)), -1, 1))
    return ang < np.arcsin(radius / np.linalg.norm(oc)) - margin


def test_mirror_that_fills_the_view_is_the_sky_exactly(ptmi_lib):
    P = ptmi_lib
    for camera in (MOVED, ALONG_Y):
        p, _, _, f = _basis(camera)
        scene = [_sphere(p + 3.0 * f, 2.5, "specular")]          # angular radius 56 degrees > the 51 of the image's corners
        rec, film, st = _render(P, 128, 96, camera=camera, scene=scene, const=L_SKY, spp=8, depth=6, roulette=6)
        assert np.all(film == np.float32([L_SKY[2], L_SKY[1], L_SKY[0]]))      # BGR
        assert np.all(rec["pathLength"] == 16)
        assert st[0]["escaped"] == st[0]["paths"] == 128 * 96 * 8 and st[0]["segments"] == 2 * st[0]["paths"]


@pytest.mark.parametrize("roulette", [8, 1])
def test_furnace_from_an_oblique_camera(ptmi_lib, roulette):
    """One diffuse sphere of colour c under a constant L: inside its silhouette E[cos theta] = 1/2, so the mean is c L / 2."""
    P = ptmi_lib
    W, H, spp = 128, 96, 64
    c, L = np.array([0.8, 0.5, 0.25]), 2.0
    centre = (0.0, 0.0, -3.0)
    camera = dict(position=(1.8, 1.2, -1.0), look_at=(0.1, -0.1, -3.0), up=(0.2, 1.0, 0.1))
    rec, film, st = _render(P, W, H, camera=camera, scene=[_sphere(centre, 1.0, "diffuse", tuple(c))], const=(L, L, L), spp=spp,
                            depth=8, roulette=roulette, precision=P.SAMPLES_FLOAT)
    mask = _silhouette_mask(camera, W, H, centre, 1.0, 0.03).reshape(-1)
    n = int(mask.sum()) * spp
    assert n > 40000
    mean = film[mask].astype(np.float64).mean(axis=0)[::-1]                # RGB
    stop = float(np.float16(0.3))
    second = 1.0 / 3.0 / (1.0 - stop) if roulette == 1 else 1.0 / 3.0   # E[(c L cos)^2 rr^2 ...] / (c L)^2
    sigma = c * L * np.sqrt((second - 0.25) / n)
    assert np.all(np.abs(mean - c * L / 2) < 5 * sigma), (mean, c * L / 2, sigma)
    outside = ~_silhouette_mask(camera, W, H, centre, 1.0, -0.05).reshape(-1)
    assert outside.sum() > 5000 and np.all(film[outside] == np.float32(L))


# ---- 6. sharing and the memo

def test_sharing_and_memo_under_a_camera(ptmi_lib):
    P = ptmi_lib
    camera = dict(position=(0.8, 0.4, 0.6), look_at=(0.0, -0.8, -4.0), up=(0.05, 1.0, 0.0))
    other = dict(position=(-0.6, 0.2, 0.3), look_at=(0.3, -0.9, -4.0), up=(0.0, 1.0, 0.1), lens_radius=0.05, focus_distance=4.0)
    for kw in (dict(camera=camera, spp=6, steps=2), dict(camera=camera, camera_after=other, spp=6, steps=4),
               dict(camera=other, camera_after="null", spp=6, steps=4)):
        _, off, st = _render(P, 128, 96, **kw)
        _, step, _ = _render(P, 128, 96, mode="step", **kw)
        _, batch, _ = _render(P, 128, 96, mode="batch", **kw)
        _, memo, _ = _render(P, 128, 96, memo=1 << 28, **kw)
        assert off.tobytes() == step.tobytes() == batch.tobytes() == memo.tobytes()
        assert all(s["escaped"] > 0 for s in st)
    _, plain, _ = _render(P, 128, 96, spp=6, steps=2)
    _, moved, _ = _render(P, 128, 96, camera=camera, spp=6, steps=2)
    assert plain.tobytes() != moved.tobytes()


# ---- 7. the thin lens

def _disc(centre, normal, radius, emission):
    return {"shape": "disc", "centre": tuple(float(x) for x in centre), "normal": tuple(float(x) for x in normal), "radius": radius,
            "material": "emissive", "emission": emission}


def _all_pixels(P, W, H):
    rec = P.worklist(W, H)
    return rec, rec["u"].copy(), rec["v"].copy()


def test_lens_disc_in_the_focal_plane_is_sharp(ptmi_lib):
    P = ptmi_lib
    W, H, spp = 128, 96, 8
    E = (4.0, 2.0, 1.0)
    F, a, rd = 4.0, 0.2, 1.5
    for pose in (DEFAULT, MOVED):
        p, _, _, f = _basis(pose)
        scene = [_disc(p + F * f, -f, rd, E)]
        kw = dict(scene=scene, const=(0, 0, 0), spp=spp, precision=P.SAMPLES_FLOAT)
        rec, lens, _ = _render(P, W, H, camera=dict(lens_radius=a, focus_distance=F, **pose), **kw)
        _, pin, _ = _render(P, W, H, camera=pose, **kw)
        # distance of the pixel's focus point from the disc's axis, in the focal plane; the margin is 4 pixels there (the AA
        # noise, sigma 0.3 pixels, stays below 2)
        px = (2 * (rec["u"] + 0.0) - W) / W
        py = -((2 * (rec["v"] + 0.0) - H) / H) * (H / W)
        rho = F * np.hypot(px, py)
        margin = 4 * (2.0 * F / W)
        inside, outside = rho < rd - margin, rho > rd + margin
        assert inside.sum() > 1000 and outside.sum() > 1000
        assert np.all(lens[inside] == np.float32(E[::-1])) and np.all(lens[outside] == 0)
        assert np.array_equal(lens[inside | outside], pin[inside | outside])
        # the lens sample has no say in the focal plane, but it has elsewhere: the same disc at 2 F is blurred
        _, far, _ = _render(P, W, H, camera=dict(lens_radius=a, focus_distance=F / 2, **pose), **kw)
        assert not np.array_equal(far, pin)


def _overlap(d, a, r):
    """Area of the intersection of a circle of radius a whose centre is d from the centre of a circle of radius r > a."""
    d = np.asarray(d, dtype=np.float64)
    out = np.where(d <= r - a, np.pi * a * a, 0.0)
    band = (d > r - a) & (d < r + a)
    x = d[band]
    t1 = a * a * np.arccos(np.clip((x * x + a * a - r * r) / (2 * x * a), -1, 1))
    t2 = r * r * np.arccos(np.clip((x * x + r * r - a * a) / (2 * x * r), -1, 1))
    t3 = 0.5 * np.sqrt(np.maximum((-x + a + r) * (x + a - r) * (x - a + r) * (x + a + r), 0))
    out[band] = t1 + t2 - t3
    return out


def test_lens_defocus_circle_on_a_disc_at_twice_the_focus_distance(ptmi_lib):
    """A ray from the lens point l through the focus point F (camx, camy, -1) meets the plane z = -2 F at 2 F (camx, camy) - l:
    a pixel sees the uniform circle of radius a about 2 F (camx, camy).  Every sample is E or 0, so a pixel's mean is k E / n."""
    P = ptmi_lib
    W, H, n = 96, 72, 256
    E = (4.0, 2.0, 1.0)
    F, a, rd = 2.0, 0.4, 1.2
    scene = [_disc((0, 0, -2 * F), (0, 0, 1), rd, E)]
    camera = dict(lens_radius=a, focus_distance=F)
    rec, film, st = _render(P, W, H, camera=camera, scene=scene, const=(0, 0, 0), spp=n, aa=0.0, precision=P.SAMPLES_FLOAT)
    cam = _paths(P, W, H, camera=camera, scene=scene, const=(0, 0, 0), aa=0.0, pixels=(rec["u"], rec["v"]))["cam"].astype(np.float64)
    d = 2 * F * np.hypot(cam[:, 0], cam[:, 1])
    tol = 1e-4
    inside, outside = d + a < rd - tol, d - a > rd + tol
    band = (d + a > rd + tol) & (d - a < rd - tol)
    assert inside.sum() > 200 and outside.sum() > 1000 and band.sum() > 300
    assert np.all(film[inside] == np.float32(E[::-1])) and np.all(film[outside] == 0)
    k = film[:, 2].astype(np.float64) / E[0] * n                    # samples that saw the disc (R channel)
    assert np.array_equal(k, np.round(k)) and np.array_equal(film[:, 0] * 4, film[:, 2]) and np.array_equal(film[:, 1] * 2, film[:, 2])
    p = _overlap(d[band], a, rd) / (np.pi * a * a)
    kb = k[band]
    assert np.any((kb > 0) & (kb < n))
    # the band as a whole, and in four classes of p: sum of independent binomials
    classes = [np.ones(len(p), bool)] + [(p >= lo) & (p < lo + 0.25) for lo in (0.0, 0.25, 0.5, 0.75)]
    for sel in classes:
        assert sel.sum() > 20
        mean, want = kb[sel].sum() / (n * sel.sum()), p[sel].mean()
        sigma = np.sqrt(np.sum(p[sel] * (1 - p[sel]) / n)) / sel.sum()
        print("defocus band: %d pixels, mean %.5f, overlap %.5f, sigma %.2g" % (sel.sum(), mean, want, sigma))
        assert abs(mean - want) < 5 * sigma, (mean, want, sigma)


def test_lens_samples_through_trace_paths(ptmi_lib):
    P = ptmi_lib
    W, H, n = 128, 96, 20000
    a, F = 0.3, 2.5
    for pose, precision in ((MOVED, P.SAMPLES_FLOAT), (DEFAULT, P.SAMPLES_FLOAT), (ALONG_Y, P.SAMPLES_HALF)):
        camera = dict(lens_radius=a, focus_distance=F, **pose)
        p = _paths(P, W, H, camera=camera, scene=_behind(pose), n=n, precision=precision)
        assert np.all(p["length"] == 1) and np.all(p["escaped"] == 1) and np.all(p["throughput"] == 1.0)
        d = _to_camera(pose, p["dir"].astype(np.float64))
        focus = F * np.stack([p["cam"][:, 0], p["cam"][:, 1], -np.ones(n)], -1).astype(np.float64)
        t = -F / d[:, 2]                                            # back along the ray to the lens plane z = 0
        lens = focus - d * t[:, None]
        assert np.max(np.abs(lens[:, 2])) < 1e-9
        rho2 = lens[:, 0] ** 2 + lens[:, 1] ** 2
        assert np.sqrt(rho2.max()) <= a * (1 + 1e-4)
        # uniform on the disc: E[rho^2] = a^2 / 2, Var[rho^2] = a^4 / 12; E[x] = E[y] = 0, Var[x] = a^2 / 4
        assert abs(rho2.mean() - a * a / 2) < 5 * a * a / np.sqrt(12 * n), (rho2.mean(), a * a / 2)
        assert abs(lens[:, 0].mean()) < 5 * a / 2 / np.sqrt(n) and abs(lens[:, 1].mean()) < 5 * a / 2 / np.sqrt(n)
        assert len(np.unique(np.round(lens[:, :2] / a, 3), axis=0)) > 0.9 * n   # (not a handful of points)
        # the same pixels and samples through the pinhole: the lens moves the ray, cam stays
        q = _paths(P, W, H, camera=pose, scene=_behind(pose), n=n, precision=precision)
        assert np.array_equal(q["cam"], p["cam"]) and not np.array_equal(q["dir"], p["dir"])


def test_lens_carries_no_weight(ptmi_lib):
    P = ptmi_lib
    for pose in (DEFAULT, MOVED):
        p, _, _, f = _basis(pose)
        scene = [_sphere(p + 3.0 * f, 2.5, "specular")]
        rec, film, st = _render(P, 128, 96, camera=dict(lens_radius=0.1, focus_distance=3.0, **pose), scene=scene, const=L_SKY,
                                spp=8, depth=6, roulette=6)
        assert np.all(film == np.float32([L_SKY[2], L_SKY[1], L_SKY[0]]))
        assert np.all(rec["pathLength"] == 16) and st[0]["escaped"] == st[0]["paths"]


# ---- 8. the CLI

def _read_exr(path, W, H):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=np.float32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert L.pth_read_exr(str(path).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    return film


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_cli_camera_writes_the_same_exr_as_the_api(ptmi_lib, tmp_path, lens):
    P = ptmi_lib
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    W, H, spp = 96, 64, 8
    objects = [{"shape": "sphere", "centre": [0, 0, -3], "radius": 1, "material": "diffuse", "colour": [1.6, 1.2, 0.8]},
               {"shape": "disc", "centre": [0, -1.6, -5], "normal": [0, 1, 0], "radius": 3.5, "material": "specular"},
               {"shape": "sphere", "centre": [2, 3, -4], "radius": 0.3, "material": "emissive", "emission": [8, 8, 8]},
               {"shape": "sphere", "centre": [-1.5, 0.5, -3], "radius": 0.5, "material": "refractive", "colour": [0.9, 0.9, 0.7]}]
    camera = {"position": [2.5, 1.0, 1.5], "look_at": [0, -0.5, -3.5], "up": [0.1, 1, 0]}
    if lens:
        camera.update({"lens_radius": 0.08, "focus_distance": 5.0})
    path = tmp_path / "scene.json"
    path.write_text(json.dumps({"objects": objects, "camera": camera}))
    r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in L_SKY), "--scene", str(path),
                        "-w", str(W), "-h", str(H), "-s", str(spp), "--samples-per-step", str(spp), "--max-path-length", "7",
                        "-o", str(tmp_path / "cam.png"), "--save-interval", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    exr = _read_exr(tmp_path / "cam.exr", W, H)
    scene = [dict(o, colour=o.get("colour", o.get("emission", (1, 1, 1)))) for o in objects]
    for o in scene:
        o.pop("emission", None)
    rec, film, _ = _render(P, W, H, camera=camera, scene=scene, const=L_SKY, spp=spp, depth=7, roulette=3)
    image = np.zeros((H, W, 3), dtype=np.float32)
    image[rec["v"], rec["u"]] = film
    assert np.array_equal(exr, image)
    _, plain, _ = _render(P, W, H, scene=scene, const=L_SKY, spp=spp, depth=7, roulette=3)
    assert not np.array_equal(plain, film)
