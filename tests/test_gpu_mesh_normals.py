"""Vertex normals of meshes (pt_set_mesh_normals) on the GPU.  Scenes are the fixtures of tests/mesh_normals_fixtures.py: two or three
meshes, one of them flat, so a smooth mesh's slots and normals do not start at 0.

1. pt_mesh_shade equals the CPU program tests/mesh_normals_main.cpp on its own rays, bit for bit, on every fixture.
2. Off means off: normals removed, a flat mesh beside a smooth one, a scene set again.
3. The production kernels' smooth instances equal pt_trace_paths bit for bit.
4. pt_trace_paths against the float64 model with the shading normal (tests/scene_mesh_normals_model.py): four cameras, both sample
   precisions, the smooth mesh glass, mirror and diffuse, at the project's rule 2 R (spread + 2e-6 scale), R = 0.68.
5. Feature buffers: the closed form normalise(hp - centre) on the radial icosphere within the bound calibrated on the CPU
   (tests/test_mesh_normals.py), continuity across interior edges; the same test fails on the flat mesh.
6. The guides.   7. The camera.   8. NIF sharing, the memo and the denoiser.
"""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import mesh_normals_fixtures as F
from tests import scene_mesh_normals_model as NM
from tests import scene_model as M
from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 64, 48
ENV = (0.75, 1.5, 3.0)
LAMP = (6.0, 4.5, 3.0)
CLOSE = 24.0         # degrees: the icosphere nearly fills the view, 28 pixels of radius
NARROW = 8.0         # degrees: the front cap of the icosphere alone, every pixel on it
ZOOM = 40.0          # degrees: the icosphere, a fifth of a unit across, covers a few hundred of the 64 x 48 pixels


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return F.build_program(tmp_path_factory.mktemp("mesh_normals_gpu"))


def _renderer(P, scene, camera="none", half=False, spp=1, ipb=0, const=True, aa=PM.AA_SCALE, fov=90.0):
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT, iterations_per_batch=ipb)
    if const:
        r.set_constant_env(ENV)
    else:
        r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
    r.init_render_settings(seed=PM.SEED, samples_per_step=spp, aa_noise_scale=aa, fov_degrees=fov)
    r.set_scene(scene)
    if PM.CAMERAS[camera] is not None:
        r.set_camera(**PM.CAMERAS[camera])
    return r


def _step(P, r):
    rec = P.worklist(W, H)
    r.setup(rec)
    r.path_trace()
    return rec, r.read_results(rec)


def _radiance(p, emission=LAMP, env=F32(ENV)):
    want = np.zeros((len(p), 3), F32)
    for code, col in ((1, env), (2, F32(emission))):
        m = p["escaped"] == code
        want[m] = col[None, :] * p["throughput"][m]
    return want


def _extras():
    return [{"shape": "parallelogram", "material": "emissive", "colour": LAMP,
             "vertices": ((-0.08, 0.22, -0.62), (0.08, 0.23, -0.62), (-0.08, 0.2, -0.48))},
            {"shape": "sphere", "material": "specular", "centre": (-0.15, -0.1, -0.6), "radius": 0.05, "colour": (1.0, 1.0, 1.0)}]


# ---- 1. pt_mesh_shade against the CPU program

@pytest.mark.parametrize("name", F.NAMES)
def test_mesh_shade_equals_the_cpu_program(ptmi_lib, program, tmp_path, name):
    P = ptmi_lib
    _, path = F.run_fixture(program, tmp_path, name)
    cpu = F.read_dump(path)
    assert len(cpu["t"]) >= 1 << 14
    r = P.Renderer(W, H)
    try:
        with pytest.raises(P.PtError, match="holds no mesh"):
            r.mesh_shade(cpu["origin"][:4], cpu["dir"][:4])
        r.set_scene(F.scene(name))
        infos = [r.mesh_normals_info(k) for k in range(len(F.meshes(name)))]
        t, obj, tri, bary, nrm = r.mesh_shade(cpu["origin"], cpu["dir"])
        r.set_camera(**PM.CAMERAS["moved"])                        # the hook ignores the camera
        posed = r.mesh_shade(cpu["origin"][:4096], cpu["dir"][:4096])
        assert r.mesh_shade(cpu["origin"][:0], cpu["dir"][:0])[4].shape == (0, 3)
    finally:
        r.close()
    for info, (v, tr, n, i) in zip(infos, F.meshes(name)):
        assert info == {"has_normals": int(n is not None), "per_corner": int(i is not None), "n_normals": 0 if n is None else len(n),
                        "device_bytes": 0 if n is None else 48 * len(tr)}
    differ = (_bits(t) != _bits(cpu["t"])) | (obj != cpu["mesh"]) | (tri != cpu["triangle"]) | \
        (_bits(bary) != _bits(cpu["bary"])).any(axis=1) | (_bits(nrm) != _bits(cpu["normal"])).any(axis=1)
    print("%s: %d rays, %d hits, %d differ between device and CPU" % (name, len(t), np.count_nonzero(obj >= 0), differ.sum()))
    for i in np.flatnonzero(differ)[:5]:
        print("ray %d: device %r %d %d %r %r, CPU %r %d %d %r %r" % (i, t[i], obj[i], tri[i], bary[i].tolist(), nrm[i].tolist(), cpu["t"][i],
                                                                   cpu["mesh"][i], cpu["triangle"][i], cpu["bary"][i].tolist(), cpu["normal"][i].tolist()))
    assert not differ.any()
    miss = obj < 0
    assert miss.any() and np.all(bary[miss] == 0) and np.all(nrm[miss] == 0) and np.all(t[miss] == 0)
    assert all(np.array_equal(_bits(a[:4096]), _bits(b)) for a, b in zip((t, bary, nrm), (posed[0], posed[3], posed[4])))


def test_mesh_shade_reports_zero_off_a_mesh_and_rejections_keep_the_normals(ptmi_lib):
    P = ptmi_lib
    scene = [{"shape": "sphere", "material": "diffuse", "centre": F.CENTRE, "radius": 0.12, "colour": (1.0, 1.0, 1.0)}] + F.scene("sphere")
    o = np.tile(F32([0.0, 0.0, 0.0]), (64, 1))
    d = F32(np.asarray(F.CENTRE) + np.random.default_rng(1).normal(0, 0.02, (64, 3)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = P.Renderer(W, H)
    try:
        r.set_scene(scene)
        t, obj, tri, bary, nrm = r.mesh_shade(o, d)
        assert np.all(obj == 0) and np.all(tri == -1) and np.all(t > 0) and np.all(bary == 0) and np.all(nrm == 0)   # the sphere hides the mesh
        before = r.mesh_normals_info(0)
        v, tr, n, _ = F.meshes("sphere")[0]
        bad = n.copy()
        bad[int(tr[7, 1])] = (0.0, np.float32("nan"), 0.0)
        with pytest.raises(P.PtError, match="mesh 0: triangle %d: normals\\[%d\\] must be finite \\(got nan\\)" % (np.flatnonzero((tr == tr[7, 1]).any(axis=1))[0], tr[7, 1])):
            r.set_mesh_normals(0, bad)
        with pytest.raises(P.PtError, match="mesh 0: n_normals must equal n_vertices = %d when normal_indices is null \\(got 3\\)" % len(v)):
            r.set_mesh_normals(0, n[:3])
        with pytest.raises(P.PtError, match="mesh 1: triangle 0: normal_indices\\[0\\] must be < n_normals = 1 \\(got 5\\)"):
            r.set_mesh_normals(1, n[:1], np.full((128, 3), 5, np.uint32))
        with pytest.raises(P.PtError, match="mesh 2 of 2"):
            r.set_mesh_normals(2, n)
        with pytest.raises(P.PtError, match="mesh 2 of 2"):
            r.mesh_normals_info(2)
        assert r.mesh_normals_info(0) == before and before["has_normals"] == 1 and r.mesh_normals_info(1)["has_normals"] == 0
    finally:
        r.close()


# ---- 2. off means off

def _everything(P, scene, setup=lambda r: None, camera="lens_moved", const=False):
    r = _renderer(P, scene, camera, spp=3, ipb=2, const=const)
    try:
        setup(r)
        rec = P.worklist(W, H)
        r.setup(rec)
        out = []
        for _ in range(2):
            r.path_trace()
            st = r.read_results(rec)
            out.append((rec.tobytes(), st.paths, st.segments, st.escaped))
        out.append(r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 4, np.uint32)).tobytes())
        out.append({k: v.tobytes() for k, v in r.feature_buffers().items()})
        return out
    finally:
        r.close()


def test_normals_removed_are_never_attached(ptmi_lib):
    P = ptmi_lib
    for name in ("sphere", "odd"):
        flat = _everything(P, F.scene(name, normals=False))

        def remove(r):
            n = len(F.meshes(name))
            assert any(r.mesh_normals_info(k)["has_normals"] for k in range(n))
            for k in range(n):
                r.set_mesh_normals(k, None)
            assert not any(r.mesh_normals_info(k)["has_normals"] or r.mesh_normals_info(k)["device_bytes"] for k in range(n))
        assert _everything(P, F.scene(name), remove) == flat
        smooth = _everything(P, F.scene(name))
        assert smooth[0] != flat[0] and smooth[3]["normal"] != flat[3]["normal"]          # and attached is not flat
        assert smooth[3]["object_id"] == flat[3]["object_id"] and smooth[3]["depth"] == flat[3]["depth"] and smooth[3]["albedo"] == flat[3]["albedo"]


def test_a_flat_mesh_beside_a_smooth_one_keeps_its_flat_bits_and_a_new_scene_drops_the_normals(ptmi_lib, program, tmp_path):
    P = ptmi_lib
    _, path = F.run_fixture(program, tmp_path, "sphere")
    cpu = F.read_dump(path)
    out = {}
    for normals in (True, False):
        r = _renderer(P, F.scene("sphere", normals=normals), "moved", fov=ZOOM)
        try:
            out[normals] = (r.feature_buffers(), r.mesh_shade(cpu["origin"], cpu["dir"]))
            if normals:
                assert r.mesh_normals_info(0)["has_normals"] == 1
                r.set_scene(F.scene("sphere", normals=False))                              # a scene set again drops the normals
                assert [r.mesh_normals_info(k)["has_normals"] for k in range(2)] == [0, 0]
                assert r.feature_buffers()["normal"].tobytes() != out[True][0]["normal"].tobytes()
        finally:
            r.close()
    (fs, ms), (ff, mf) = out[True], out[False]
    assert np.array_equal(fs["object_id"], ff["object_id"])
    on_flat = fs["object_id"] == 1
    on_smooth = fs["object_id"] == 0
    assert on_flat.sum() > 100 and on_smooth.sum() > 100        # not vacuous
    assert np.array_equal(_bits(fs["normal"][on_flat]), _bits(ff["normal"][on_flat]))
    assert np.count_nonzero((_bits(fs["normal"][on_smooth]) != _bits(ff["normal"][on_smooth])).any(axis=1)) > 0.9 * on_smooth.sum()
    hit_flat = ms[1] == 1
    assert hit_flat.sum() > 1000 and np.array_equal(_bits(ms[4][hit_flat]), _bits(mf[4][hit_flat]))     # its stored normal, flipped
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ms[:4], mf[:4]))                      # t, object, triangle, bary: the same hit


# ---- 3. production kernels against pt_trace_paths

PRODUCTION = [("none", False, True, ("refractive", "diffuse"), False), ("moved", True, False, ("diffuse", "refractive"), False),
              ("lens", True, True, ("specular", "diffuse"), True), ("lens_moved", False, True, ("refractive", "diffuse"), True),
              ("moved", False, False, ("specular", "diffuse"), True)]


@pytest.mark.parametrize("camera,half,const,materials,extras", PRODUCTION,
                         ids=["%s-%s-%s-%s%s" % (c, "half" if h else "float", "const" if e else "nif", m[0], "-lamp" if x else "") for c, h, e, m, x in PRODUCTION])
def test_production_kernels_equal_trace_paths(ptmi_lib, camera, half, const, materials, extras):
    P = ptmi_lib
    spp = 5
    scene = F.scene("sphere", materials) + (_extras() if extras else [])
    r = _renderer(P, scene, camera, half, spp=spp, ipb=2, const=const)
    try:
        assert r.mesh_normals_info(0)["has_normals"] == 1 and r.mesh_normals_info(1)["has_normals"] == 0
        seen = set()
        for step in range(3):
            rec, st = _step(P, r)
            assert st.first_sample == step * spp and st.trace_launches >= 3                       # 5 = 2 + 2 + 1: ragged
            paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
            assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
            assert st.paths == spp * W * H and st.segments == sum(int(p["length"].sum()) for p in paths)
            assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
            if const:
                terms = np.stack([_radiance(p).astype(np.float64) for p in paths])
                got = np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64)
                assert np.all(np.abs(got - terms.sum(0)) <= 5 * 2.0 ** -24 * np.abs(terms).sum(0))  # any order of summation
            for p in paths:
                seen |= set(np.unique(p["escaped"]).tolist())
        r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)       # one sample: bit for bit
        rec, st = _step(P, r)
        p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
        assert np.array_equal(rec["pathLength"], p["length"])
        if const:
            assert np.array_equal(_bits(np.stack([rec["r"], rec["g"], rec["b"]], -1)), _bits(_radiance(p)))
        smooth_paths = p.tobytes()
        for k in range(2):
            r.set_mesh_normals(k, None)
        assert r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32)).tobytes() != smooth_paths   # the normals matter
    finally:
        r.close()
    assert seen >= ({0, 1, 2} if extras else {0, 1}) and p["length"].max() >= 3


# ---- 4. pt_trace_paths against the float64 model with the shading normal

@pytest.mark.parametrize("camera,half,material,odd", NM.CASES,
                         ids=["%s-%s-%s%s" % (c, "half" if h else "float", m, "-odd" if o else "") for c, h, m, o in NM.CASES])
def test_trace_paths_against_the_float64_model(oracle, ptmi_lib, camera, half, material, odd):
    """The project's rule 2 R (spread + 2e-6 scale), R = 0.68, on the well-conditioned paths; at most 10 % fragile.  Shares and
    largest ratios measured on an MI355X: DESIGN.md section 4.17."""
    P = ptmi_lib
    uu, vv, ss, cam, plain, fragile, spread = NM.case(camera, half, material, odd)
    r = P.Renderer(PM.W, PM.H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT)
    try:
        r.set_constant_env(PM.ENV)
        r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
        r.set_scene(NM.world_scene(camera, material, odd))
        if PM.CAMERAS[camera] is not None:
            r.set_camera(**PM.CAMERAS[camera])
        info = [r.mesh_normals_info(k) for k in range(2)]
        p = r.trace_paths(uu, vv, ss)
    finally:
        r.close()
    assert [i["has_normals"] for i in info] == [1, 0] and info[0]["per_corner"] == int(odd)
    assert np.array_equal(p["cam"], cam)                    # the model ran on the camera rays the library forms
    same, ratio = PM.compare(p, plain, fragile, spread)
    ok = ~fragile
    print("mesh normals model / %s / %s / %s%s: fragile %.2f %%, largest ratio %.3f of %.3f allowed; mismatching outcomes %d" % (
        camera, "half" if half else "float", material, " / odd" if odd else "", 100 * fragile.mean(), ratio, M.GPU_FACTOR,
        np.count_nonzero((p["length"] != plain["length"])[ok] | (p["escaped"] != plain["escaped"])[ok])))
    assert fragile.mean() <= M.FRAGILE_CAP
    assert same
    assert ratio <= M.GPU_FACTOR
    assert set(np.unique(p["escaped"]).tolist()) == {0, 1, 2} and p["length"].max() >= 4


# ---- 5. feature buffers: the closed form and continuity

def _sphere_features(P, normals, fov):
    """(features, centre-ray directions (H, W, 3) in float64) of the sphere fixture under the built-in camera."""
    r = _renderer(P, F.scene("sphere", normals=normals), "none", aa=0.0, fov=fov)
    try:
        feats = r.feature_buffers()
        u, v = PM.all_pixels()
        cam = r.trace_paths(u, v, np.zeros(len(u), np.uint32))["cam"].astype(np.float64)   # AA scale 0: the centre rays' (camx, camy)
    finally:
        r.close()
    d = np.stack([cam[:, 0], cam[:, 1], -np.ones(len(cam))], -1)
    return feats, (d / np.linalg.norm(d, axis=1, keepdims=True)).reshape(H, W, 3)


def _closed_form_deviation(feats, d, on):
    hp = feats["depth"].astype(np.float64)[..., None] * d
    ref = hp - np.asarray(F.CENTRE)
    ref /= np.linalg.norm(ref, axis=-1, keepdims=True)
    ref[np.einsum("hwk,hwk->hw", ref, d) > 0] *= -1.0
    return np.abs(feats["normal"].astype(np.float64) - ref).max(axis=-1)[on]


def _neighbour_jumps(feats, on):
    n = feats["normal"].astype(np.float64)
    jumps = []
    for a, b, pa, pb in ((n[:, 1:], n[:, :-1], on[:, 1:], on[:, :-1]), (n[1:], n[:-1], on[1:], on[:-1])):
        jumps.append(np.abs(a - b).max(axis=-1)[pa & pb])
    return np.concatenate(jumps)


def _smooth_and_flat(P, fov):
    """(smooth features, flat features, centre rays, sphere pixels, the well-conditioned ones among them): a sphere pixel is well
    conditioned unless rule 4 (or 2) gave the geometric normal back, which shows as the flat render's bits."""
    smooth, d = _sphere_features(P, True, fov)
    flat, _ = _sphere_features(P, False, fov)
    assert np.array_equal(smooth["object_id"], flat["object_id"]) and np.array_equal(_bits(smooth["depth"]), _bits(flat["depth"]))
    on = smooth["object_id"] == 0
    kept = on & (_bits(smooth["normal"]) != _bits(flat["normal"])).any(axis=-1)
    assert on.sum() > 1000 and kept.sum() >= 0.9 * on.sum()
    return smooth, flat, d, on, kept


def test_feature_normals_follow_the_sphere(ptmi_lib):
    """The whole ball in view.  Fails on a build that accepts the normals and shades flat: the flat mesh's own figure is asserted
    to break the bound."""
    smooth, flat, d, on, kept = _smooth_and_flat(ptmi_lib, CLOSE)
    dev, dev_flat = _closed_form_deviation(smooth, d, kept), _closed_form_deviation(flat, d, kept)
    print("sphere pixels %d (kept %d): closed form smooth %.3e (bound %.3e) flat %.3e" % (on.sum(), kept.sum(), dev.max(), F.CLOSED_FORM_BOUND, dev_flat.max()))
    assert dev.max() <= F.CLOSED_FORM_BOUND
    assert dev_flat.max() > 100 * F.CLOSED_FORM_BOUND


def test_feature_normals_are_continuous_across_edges(ptmi_lib):
    """Every pair of adjacent well-conditioned sphere pixels differs by less than the flat render's smallest facet-to-facet jump.
    The yardstick needs a zoom at which the sphere itself turns slower than a facet: the true normal changes by
    (pixel footprint) / (radius cos) between neighbours, which no zoom bounds at the limb.  So the camera looks at the ball's
    front cap alone, 8 degrees of view: every pixel is on the ball, the incidence stays under 63 degrees (cos > 0.45), a pixel's
    footprint is 0.011 radii and the true change at most 0.025, against facet jumps of about 0.1.  Fails on the flat mesh."""
    smooth, flat, d, on, kept = _smooth_and_flat(ptmi_lib, NARROW)
    assert on.all()
    cos = -np.einsum("hwk,hwk->hw", smooth["normal"].astype(np.float64), d)
    assert cos.min() > 0.45
    jumps, jumps_flat = _neighbour_jumps(smooth, kept), _neighbour_jumps(flat, kept)
    facet = jumps_flat[jumps_flat > 0].min()                                        # the flat render's smallest facet-to-facet jump
    facets = len(np.unique(_bits(flat["normal"]).reshape(-1, 3), axis=0))
    dev = _closed_form_deviation(smooth, d, kept)
    print("front cap: %d pixels (kept %d) over %d facets, smallest cos %.3f: neighbour jump smooth %.3e, flat facets %.3e .. %.3e; closed form %.3e" % (
        on.sum(), kept.sum(), facets, cos.min(), jumps.max(), facet, jumps_flat.max(), dev.max()))
    assert facets >= 20 and np.count_nonzero(jumps_flat > 0) >= 100                  # interior edges are crossed, many times
    assert jumps.max() < facet
    assert jumps_flat.max() >= facet and dev.max() <= F.CLOSED_FORM_BOUND           # the flat mesh fails


# ---- 6. the guides

def test_guides_on_a_smooth_scene(ptmi_lib):
    P = ptmi_lib
    scene = F.scene("sphere", ("diffuse", "diffuse")) + [
        {"shape": "sphere", "material": "emissive", "centre": (0.12, 0.12, -0.5), "radius": 0.04, "colour": LAMP}]

    def run(setup, spp=2, steps=2):
        r = _renderer(P, scene, "moved", spp=spp, ipb=1, fov=ZOOM)
        try:
            setup(r)
            rec = P.worklist(W, H)
            r.setup(rec)
            for _ in range(steps):
                r.path_trace()
                r.read_results(rec)
            return rec.tobytes()
        finally:
            r.close()

    sky = np.full((16, 32, 3), 0.1, F32)
    sky[3, 5] = 50.0
    assert run(lambda r: (r.set_env_guide(sky, rows=8, cols=16, alpha=0.0), r.set_light_guide(beta=0.0))) == run(lambda r: None)
    # guided and unguided estimate the same image on the smooth diffuse mesh's pixels: fixed seeds, |z| < 4 of the step means
    r = _renderer(P, scene, "moved", fov=ZOOM)
    try:
        on = (r.feature_buffers()["object_id"] == 0).ravel()
    finally:
        r.close()
    assert on.sum() > 100
    steps, spp = 12, 16
    films = {}
    # alpha + beta may not exceed 0.9 (pt_set_light_guide): each guide alone at 0.5, and the mixture of both at 0.45 + 0.45
    settings = {None: (0.0, 0.0), "emitter": (0.0, 0.5), "environment": (0.5, 0.0), "both": (0.45, 0.45)}
    for guided, (alpha, beta) in settings.items():
        r = _renderer(P, scene, "moved", spp=spp, fov=ZOOM)
        try:
            if alpha:
                r.set_env_guide(sky, rows=8, cols=16, alpha=alpha)
            if beta:
                r.set_light_guide(beta=beta)
            means = []
            for _ in range(steps):
                rec, st = _step(P, r)
                means.append(np.stack([rec["r"], rec["g"], rec["b"]], -1).astype(np.float64)[on].mean(axis=0) / spp)
            films[guided] = np.array(means)
            if guided:                                                                     # and it is pt_trace_paths' guided twin
                r.init_render_settings(seed=PM.SEED + 1, samples_per_step=1, aa_noise_scale=PM.AA_SCALE, fov_degrees=ZOOM)
                rec, st = _step(P, r)
                p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
                assert np.array_equal(rec["pathLength"], p["length"])
                assert np.array_equal(_bits(np.stack([rec["r"], rec["g"], rec["b"]], -1)), _bits(_radiance(p)))
        finally:
            r.close()
    off = films[None]
    for guided in ("emitter", "environment", "both"):
        on_ = films[guided]
        se = np.sqrt(off.var(axis=0, ddof=1) / steps + on_.var(axis=0, ddof=1) / steps)
        z = (on_.mean(axis=0) - off.mean(axis=0)) / se
        print("%s guide on a smooth mesh: off %s on %s, z %s" % (guided, off.mean(axis=0), on_.mean(axis=0), z))
        assert np.all(np.abs(z) < 4.0) and not np.array_equal(off, on_)


# ---- 7. the camera

def test_normals_follow_a_new_pose_without_allocating(ptmi_lib):
    P = ptmi_lib
    scene = F.scene("odd") + _extras()
    r = _renderer(P, scene, "none", spp=2, ipb=1)
    try:
        _step(P, r)
        first = [r.mesh_normals_info(k) for k in range(3)]
        r.set_camera(**PM.CAMERAS["moved"])
        rec, st = _step(P, r)
        paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 3, np.uint32))
        feats = r.feature_buffers()
        assert [r.mesh_normals_info(k) for k in range(3)] == first                                # nothing allocated, nothing lost
    finally:
        r.close()
    assert [i["device_bytes"] for i in first] == [0, 48 * 320, 48]
    fresh = _renderer(P, scene, "moved", spp=2, ipb=1)
    try:
        _step(P, fresh)
        rec_f, _ = _step(P, fresh)
        paths_f = fresh.trace_paths(rec_f["u"], rec_f["v"], np.full(len(rec_f), 3, np.uint32))
        feats_f = fresh.feature_buffers()
    finally:
        fresh.close()
    assert paths.tobytes() == paths_f.tobytes() and rec.tobytes() == rec_f.tobytes()
    assert all(feats[k].tobytes() == feats_f[k].tobytes() for k in feats)
    assert np.count_nonzero(feats["object_id"] == 1) > 20


# ---- 8. NIF sharing, the memo and the denoiser

def test_sharing_memo_and_denoiser_on_a_smooth_scene(ptmi_lib):
    P = ptmi_lib
    scene = F.scene("sphere") + _extras()

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
