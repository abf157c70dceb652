"""Texture coordinates and image textures of meshes (pt_set_mesh_texture) on the GPU.  Scenes are the fixtures of
tests/mesh_texture_fixtures.py: two or three meshes, the first without a texture, so a textured mesh's slots and its descriptor do not
start at 0; 64 x 48 images, a few hundred triangles, images of at most 5 x 3 texels.

1. pt_mesh_texel equals the CPU program tests/mesh_texture_main.cpp on its own rays, bit for bit, for both filters and both wraps.
2. Off means off: a texture removed, an untextured mesh beside a textured one, a scene set again.
3. Pins, bit for bit: an all-ones image renders the untextured bits (without normals: the MESH instances' render; with normals: the
   SMOOTH instances'), a constant image k the untextured scene with colour fl(colour x k) for diffuse, glass and emissive; a mirror
   ignores its texture.
4. Closed form, exact: an emissive grid at z = -1 under the built-in camera with a 4 x 3 NEAREST image.
5. The production kernels' textured instances equal pt_trace_paths bit for bit.
6. pt_trace_paths against the float64 model with textures (tests/scene_mesh_texture_model.py): four cameras, both sample precisions,
   the textured smooth ball glass, mirror and diffuse over a textured field, at the project's rule 2 R (spread + 2e-6 scale), R = 0.68.
7. Feature buffers: albedo = colour x pt_mesh_texel's bgr on the centre rays, bit for bit.
8. The guides at zero, guided twins, a pose change, NIF sharing and the memo.
"""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests import mesh_normals_fixtures as NF
from tests import mesh_texture_fixtures as F
from tests import scene_mesh_texture_model as TM
from tests import scene_model as M
from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 64, 48
ENV = (0.75, 1.5, 3.0)
LAMP = (6.0, 4.5, 3.0)
ZOOM = 40.0          # degrees: the icosphere, a fifth of a unit across, covers a few hundred of the 64 x 48 pixels


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return F.build_program(tmp_path_factory.mktemp("mesh_texture_gpu"))


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


def _radiance(p, env=F32(ENV)):
    """What an escaped path's record adds to its accumulator: the environment's radiance times the throughput.  (A path that ended
    on an emitter adds the emitter's colour -- times its texel -- times the throughput; the record does not say which emitter.)"""
    want = np.zeros((len(p), 3), F32)
    m = p["escaped"] == 1
    want[m] = env[None, :] * p["throughput"][m]
    return want


def _extras():
    return [{"shape": "parallelogram", "material": "emissive", "colour": LAMP,
             "vertices": ((-0.08, 0.22, -0.62), (0.08, 0.23, -0.62), (-0.08, 0.2, -0.48))},
            {"shape": "sphere", "material": "specular", "centre": (-0.15, -0.1, -0.6), "radius": 0.05, "colour": (1.0, 1.0, 1.0)}]


def _expected_info(tex, triangles):
    if tex is None:
        return {"has_texture": 0, "per_corner": 0, "width": 0, "height": 0, "filter": 0, "wrap": 0, "n_uvs": 0, "device_bytes": 0}
    h, w = tex["image"].shape[:2]
    return {"has_texture": 1, "per_corner": int(tex["uv_indices"] is not None), "width": w, "height": h, "filter": tex["filter"],
            "wrap": tex["wrap"], "n_uvs": len(tex["uvs"]), "device_bytes": 24 * triangles + 16 * w * h}


# ---- 1. pt_mesh_texel against the CPU program

@pytest.mark.parametrize("name", F.NAMES)
def test_mesh_texel_equals_the_cpu_program(ptmi_lib, program, tmp_path, name):
    P = ptmi_lib
    _, path = F.run_fixture(program, tmp_path, name)
    cpu = F.read_dump(path)
    assert len(cpu["t"]) >= 1 << 14
    r = P.Renderer(W, H)
    try:
        with pytest.raises(P.PtError, match="holds no mesh"):
            r.mesh_texel(cpu["origin"][:4], cpu["dir"][:4])
        r.set_scene(F.scene(name))
        infos = [r.mesh_texture_info(k) for k in range(len(F.meshes(name)))]
        t, obj, tri, uv, bgr = r.mesh_texel(cpu["origin"], cpu["dir"])
        r.set_camera(**PM.CAMERAS["moved"])                        # the hook ignores the camera
        posed = r.mesh_texel(cpu["origin"][:4096], cpu["dir"][:4096])
        assert r.mesh_texel(cpu["origin"][:0], cpu["dir"][:0])[4].shape == (0, 3)
    finally:
        r.close()
    for info, (v, tr, tex) in zip(infos, F.meshes(name)):
        assert info == _expected_info(tex, len(tr))
    differ = (_bits(t) != _bits(cpu["t"])) | (obj != cpu["mesh"]) | (tri != cpu["triangle"]) | \
        (_bits(uv) != _bits(cpu["uv"])).any(axis=1) | (_bits(bgr) != _bits(cpu["bgr"])).any(axis=1)
    print("%s: %d rays, %d hits (%d on textured meshes), %d differ between device and CPU" % (
        name, len(t), np.count_nonzero(obj >= 0), np.count_nonzero(obj > 0), differ.sum()))
    for i in np.flatnonzero(differ)[:5]:
        print("ray %d: device %r %d %d %r %r, CPU %r %d %d %r %r" % (i, t[i], obj[i], tri[i], uv[i].tolist(), bgr[i].tolist(), cpu["t"][i],
                                                                   cpu["mesh"][i], cpu["triangle"][i], cpu["uv"][i].tolist(), cpu["bgr"][i].tolist()))
    assert not differ.any()
    miss = obj < 0
    assert miss.any() and np.all(uv[miss] == 0) and np.all(bgr[miss] == 0) and np.all(t[miss] == 0)
    plain = obj == 0
    assert plain.sum() > 1000 and np.all(uv[plain] == 0) and np.all(bgr[plain] == 1)
    assert all(np.array_equal(_bits(a[:4096]), _bits(b)) for a, b in zip((t, uv, bgr), (posed[0], posed[3], posed[4])))


def test_mesh_texel_reports_zero_off_a_mesh_and_rejections_keep_the_texture(ptmi_lib):
    P = ptmi_lib
    name = "bilinear_clamp"
    scene = [{"shape": "sphere", "material": "diffuse", "centre": NF.CENTRE, "radius": 0.12, "colour": (1.0, 1.0, 1.0)}] + F.scene(name)
    o = np.tile(F32([0.0, 0.0, 0.0]), (64, 1))
    d = F32(np.asarray(NF.CENTRE) + np.random.default_rng(1).normal(0, 0.02, (64, 3)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = P.Renderer(W, H)
    try:
        r.set_scene(scene)
        t, obj, tri, uv, bgr = r.mesh_texel(o, d)
        assert np.all(obj == 0) and np.all(tri == -1) and np.all(t > 0) and np.all(uv == 0) and np.all(bgr == 0)   # the sphere hides the mesh
        before = [r.mesh_texture_info(k) for k in range(3)]
        v, tr, tex = F.meshes(name)[1]
        img, uvs = tex["image"], tex["uvs"]
        bad = img.copy()
        bad[2, 3, 1] = -0.5
        with pytest.raises(P.PtError, match="mesh 1: texture: texel \\(row 2, column 3\\) channel 1 must be finite and >= 0 \\(got -0.5\\)"):
            r.set_mesh_texture(1, bad, uvs)
        bad_uv = uvs.copy()
        bad_uv[int(tr[7, 1])] = (0.0, np.float32("nan"))
        with pytest.raises(P.PtError, match="mesh 1: triangle %d: uvs\\[%d\\] must be finite \\(got nan\\)" % (np.flatnonzero((tr == tr[7, 1]).any(axis=1))[0], tr[7, 1])):
            r.set_mesh_texture(1, img, bad_uv)
        with pytest.raises(P.PtError, match="mesh 1: texture: n_uvs must equal n_vertices = %d when uv_indices is null \\(got 3\\)" % len(v)):
            r.set_mesh_texture(1, img, uvs[:3])
        with pytest.raises(P.PtError, match="mesh 0: triangle 0: uv_indices\\[0\\] must be < n_uvs = 1 \\(got 5\\)"):
            r.set_mesh_texture(0, img, uvs[:1], np.full((128, 3), 5, np.uint32))
        with pytest.raises(P.PtError, match="filter must be 0 \\(nearest\\) or 1 \\(bilinear\\) \\(got 7\\)"):
            r.set_mesh_texture(1, img, uvs, filter=7)
        with pytest.raises(P.PtError, match="wrap must be 0 \\(repeat\\) or 1 \\(clamp\\) \\(got 2\\)"):
            r.set_mesh_texture(1, img, uvs, wrap=2)
        with pytest.raises(P.PtError, match="mesh 3 of 3"):
            r.set_mesh_texture(3, img, uvs)
        with pytest.raises(P.PtError, match="mesh 3 of 3"):
            r.mesh_texture_info(3)
        assert [r.mesh_texture_info(k) for k in range(3)] == before and [b["has_texture"] for b in before] == [0, 1, 1]
        r.set_mesh_texture(1, img[:2, :4], uvs, filter="nearest", wrap="repeat")            # replaced: the new image's size and modes
        assert r.mesh_texture_info(1) == dict(before[1], width=4, height=2, filter=0, wrap=0, device_bytes=24 * len(tr) + 16 * 8)
    finally:
        r.close()


# ---- 2. off means off

def _everything(P, scene, setup=lambda r: None, camera="lens_moved", const=False, fov=90.0):
    r = _renderer(P, scene, camera, spp=3, ipb=2, const=const, fov=fov)
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


def test_a_texture_removed_is_never_attached(ptmi_lib):
    P = ptmi_lib
    for name, materials in (("nearest_repeat", ("refractive", "diffuse")), ("bilinear_repeat", ("diffuse", "refractive", "emissive"))):
        plain = _everything(P, F.scene(name, materials, textures=False))

        def remove(r):
            n = len(F.meshes(name))
            assert any(r.mesh_texture_info(k)["has_texture"] for k in range(n))
            for k in range(n):
                r.set_mesh_texture(k, None)
            assert not any(r.mesh_texture_info(k)["has_texture"] or r.mesh_texture_info(k)["device_bytes"] for k in range(n))
        assert _everything(P, F.scene(name, materials), remove) == plain
        textured = _everything(P, F.scene(name, materials))
        assert textured[0] != plain[0] and textured[2] != plain[2] and textured[3]["albedo"] != plain[3]["albedo"]   # and attached is not plain
        assert all(textured[3][k] == plain[3][k] for k in ("object_id", "depth", "normal"))


def test_an_untextured_mesh_beside_a_textured_one_keeps_its_bits_and_a_new_scene_drops_the_texture(ptmi_lib):
    P = ptmi_lib
    name = "bilinear_clamp"
    out = {}
    for textures in (True, False):
        r = _renderer(P, F.scene(name, textures=textures), "moved", fov=ZOOM)
        try:
            u, v = PM.all_pixels()
            out[textures] = (r.feature_buffers(), r.trace_paths(u, v, np.zeros(len(u), np.uint32)))
            if textures:
                assert [r.mesh_texture_info(k)["has_texture"] for k in range(3)] == [0, 1, 1]
                r.set_scene(F.scene(name, textures=False))                                # a scene set again drops the textures
                assert [r.mesh_texture_info(k)["has_texture"] for k in range(3)] == [0, 0, 0]
                again = (r.feature_buffers(), r.trace_paths(u, v, np.zeros(len(u), np.uint32)))
        finally:
            r.close()
    (ft, pt), (fp, pp) = out[True], out[False]
    assert all(again[0][k].tobytes() == fp[k].tobytes() for k in fp) and again[1].tobytes() == pp.tobytes()
    assert all(ft[k].tobytes() == fp[k].tobytes() for k in ("object_id", "depth", "normal"))
    on_plain, on_textured = ft["object_id"] == 0, ft["object_id"] == 1
    assert on_plain.sum() > 100 and on_textured.sum() > 100          # not vacuous
    assert np.array_equal(_bits(ft["albedo"][on_plain]), _bits(fp["albedo"][on_plain]))
    assert np.count_nonzero((_bits(ft["albedo"][on_textured]) != _bits(fp["albedo"][on_textured])).any(axis=1)) > 0.9 * on_textured.sum()
    # a path whose first hit is the plain mesh and that ends there or escapes from it saw no texture: its record keeps its bits
    first_plain = on_plain.ravel() & (pp["length"] <= 2)
    assert first_plain.sum() > 50 and pt[first_plain].tobytes() == pp[first_plain].tobytes()
    assert pt.tobytes() != pp.tobytes()


# ---- 3. pins

def _with_texture(scene, image, which=None, filter="bilinear", wrap="repeat"):
    """The scene's meshes (those of index `which`, or all) with `image` on planar per-vertex uvs that leave the unit square."""
    out, k = [], 0
    for o in scene:
        o = dict(o)
        if o["shape"] == "mesh":
            if which is None or k in which:
                for key in ("uv_indices",):
                    o.pop(key, None)
                o.update(texture=image, uvs=F.planar_uvs(o["vertices"], -0.7, 1.6, axes=(0, 1) if np.ptp(np.asarray(o["vertices"])[:, 1]) > 0.05 else (0, 2)),
                         texture_filter=filter, texture_wrap=wrap)
            k += 1
        out.append(o)
    return out


@pytest.mark.parametrize("normals", [False, True], ids=["flat", "smooth"])
@pytest.mark.parametrize("filter", ["nearest", "bilinear"])
def test_an_all_ones_image_renders_the_untextured_bits(ptmi_lib, normals, filter):
    """Without normals the yardstick is the MESH instances' render, with normals the SMOOTH instances': the TEX instances carry both."""
    P = ptmi_lib
    scene = NF.scene("sphere", ("refractive", "diffuse"), normals=normals) + _extras()
    ones = np.ones((3, 5, 3), F32)
    plain = _everything(P, scene)
    seen = {}

    def check(r):
        seen["tex"] = [r.mesh_texture_info(k)["has_texture"] for k in range(2)]
        seen["normals"] = [r.mesh_normals_info(k)["has_normals"] for k in range(2)]
    assert _everything(P, _with_texture(scene, ones, filter=filter), check) == plain
    assert seen == {"tex": [1, 1], "normals": [int(normals), 0]}


K = F32((0.5, 0.3, 0.7))          # a constant image, (B, G, R)
COLOUR = F32((0.8, 0.7, 0.5))     # (R, G, B)


@pytest.mark.parametrize("material", ["diffuse", "refractive", "emissive"])
def test_a_constant_image_scales_the_colour(ptmi_lib, material):
    """colour x k is ONE multiply per channel before the material branch, so the render equals the untextured scene whose colour is
    fl(colour x k), bit for bit: as a diffuse factor, as glass's tint, as an emitter's radiance."""
    P = ptmi_lib
    colour = F32(LAMP) if material == "emissive" else COLOUR
    base = NF.scene("sphere", (material, "diffuse"), normals=False) + _extras()
    base[0]["colour"] = tuple(colour)
    scaled = [dict(o) for o in base]
    scaled[0]["colour"] = tuple(colour * K[::-1])                    # R x k.R, G x k.G, B x k.B in binary32
    image = np.broadcast_to(K, (2, 3, 3))
    want = _everything(P, scaled, fov=ZOOM)
    assert _everything(P, _with_texture(base, image, which={0}, filter="nearest", wrap="clamp"), fov=ZOOM) == want
    assert _everything(P, _with_texture(base, image, which={0}), fov=ZOOM) == want
    assert _everything(P, base, fov=ZOOM)[0] != want[0]                  # and the constant matters


def test_a_mirror_ignores_its_texture(ptmi_lib):
    P = ptmi_lib
    base = NF.scene("sphere", ("specular", "diffuse"), normals=False) + _extras()
    want = _everything(P, base, fov=ZOOM)
    assert _everything(P, _with_texture(base, F.image_5x3(), which={0}), fov=ZOOM) == want
    assert _everything(P, _with_texture(base, F.image_5x3(), which={1}), fov=ZOOM)[0] != want[0]   # the diffuse mesh beside it does not


# ---- 4. closed form, exact

X0, X1, Y0, Y1 = -1.015625, 0.984375, -0.734375, 0.765625
GRID_COLOUR = F32((2.0, 0.5, 4.0))       # powers of two: colour x texel is exact


def _grid(nx=8, ny=12):
    """A flat grid at z = -1 over [X0, X1] x [Y0, Y1], nx x ny cells of 1/4 x 1/8, each split along the diagonal from its lower left
    to its upper right corner; uvs linear in x and y over the rectangle.  A pixel's centre ray meets z = -1 at (u / 32 - 1,
    3 / 4 - v / 32) times 1 - 2^-11 (the half-rounded tan of 45 degrees): never on a grid line (those lie at odd multiples of 1 / 64) and never on a diagonal (2 (y - y_j) = x - x_i has
    an even left and an odd right side in units of 1 / 64, and the scale moves a point by less than 1 / 2048), so no ray meets an edge."""
    xs, ys = np.linspace(X0, X1, nx + 1), np.linspace(Y0, Y1, ny + 1)
    gx, gy = np.meshgrid(xs, ys)
    v = F32(np.stack([gx.ravel(), gy.ravel(), -np.ones(gx.size)], -1))
    uvs = F32(np.stack([(gx.ravel() - X0) / (X1 - X0), (gy.ravel() - Y0) / (Y1 - Y0)], -1))
    tris = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            tris += [(a, a + 1, a + nx + 2), (a, a + nx + 2, a + nx + 1)]
    assert np.array_equal(v[:, :2].astype(np.float64), np.stack([gx.ravel(), gy.ravel()], -1))      # the corners are exact in binary32
    return v, np.uint32(tris), uvs


def test_closed_form_on_an_emissive_grid(ptmi_lib):
    """Every accumulator equals colour x texel(column floor(4 s), row floor(3 (1 - t))) exactly, path length 1: s = (x - X0) / 2 and
    t = (y - Y0) / 1.5 at the hit, texel boundaries 1 / 128 in s away from every pixel.  A transposed or flipped lookup fails this."""
    P = ptmi_lib
    v, tris, uvs = _grid()
    assert len(tris) == 192
    image = F32(1.0 + np.arange(36).reshape(3, 4, 3) / 64.0)         # twelve distinct texels, exact in binary32
    scene = [{"shape": "mesh", "material": "emissive", "colour": tuple(GRID_COLOUR), "vertices": v, "triangles": tris,
              "texture": image, "uvs": uvs, "texture_filter": "nearest", "texture_wrap": "repeat"}]
    r = _renderer(P, scene, "none", aa=0.0, fov=90.0)
    try:
        rec, st = _step(P, r)
        u, vv = PM.all_pixels()
        cam = r.trace_paths(u, vv, np.zeros(len(u), np.uint32))["cam"].astype(np.float64)
    finally:
        r.close()
    # the work items in pixel order
    order = np.lexsort((rec["u"], rec["v"]))
    rec = rec[order]
    assert np.array_equal(rec["u"], u) and np.array_equal(rec["v"], vv)
    x, y = cam[:, 0], cam[:, 1]
    # multiples of 1 / 32 but for the half-rounded tan(45 degrees) = 1 - 2^-11 they are scaled by: within 2^-10 of one
    assert np.abs(x * 32 - np.round(x * 32)).max() <= 32 * 2.0 ** -10 and np.abs(y * 32 - np.round(y * 32)).max() <= 32 * 2.0 ** -10
    assert x.min() > X0 and x.max() < X1 and y.min() > Y0 and y.max() < Y1
    s, t = (x - X0) / (X1 - X0), (y - Y0) / (Y1 - Y0)
    margin = min(np.abs(4 * s - np.round(4 * s)).min() / 4, np.abs(3 * t - np.round(3 * t)).min() / 3)
    assert margin >= 1.0 / 128 - 2.0 ** -10                          # the texel boundaries lie halfway between two such multiples
    col, row = np.floor(4 * s).astype(int), np.floor(3 * (1 - t)).astype(int)
    assert set(zip(row.tolist(), col.tolist())) == {(a, b) for a in range(3) for b in range(4)}       # every texel is seen
    texel = image[row, col]                                           # (n, 3) B, G, R
    want = np.stack([GRID_COLOUR[0] * texel[:, 2], GRID_COLOUR[1] * texel[:, 1], GRID_COLOUR[2] * texel[:, 0]], -1).astype(F32)
    got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
    wrong = (_bits(got) != _bits(want)).any(axis=1)
    print("emissive grid: %d pixels, %d wrong, margin %.6f" % (len(got), wrong.sum(), margin))
    assert np.all(rec["pathLength"] == 1)
    assert not wrong.any()
    assert st.escaped == 0


# ---- 5. production kernels against pt_trace_paths

PRODUCTION = [("none", False, True, ("diffuse", "refractive", "emissive"), True), ("moved", True, False, ("refractive", "diffuse", "emissive"), False),
              ("lens", True, True, ("diffuse", "diffuse", "emissive"), True), ("lens_moved", False, False, ("diffuse", "refractive", "diffuse"), True),
              ("moved", False, True, ("specular", "emissive", "refractive"), True)]


@pytest.mark.parametrize("camera,half,const,materials,extras", PRODUCTION,
                         ids=["%s-%s-%s-%s%s" % (c, "half" if h else "float", "const" if e else "nif", m[1], "-lamp" if x else "") for c, h, e, m, x in PRODUCTION])
def test_production_kernels_equal_trace_paths(ptmi_lib, camera, half, const, materials, extras):
    P = ptmi_lib
    spp = 5
    scene = F.scene("bilinear_repeat", materials) + (_extras() if extras else [])
    r = _renderer(P, scene, camera, half, spp=spp, ipb=2, const=const)
    try:
        assert [r.mesh_texture_info(k)["has_texture"] for k in range(3)] == [0, 1, 1]
        seen = set()
        for step in range(3):
            rec, st = _step(P, r)
            assert st.first_sample == step * spp and st.trace_launches >= 3                       # 5 = 2 + 2 + 1: ragged
            paths = [r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample + k, np.uint32)) for k in range(spp)]
            assert np.array_equal(rec["pathLength"], sum(p["length"] for p in paths))
            assert st.paths == spp * W * H and st.segments == sum(int(p["length"].sum()) for p in paths)
            assert st.escaped == sum(np.count_nonzero(p["escaped"] == 1) for p in paths)
            for p in paths:
                seen |= set(np.unique(p["escaped"]).tolist())
        r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)       # one sample: bit for bit
        rec, st = _step(P, r)
        p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
        assert np.array_equal(rec["pathLength"], p["length"])
        if const:
            got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
            esc = p["escaped"] == 1
            assert np.array_equal(_bits(got[esc]), _bits(_radiance(p)[esc]))
            assert np.all(got[p["escaped"] == 0] == 0)
            if materials[1] != "emissive":
                # a path that ended on an emitter: the lamp's colour, or the triangle's colour x its 1 x 1 image, times the throughput
                lamps = ([F32(LAMP)] if extras else []) + \
                    ([F32((0.8, 0.7, 0.5)) * F.meshes("bilinear_repeat")[2][2]["image"][0, 0][::-1]] if materials[2] == "emissive" else [])
                em = p["escaped"] == 2
                hit = np.zeros(em.sum(), bool)
                for lamp in lamps:
                    hit |= (_bits(got[em]) == _bits(lamp[None, :] * p["throughput"][em])).all(axis=1)
                assert em.sum() > 0 and hit.all()
        textured_paths = p.tobytes()
        for k in range(3):
            r.set_mesh_texture(k, None)
        plain = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
        assert plain.tobytes() != textured_paths                                                   # the textures matter
    finally:
        r.close()
    assert seen >= {0, 1, 2} and p["length"].max() >= 3


def test_production_emitted_radiance_is_the_textured_colour(ptmi_lib):
    """A one-sample step under a constant sky: every accumulator of a path that ended on the textured emissive triangle (length 1:
    seen directly) is LAMP x its 1 x 1 image, one multiply per channel."""
    P = ptmi_lib
    scene = F.scene("bilinear_repeat", ("diffuse", "diffuse", "emissive"), colour=LAMP)
    image = F.meshes("bilinear_repeat")[2][2]["image"][0, 0]
    r = _renderer(P, scene, "none", aa=0.0)
    try:
        rec, st = _step(P, r)
        ids = r.feature_buffers()["object_id"]
    finally:
        r.close()
    on = (ids[rec["v"], rec["u"]] == 2)
    assert on.sum() >= 5 and np.all(rec["pathLength"][on] == 1)
    want = F32(LAMP) * image[::-1]
    assert np.array_equal(_bits(np.stack([rec["r"], rec["g"], rec["b"]], -1)[on]), _bits(np.tile(want, (on.sum(), 1))))


# ---- 6. pt_trace_paths against the float64 model with textures

@pytest.mark.parametrize("camera,half,material,odd", TM.CASES,
                         ids=["%s-%s-%s%s" % (c, "half" if h else "float", m, "-odd" if o else "") for c, h, m, o in TM.CASES])
def test_trace_paths_against_the_float64_model(oracle, ptmi_lib, camera, half, material, odd):
    """The project's rule 2 R (spread + 2e-6 scale), R = 0.68, on the well-conditioned paths; at most 10 % fragile; no outcome among
    the well-conditioned paths may mismatch.  Shares and largest ratios measured on an MI355X: DESIGN.md section 4.18."""
    P = ptmi_lib
    uu, vv, ss, cam, plain, fragile, spread = TM.case(camera, half, material, odd)
    r = P.Renderer(PM.W, PM.H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE,
                   sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT)
    try:
        r.set_constant_env(PM.ENV)
        r.init_render_settings(seed=PM.SEED, samples_per_step=1, aa_noise_scale=PM.AA_SCALE)
        r.set_scene(TM.world_scene(camera, material, odd))
        if PM.CAMERAS[camera] is not None:
            r.set_camera(**PM.CAMERAS[camera])
        info = [r.mesh_texture_info(k) for k in range(2)]
        normals = [r.mesh_normals_info(k)["has_normals"] for k in range(2)]
        p = r.trace_paths(uu, vv, ss)
    finally:
        r.close()
    assert [i["has_texture"] for i in info] == [1, 1] and info[0]["per_corner"] == int(odd) and normals == [1, 0]
    assert [(i["filter"], i["wrap"]) for i in info] == [(1, 0), (1, 1)]
    assert np.array_equal(p["cam"], cam)                    # the model ran on the camera rays the library forms
    same, ratio = PM.compare(p, plain, fragile, spread)
    ok = ~fragile
    print("mesh texture model / %s / %s / %s%s: fragile %.2f %%, largest ratio %.3f of %.3f allowed; mismatching outcomes %d" % (
        camera, "half" if half else "float", material, " / odd" if odd else "", 100 * fragile.mean(), ratio, M.GPU_FACTOR,
        np.count_nonzero((p["length"] != plain["length"])[ok] | (p["escaped"] != plain["escaped"])[ok])))
    assert fragile.mean() <= M.FRAGILE_CAP
    assert same
    assert ratio <= M.GPU_FACTOR
    assert set(np.unique(p["escaped"]).tolist()) == {0, 1, 2} and p["length"].max() >= 4


# ---- 7. feature buffers

@pytest.mark.parametrize("name", ["nearest_repeat", "bilinear_clamp"])
def test_feature_albedo_is_colour_times_the_hooks_texel(ptmi_lib, name):
    P = ptmi_lib
    colour = F32((0.8, 0.7, 0.5))
    r = _renderer(P, F.scene(name, colour=tuple(colour)), "none", aa=0.0, fov=ZOOM)
    try:
        feats = r.feature_buffers()
        u, v = PM.all_pixels()
        cam = r.trace_paths(u, v, np.zeros(len(u), np.uint32))["cam"]
        # the centre ray as start_path forms it: normalise((camx, camy, -1)) = v * (1 / sqrtf(dot(v, v))), every operation binary32
        x, y = cam[:, 0].astype(F32), cam[:, 1].astype(F32)
        inv = F32(1.0) / np.sqrt((x * x + y * y) + F32(1.0), dtype=F32)
        d = np.stack([x * inv, y * inv, -inv], -1).astype(F32)
        t, obj, tri, uv, bgr = r.mesh_texel(np.zeros_like(d), d)
    finally:
        r.close()
    plain = _renderer(P, F.scene(name, colour=tuple(colour), textures=False), "none", aa=0.0, fov=ZOOM)
    try:
        before = plain.feature_buffers()
    finally:
        plain.close()
    assert all(feats[k].tobytes() == before[k].tobytes() for k in ("object_id", "depth", "normal"))
    assert np.array_equal(feats["object_id"].ravel(), obj) and np.array_equal(_bits(feats["depth"].ravel()), _bits(t))
    textured = obj >= 1
    assert textured.sum() > 300 and len(np.unique(bgr[textured], axis=0)) >= 8
    want = bgr * colour[::-1][None, :]                               # albedo is B, G, R: colour.B x texel.B, ...
    got = feats["albedo"].reshape(-1, 3)
    wrong = (_bits(got) != _bits(want)).any(axis=1) & textured
    print("%s: %d pixels on textured meshes, %d albedo values differ from colour x texel" % (name, textured.sum(), wrong.sum()))
    assert not wrong.any()
    assert np.array_equal(_bits(got[~textured]), _bits(before["albedo"].reshape(-1, 3)[~textured]))


# ---- 8. the guides, the camera, sharing and the memo

def test_guides_at_zero_and_guided_twins(ptmi_lib):
    P = ptmi_lib
    scene = F.scene("bilinear_repeat", ("diffuse", "diffuse", "emissive")) + [
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
    for alpha, beta in ((0.0, 0.5), (0.5, 0.0), (0.45, 0.45)):
        r = _renderer(P, scene, "moved", fov=ZOOM)
        try:
            if alpha:
                r.set_env_guide(sky, rows=8, cols=16, alpha=alpha)
            if beta:
                r.set_light_guide(beta=beta)
            r.init_render_settings(seed=PM.SEED + 1, samples_per_step=1, aa_noise_scale=PM.AA_SCALE, fov_degrees=ZOOM)
            rec, st = _step(P, r)
            p = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), st.first_sample, np.uint32))
            assert np.array_equal(rec["pathLength"], p["length"])
            got = np.stack([rec["r"], rec["g"], rec["b"]], -1)
            esc = p["escaped"] == 1
            assert esc.sum() > 100 and np.array_equal(_bits(got[esc]), _bits(_radiance(p)[esc]))
            assert np.count_nonzero(p["escaped"] == 2) > 0
        finally:
            r.close()


def test_uvs_follow_a_new_pose_without_allocating(ptmi_lib):
    P = ptmi_lib
    scene = F.scene("bilinear_repeat", ("diffuse", "refractive", "emissive")) + _extras()
    r = _renderer(P, scene, "none", spp=2, ipb=1)
    try:
        _step(P, r)
        first = [r.mesh_texture_info(k) for k in range(3)]
        r.set_camera(**PM.CAMERAS["moved"])
        rec, st = _step(P, r)
        paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 3, np.uint32))
        feats = r.feature_buffers()
        assert [r.mesh_texture_info(k) for k in range(3)] == first                                # nothing allocated, nothing lost
    finally:
        r.close()
    assert [i["device_bytes"] for i in first] == [0, 24 * 320 + 16 * 15, 24 + 16]
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


def test_sharing_and_memo_on_a_textured_scene(ptmi_lib):
    P = ptmi_lib
    scene = F.scene("bilinear_repeat", ("diffuse", "refractive", "emissive")) + _extras()

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
