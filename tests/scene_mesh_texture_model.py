"""The float64 path model of a scene whose meshes may carry textures (pt_set_mesh_texture) -- test infrastructure only.

tests/scene_mesh_normals_model.py restates scene_poly_model.trace with the shading normal.  This file RESTATES that function -- the
same expressions in the same order with the same random draws -- with rules 1-5 of include/ptmi.h's texture section where the hit
row belongs to a textured mesh.  On a scene without textures no extra draw is made and the result equals
scene_mesh_normals_model.trace exactly, perturbed runs included (tests/test_scene_mesh_texture_model.py).

What a texture adds to a bounce, written here on its own (it shares nothing with csrc/pt_mesh.h):
  * a, b by the triangle test's expressions on the ray that hit (pv, tv and qv perturbed as poly_hit perturbs them), c = 1 - a - b;
  * (s, t) = c uv0 + a uv1 + b uv2 (perturbed); the wrap; (0, 0) the image's bottom-left corner, rows stored top to bottom;
  * the BILINEAR lookup with texel centres at half-integers (perturbed), indices wrapped or clamped;
  * the texel multiplies the row's colour before the material branch: the diffuse factor, the tint of a refracted ray only, the
    emitted radiance; a mirror takes none of the steps.
The model's cases use BILINEAR only: it is continuous across texel boundaries and across the wrap, so it adds no decision and no
`choice` flag; NEAREST is pinned bit for bit by tests/mesh_texture_main.cpp instead.
"""
import functools

import numpy as np

from tests import mesh_texture_fixtures as F
from tests import scene_mesh_model as MM
from tests import scene_mesh_normals_model as NM
from tests import scene_model as M
from tests import scene_poly_model as PM

DIFFUSE, SPECULAR, REFRACTIVE, EMISSIVE = PM.DIFFUSE, PM.SPECULAR, PM.REFRACTIVE, PM.EMISSIVE
DISC, TRIANGLE = PM.DISC, PM.TRIANGLE
FLIPPED = PM.FLIPPED
FALLBACK, DROPPED, GUARDED = NM.FALLBACK, NM.DROPPED, NM.GUARDED
MIN_LEN2 = NM.MIN_LEN2
REPEAT, CLAMP = 0, 1
MUTATIONS = ("no_texture", "flip_t", "swap_st")      # the texture left out; t not turned upside down; s and t exchanged

_dot, _perturb = M._dot, M._perturb


def corner_uvs(objects):
    """(textured (rows,), uv (rows, 3, 2) float64, image (rows,), [(image float64 (H, W, 3) B,G,R, wrap)]) over the expanded table of
    tests/scene_mesh_model.expand: the (s, t) of the three corners of every triangle of a mesh that has "texture" (per vertex, or
    per corner with "uv_indices"), and which image the row looks up."""
    textured, uv, image, images = [], [], [], []
    for o in objects:
        nt = len(o["triangles"]) if o["shape"] == "mesh" else 1
        if o["shape"] != "mesh" or o.get("texture") is None:
            textured += [False] * nt
            uv += [np.zeros((3, 2))] * nt
            image += [-1] * nt
            continue
        assert o.get("texture_filter", "bilinear") in ("bilinear", 1), "the model looks up bilinear only"
        idx = np.asarray(o["triangles"] if o.get("uv_indices") is None else o["uv_indices"])
        q = np.asarray(o["uvs"], np.float32).astype(np.float64)
        textured += [True] * nt
        uv += list(q[idx])
        image += [len(images)] * nt
        images.append((np.asarray(o["texture"], np.float32).astype(np.float64), CLAMP if o.get("texture_wrap", "repeat") in ("clamp", 1) else REPEAT))
    return np.array(textured, bool), np.array(uv, np.float64), np.array(image), images


def bilinear(img, wrap, s, t, mutation=None):
    """The B,G,R texel at (s, t) in float64: rules 3 and 4 for the BILINEAR filter."""
    if mutation == "swap_st":
        s, t = t, s
    H, W = img.shape[:2]
    if wrap == CLAMP:
        sw, tw = np.clip(s, 0.0, 1.0), np.clip(t, 0.0, 1.0)
    else:
        sw, tw = s - np.floor(s), t - np.floor(t)
    down = tw if mutation == "flip_t" else 1.0 - tw
    X, Y = sw * W - 0.5, down * H - 0.5
    c0, r0 = np.floor(X), np.floor(Y)
    fx, fy = (X - c0)[:, None], (Y - r0)[:, None]
    ix = (lambda i, n: np.clip(i, 0, n - 1)) if wrap == CLAMP else (lambda i, n: np.mod(i, n))
    c0, c1, r0, r1 = ix(c0.astype(int), W), ix(c0.astype(int) + 1, W), ix(r0.astype(int), H), ix(r0.astype(int) + 1, H)
    top = img[r0, c0] + fx * (img[r0, c1] - img[r0, c0])
    bot = img[r1, c0] + fx * (img[r1, c1] - img[r1, c0])
    return top + fy * (bot - top)


def trace(scene, normals, textures, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0), rng=None, mutation=None):
    """scene_mesh_normals_model.trace, restated; `normals` = its corner_normals() and `textures` = corner_uvs() of the objects the
    table was expanded from.  The same inputs and outputs.  `mutation` (one of MUTATIONS) gets a rule wrong: the comparison must
    notice."""
    smooth, corner = normals
    textured, corner_uv, image_of, images = textures
    n = len(u)
    D = opt["max_path_length"]
    half = opt["samples_half"]
    k0, k1 = opt["seed"] & 0xFFFFFFFF, opt["seed"] >> 32
    pixel = np.asarray(u, dtype=np.uint64) | (np.asarray(v, dtype=np.uint64) << np.uint64(16))
    sample = np.asarray(sample, dtype=np.uint64)
    stop, ri = opt["stop_prob"], opt["refractive_index"]
    env = np.asarray(env, dtype=np.float64)

    focus = np.stack([np.asarray(cam[:, 0], np.float64), np.asarray(cam[:, 1], np.float64), -np.ones(n)], -1)
    a = float(np.float32(camera.get("lens_radius", 0.0))) if camera else 0.0
    if a > 0:
        F = float(np.float32(camera["focus_distance"]))
        w = M.philox(pixel, sample, M.LENS_BLOCK, 0x5054, k0, k1)
        x1, x2 = M._uniform(w[0], half), M._uniform(w[1], half)
        o = np.stack([a * np.sqrt(x1) * np.cos(2 * np.pi * x2), a * np.sqrt(x1) * np.sin(2 * np.pi * x2), np.zeros(n)], -1)
        o = _perturb(o, rng)
        d = F * focus - o
    else:
        o = np.zeros((n, 3))
        d = focus
    d = _perturb(d / np.linalg.norm(d, axis=-1, keepdims=True), rng)
    frame = None
    if M._has_pose(camera):
        p, r, up, f = M.basis(camera)
        frame = (r, up, f)
        o = p + o[:, 0:1] * r + o[:, 1:2] * up - o[:, 2:3] * f
        d = d[:, 0:1] * r + d[:, 1:2] * up - d[:, 2:3] * f

    out = dict(length=np.zeros(n, np.uint32), escaped=np.zeros(n, np.uint32), dir=np.zeros((n, 3)), uv=np.zeros((n, 2)),
               throughput=np.zeros((n, 3)), radiance=np.zeros((n, 3)), hits=np.full((n, D), -1, np.int8),
               choice=np.zeros((n, D), np.int8), risk=np.zeros(n, bool))
    colour = scene["colour"].astype(np.float64)
    centre = scene["centre"].astype(np.float64)
    is_poly = scene["shape"] >= TRIANGLE
    edge1 = np.zeros((len(scene), 3))
    edge2 = np.zeros((len(scene), 3))
    for i in np.flatnonzero(is_poly):
        edge1[i], edge2[i] = PM._edges(scene[i])
    cpath = None
    if rng is not None and frame is not None:
        uniq, uid = np.unique(centre, axis=0, return_inverse=True)
        cpath = (p + _perturb(np.broadcast_to(uniq - p, (n,) + uniq.shape), rng))[:, uid.ravel()]
    normal = scene["normal"].astype(np.float64)
    idx = np.arange(n)
    T = np.ones((n, 3))
    for depth in range(D):
        if idx.size == 0:
            break
        w = M.philox(pixel[idx], sample[idx], 1 + depth, 0x5054, k0, k1)
        rr = 1.0
        if depth >= opt["roulette_depth"]:
            dead = M._uniform(w[0], half) <= stop
            out["length"][idx[dead]] = max(depth, 1)
            keep = ~dead
            idx, o, d, T, w = idx[keep], o[keep], d[keep], T[keep], tuple(x[keep] for x in w)
            rr = 1.0 / (1.0 - stop)
        best, t = PM._nearest(scene, o, d, None, rng, None if cpath is None else cpath[idx])
        hit = best >= 0
        out["hits"][idx, depth] = best
        shape = np.where(hit, scene["shape"][np.maximum(best, 0)], -1)
        mat = np.where(hit, scene["material"][np.maximum(best, 0)], -1)
        col_hit = colour[np.maximum(best, 0)]                    # rule 5: the row's colour, times the texel on a textured mesh
        tx = hit & textured[np.maximum(best, 0)] & (mat != SPECULAR)
        if tx.any() and mutation != "no_texture":                # rules 1-4, from the ray that hit (o is its origin)
            k = np.flatnonzero(tx)
            bk, ok, dk = best[k], o[k], d[k]
            v0 = centre[bk] if cpath is None else cpath[idx[k], bk]
            e1, e2 = edge1[bk], edge2[bk]
            with np.errstate(divide="ignore", invalid="ignore"):
                pv = _perturb(np.cross(dk, e2), rng)
                inv = 1.0 / _dot(pv, e1)
                tv = _perturb(ok - v0, rng)
                ba = _dot(tv, pv) * inv
                qv = _perturb(np.cross(tv, e1), rng)
                bb = _dot(dk, qv) * inv
                bc = (1.0 - ba) - bb
            cu = corner_uv[bk]
            st = _perturb(bc[:, None] * cu[:, 0] + ba[:, None] * cu[:, 1] + bb[:, None] * cu[:, 2], rng)
            bgr = np.zeros((len(k), 3))
            for im in np.unique(image_of[bk]):
                q = image_of[bk] == im
                bgr[q] = bilinear(images[im][0], images[im][1], st[q, 0], st[q, 1], mutation)
            col_hit = col_hit.copy()
            col_hit[k] = col_hit[k] * _perturb(bgr, rng)[:, ::-1]   # R x texel.R, G x texel.G, B x texel.B
        for sel, code in ((~hit, 1), (mat == EMISSIVE, 2)):
            if sel.any():
                j = idx[sel]
                Te = T[sel] * rr
                out["length"][j] = depth + 1
                out["escaped"][j] = code
                out["dir"][j] = d[sel]
                out["throughput"][j] = Te
                if code == 1:
                    out["uv"][j] = M._dir_to_uv(d[sel])
                    out["radiance"][j] = env * Te
                else:
                    out["radiance"][j] = col_hit[sel] * Te
        go = hit & (mat != EMISSIVE)
        idx, o, d, T, best, t, shape, mat = idx[go], o[go], d[go], T[go], best[go], t[go], shape[go], mat[go]
        w = tuple(x[go] for x in w)
        col_hit = col_hit[go]
        if idx.size == 0:
            break
        t = _perturb(t, rng)
        hp = _perturb(o + d * t[:, None], rng)
        cbest = centre[best] if cpath is None else cpath[idx, best]
        radial = hp - cbest
        flat = shape >= DISC                                     # a disc or a polygon: the stored normal
        with np.errstate(divide="ignore", invalid="ignore"):
            nrm = np.where(flat[:, None], normal[best], radial / np.linalg.norm(radial, axis=-1, keepdims=True))
        nrm = _perturb(nrm, rng)
        choice = np.zeros(len(idx), np.int8)
        poly = shape >= TRIANGLE
        sm = smooth[best]
        ng = normal[best]                                        # the geometric normal of a polygon's row
        if sm.any():                                             # rules 1-4, from the ray that hit (o is still its origin)
            k = np.flatnonzero(sm)
            bk, ok, dk, g = best[k], o[k], d[k], ng[k]
            e1, e2 = edge1[bk], edge2[bk]
            with np.errstate(divide="ignore", invalid="ignore"):
                pv = _perturb(np.cross(dk, e2), rng)
                inv = 1.0 / _dot(pv, e1)
                tv = _perturb(ok - cbest[k], rng)
                ba = _dot(tv, pv) * inv
                qv = _perturb(np.cross(tv, e1), rng)
                bb = _dot(dk, qv) * inv
                bc = (1.0 - ba) - bb
                cn = corner[bk]
                mm = _perturb(bc[:, None] * cn[:, 0] + ba[:, None] * cn[:, 1] + bb[:, None] * cn[:, 2], rng)
                l2 = _dot(mm, mm)
                fallback = ~(l2 > MIN_LEN2)
                ns = np.where(fallback[:, None], g, mm / np.sqrt(np.where(fallback, 1.0, l2))[:, None])
            ns = _perturb(ns, rng)
            if mutation != "no_orientation":
                ns = np.where((_dot(ns, g) < 0)[:, None], -ns, ns)
            dropped = (_dot(ns, dk) > 0) != (_dot(g, dk) > 0)
            if mutation == "no_side_test":
                dropped &= False
            nrm[k] = np.where(dropped[:, None], g, ns)
            choice[k] += (FALLBACK * fallback + DROPPED * dropped).astype(np.int8)
        if poly.any():                                           # two-sided: the normal faces the ray (glass flips below, as for every object)
            flip = poly & (mat != REFRACTIVE) & (_dot(nrm, d) > 0)
            nrm = np.where(flip[:, None], -nrm, nrm)
            choice[flip] += FLIPPED
        new_d = np.zeros_like(d)
        col = col_hit

        m = mat == DIFFUSE
        if m.any():
            nn = nrm[m] if frame is None else np.stack([nrm[m] @ frame[0], nrm[m] @ frame[1], -(nrm[m] @ frame[2])], -1)
            u1, u2 = M._uniform(w[1][m], half), M._uniform(w[2][m], half)
            xmajor = np.abs(nn[:, 0]) > np.abs(nn[:, 1])
            mj = np.where(xmajor, nn[:, 0], nn[:, 1])
            inv = 1.0 / np.sqrt(mj * mj + nn[:, 2] ** 2)
            aa, bb = nn[:, 2] * inv, mj * inv
            zero = np.zeros(len(nn))
            rx = np.where(xmajor[:, None], np.stack([-aa, zero, bb], -1), np.stack([zero, aa, -bb], -1))
            ry = np.cross(nn, rx)
            rad = np.sqrt(1.0 - u1 * u1)
            dn = rx * (np.cos(2 * np.pi * u2) * rad)[:, None] + ry * (np.sin(2 * np.pi * u2) * rad)[:, None] + nn * u1[:, None]
            T[m] = T[m] * col[m] * (_dot(dn, nn) * rr)[:, None]
            new_d[m] = dn if frame is None else dn[:, 0:1] * frame[0] + dn[:, 1:2] * frame[1] - dn[:, 2:3] * frame[2]
            choice[m] += np.where(xmajor, 2, 1).astype(np.int8)

        m = mat == SPECULAR
        if m.any():
            nn, di = nrm[m], d[m]
            vv = di - nn * (2.0 * _dot(di, nn))[:, None]
            if sm[m].any():                                      # rule 6: a mirror never reflects into its own surface
                gf = np.where((_dot(ng[m], di) > 0)[:, None], -ng[m], ng[m])
                guarded = sm[m] & (_dot(vv, gf) <= 0) & (mutation != "no_mirror_guard")
                vv = np.where(guarded[:, None], di - gf * (2.0 * _dot(di, gf))[:, None], vv)
                choice[m] += (GUARDED * guarded).astype(np.int8)
            new_d[m] = vv / np.linalg.norm(vv, axis=-1, keepdims=True)
            T[m] = T[m] * rr

        m = mat == REFRACTIVE
        if m.any():
            nn, di = nrm[m].copy(), d[m]
            uu = M._uniform(w[1][m], half)
            r0 = ((1.0 - ri) / (1.0 + ri)) ** 2
            inside = _dot(nn, di) > 0
            nn[inside] = -nn[inside]
            eta = np.where(inside, ri, 1.0 / ri)
            cost1 = -_dot(nn, di)
            cost2 = 1.0 - eta * eta * (1.0 - cost1 * cost1)
            rprob = r0 + (1.0 - r0) * (1.0 - cost1) ** 5
            refracted = (cost2 > 0) & (uu > rprob)
            bent = di * eta[:, None] + nn * (eta * cost1 - np.sqrt(np.maximum(cost2, 0.0)))[:, None]
            mirrored = di + nn * (2.0 * cost1)[:, None]
            vv = np.where(refracted[:, None], bent, mirrored)
            new_d[m] = vv / np.linalg.norm(vv, axis=-1, keepdims=True)
            T[m] = T[m] * np.where(refracted[:, None], col[m], 1.0) * (1.15 * rr)
            choice[m] += np.where(refracted, 3, 4).astype(np.int8)

        out["choice"][idx, depth] = choice
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # (a polygon's radius is 0: its row is replaced below)
            risk = M._self_hit_risk(o, d, t, hp, nrm, new_d, radial, shape == DISC, scene["radius"][best].astype(np.float64))
            if poly.any():
                # in the frame the kernels trace in (scene_poly_model.trace); with the geometric normal on a smooth mesh
                pt = (lambda x: x) if frame is None else (lambda x: np.stack([(x - p) @ frame[0], (x - p) @ frame[1], -((x - p) @ frame[2])], -1))
                dr = (lambda x: x) if frame is None else (lambda x: np.stack([x @ frame[0], x @ frame[1], -(x @ frame[2])], -1))
                plane = np.where(sm[:, None], ng, nrm)
                risk = np.where(poly, PM._self_hit_risk_poly(pt(o), dr(d), t, pt(hp), dr(plane), dr(new_d), pt(cbest), dr(edge1[best]),
                                                             dr(edge2[best])), risk)
        out["risk"][idx] |= risk
        o, d = hp, _perturb(new_d, rng)
        if depth + 1 >= D:
            out["length"][idx] = D
    return out


def analyse(scene, normals, textures, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0)):
    """scene_mesh_normals_model.analyse over this module's trace: (plain result, fragile, spread)."""
    plain = trace(scene, normals, textures, camera, opt, u, v, sample, cam, env)
    n = len(u)
    rng = np.random.default_rng(0x5CE9E)
    K = M.K_RUNS
    tiled = trace(scene, normals, textures, camera, opt, np.tile(u, K), np.tile(v, K), np.tile(sample, K), np.tile(cam, (K, 1)), env, rng=rng)
    fragile = plain["risk"].copy()
    spread = dict(dir=np.zeros(n), uv=np.zeros(n), throughput=np.zeros(n))
    for k in range(K):
        run = {key: val[k * n:(k + 1) * n] for key, val in tiled.items()}
        fragile |= (run["length"] != plain["length"]) | (run["escaped"] != plain["escaped"])
        fragile |= np.any(run["hits"] != plain["hits"], axis=1) | np.any(run["choice"] != plain["choice"], axis=1)
        for key, val in M.deviation(run, plain).items():
            spread[key] = np.maximum(spread[key], val)
    return plain, fragile, spread


# ---- the cases: scene_mesh_normals_model's eight -- its smooth ball, glass, mirror and diffuse in turn, over the flat height field,
# the lamp and the mirror sphere -- with the 5 x 3 image of tests/mesh_texture_fixtures.py on the ball (longitude and latitude twice
# round, REPEAT; per-corner indices in the odd cases, the lower half shifted: a seam) and on the field (planar, over [-0.5, 1.5],
# CLAMP).  Texture coordinates belong to the mesh: they are made in camera space and no camera moves them.

W, H = PM.W, PM.H
SAMPLE, STRIDE = NM.SAMPLE, NM.STRIDE
CAMERAS = PM.CAMERAS
CASES = NM.CASES


def _textures(material, odd):
    """{row of the mesh table: texture keys} from the camera-space scene."""
    objs = NM.camera_scene(material, odd)
    ball, field = objs[0], objs[2]
    v = np.asarray(ball["vertices"], np.float64)
    uvs = F.spherical_uvs(v, NM.BALL_CENTRE, 2.0)
    keys = {0: dict(texture=F.image_5x3(), uvs=uvs, texture_filter="bilinear", texture_wrap="repeat"),
            2: dict(texture=F.image_5x3(), uvs=F.planar_uvs(field["vertices"], -0.5, 1.5), texture_filter="bilinear", texture_wrap="clamp")}
    if odd:
        t = np.asarray(ball["triangles"])
        low = v[t][:, :, 1].mean(axis=1) < NM.BALL_CENTRE[1]
        idx = t.astype(np.uint32).copy()
        idx[low] += np.uint32(len(v))
        keys[0].update(uvs=np.concatenate([uvs, np.float32(uvs + np.float32(0.37))]), uv_indices=idx)
    return keys


def world_scene(camera_name, material, odd, textures=True):
    """scene_mesh_normals_model.world_scene with the textures attached (textures=False: that scene as it is)."""
    out = NM.world_scene(camera_name, material, odd)
    if textures:
        for row, keys in _textures(material, odd).items():
            out[row].update(keys)
    return out


@functools.lru_cache(maxsize=None)
def case(camera_name, samples_half, material, odd):
    """The GPU test's inputs and the model's analysis of them: (u, v, sample, cam, plain, fragile, spread)."""
    u, v = MM.pixels()
    ss = np.full(len(u), SAMPLE, np.uint32)
    cam = PM.oracle_cam(SAMPLE)[::STRIDE]
    objs = world_scene(camera_name, material, odd)
    plain, fragile, spread = analyse(MM.stored(objs), NM.corner_normals(objs), corner_uvs(objs), CAMERAS[camera_name],
                                     PM.case_options(samples_half), u, v, ss, cam, PM.ENV)
    return u, v, ss, cam, plain, fragile, spread
