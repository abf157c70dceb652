"""The float64 path model of a scene whose meshes may carry vertex normals (pt_set_mesh_normals) -- test infrastructure only.

tests/scene_mesh_model.py models a mesh as its triangles, rows of tests/scene_poly_model.py's table.  This file keeps that
expansion and RESTATES scene_poly_model.trace -- the same expressions in the same order with the same random draws -- with the
shading normal of include/ptmi.h (rules 1-6) where the hit row belongs to a mesh with normals.  On a scene without normals no
extra draw is made and the result equals scene_poly_model.trace exactly, perturbed runs included
(tests/test_scene_mesh_normals_model.py).

What the shading normal adds to a bounce:
  * a, b by the triangle test's own expressions on the ray that hit (pv, tv and qv perturbed as poly_hit perturbs them), c = 1 - a - b,
    m = c n0 + a n1 + b n2 (perturbed), ns = m / |m| where dot(m, m) > 1e-12, else the stored normal ng (FALLBACK);
  * orientation: dot(ns, ng) < 0 turns ns; side: a ns that puts the ray on the other side of the surface than ng does is
    replaced by ng (DROPPED);
  * the bounce continues as for any polygon with n = ns; a mirror's vector that points into the surface, dot(v, ng_f) <= 0 with
    ng_f the stored normal facing the ray, is formed again with ng_f (GUARDED).
FALLBACK, DROPPED and GUARDED are added to the bounce's `choice`, so a perturbed run that decides one of them differently marks
the path fragile, as a changed hit does.  The ray that leaves a triangle can meet it again only through the rounding of the hit
point, whatever normal shaded it: the self-hit risk (scene_poly_model._self_hit_risk_poly) is taken with the GEOMETRIC normal.  A
diffuse direction below the geometric surface (the shading-normal terminator) is no special case: it leaves the triangle like any
other and meets the mesh again, in the model as on the device.
"""
import functools

import numpy as np

from tests import scene_mesh_model as MM
from tests import scene_model as M
from tests import scene_poly_model as PM

DIFFUSE, SPECULAR, REFRACTIVE, EMISSIVE = PM.DIFFUSE, PM.SPECULAR, PM.REFRACTIVE, PM.EMISSIVE
DISC, TRIANGLE = PM.DISC, PM.TRIANGLE
FLIPPED = PM.FLIPPED
FALLBACK, DROPPED, GUARDED = 16, 32, 64      # added to a bounce's `choice` (int8: 4 + 8 + 16 + 32 + 64 = 124 at most)
MIN_LEN2 = 1e-12
MUTATIONS = ("no_orientation", "no_side_test", "no_mirror_guard")

_dot, _perturb = M._dot, M._perturb


def unit32(n):
    """Each row n / sqrtf(dot(n, n)) as the library normalises a given normal: every operation a rounded binary32, the sum left
    to right."""
    f = np.float32
    n = np.asarray(n, f)
    dd = f(f(f(n[:, 0] * n[:, 0]) + f(n[:, 1] * n[:, 1])) + f(n[:, 2] * n[:, 2]))
    return f(n / np.sqrt(dd)[:, None])


def corner_normals(objects):
    """(smooth (rows,), corner (rows, 3, 3) float64) over the expanded table of tests/scene_mesh_model.expand: the unit normals of
    the three corners of every triangle of a mesh that has "normals" (per vertex, or per corner with "normal_indices")."""
    smooth, corner = [], []
    for o in objects:
        if o["shape"] != "mesh":
            smooth.append(False)
            corner.append(np.zeros((3, 3)))
            continue
        nt = len(o["triangles"])
        if o.get("normals") is None:
            smooth += [False] * nt
            corner += [np.zeros((3, 3))] * nt
            continue
        idx = np.asarray(o["triangles"] if o.get("normal_indices") is None else o["normal_indices"])
        n = unit32(o["normals"]).astype(np.float64)
        smooth += [True] * nt
        corner += list(n[idx])
    return np.array(smooth, bool), np.array(corner, np.float64)


def trace(scene, normals, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0), rng=None, mutation=None):
    """scene_poly_model.trace over a stored expanded table, restated; `normals` = corner_normals() of the objects it was expanded
    from.  The same inputs and outputs.  `mutation` (one of MUTATIONS) leaves a rule out: the comparison must notice."""
    smooth, corner = normals
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
                    out["radiance"][j] = colour[best[sel]] * Te
        go = hit & (mat != EMISSIVE)
        idx, o, d, T, best, t, shape, mat = idx[go], o[go], d[go], T[go], best[go], t[go], shape[go], mat[go]
        w = tuple(x[go] for x in w)
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
        col = colour[best]

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


def analyse(scene, normals, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0)):
    """scene_poly_model.analyse over this module's trace: (plain result, fragile, spread)."""
    plain = trace(scene, normals, camera, opt, u, v, sample, cam, env)
    n = len(u)
    rng = np.random.default_rng(0x5CE9E)
    K = M.K_RUNS
    tiled = trace(scene, normals, camera, opt, np.tile(u, K), np.tile(v, K), np.tile(sample, K), np.tile(cam, (K, 1)), env, rng=rng)
    fragile = plain["risk"].copy()
    spread = dict(dir=np.zeros(n), uv=np.zeros(n), throughput=np.zeros(n))
    for k in range(K):
        run = {key: val[k * n:(k + 1) * n] for key, val in tiled.items()}
        fragile |= (run["length"] != plain["length"]) | (run["escaped"] != plain["escaped"])
        fragile |= np.any(run["hits"] != plain["hits"], axis=1) | np.any(run["choice"] != plain["choice"], axis=1)
        for key, val in M.deviation(run, plain).items():
            spread[key] = np.maximum(spread[key], val)
    return plain, fragile, spread


# ---- the cases.  Camera space: x right, y up, the view along -z.  Two meshes: a smooth icosphere(2), 24 pixels across so that a
# seventh of the camera rays meet it first, over scene_mesh_model's flat height field; its lamp and its mirror sphere.

W, H = PM.W, PM.H
SAMPLE, STRIDE = MM.SAMPLE, MM.STRIDE
CAMERAS = PM.CAMERAS
BALL_CENTRE, BALL_RADIUS = (0.03, 0.0, -0.42), 0.12
# (camera, samples_half, the ball's material, odd): four cameras x both precisions; the ball glass, mirror and diffuse in turn, so
# that every material of a smooth mesh meets both precisions; odd = every second winding reversed and a creased ring of edges
CASES = [(c, h, ("refractive", "specular", "diffuse")[(2 * i + j) % 3], (i + j) % 2 == 1)
         for i, c in enumerate(CAMERAS) for j, h in enumerate((False, True))]


def ball(odd):
    """(vertices, triangles, normals, normal_indices or None) in camera space: the radial normals (v - centre) / radius per vertex;
    odd: windings of odd triangles reversed and per-corner indices into 2 V normals that crease the ring of edges between the
    triangles above the centre and those below (tests/mesh_normals_fixtures.py's odd sphere, here)."""
    v, t = MM.icosphere(2, BALL_RADIUS, BALL_CENTRE)
    radial = (v - np.asarray(BALL_CENTRE)) / BALL_RADIUS
    if not odd:
        return v, t, radial, None
    t = t.copy()
    t[1::2] = t[1::2][:, [0, 2, 1]]
    low = v[t][:, :, 1].mean(axis=1) < BALL_CENTRE[1]
    ring = np.zeros(len(v), bool)
    ring[np.intersect1d(t[low].ravel(), t[~low].ravel())] = True
    below = radial.copy()
    below[ring] += np.array([0.0, -0.6, 0.0])                  # not unit on purpose: the library normalises
    idx = t.astype(np.uint32).copy()
    idx[low] += np.uint32(len(v))
    return v, t, np.concatenate([radial, below]), idx


def camera_scene(material, odd):
    v, t, n, idx = ball(odd)
    o = {"shape": "mesh", "material": material, "colour": (0.9, 0.95, 0.9), "vertices": v, "triangles": t, "normals": n}
    if idx is not None:
        o["normal_indices"] = idx
    return [o] + [dict(x) for x in MM.SCENE[1:]]


def world_scene(camera_name, material, odd):
    """camera_scene placed in front of the camera (scene_mesh_model.world_scene's rule for points); a normal is a direction,
    x r + y u - z f, rounded to the binary32 the library is given.  A list of dicts for Renderer.set_scene."""
    camera = CAMERAS[camera_name]
    pose = M._has_pose(camera)
    if pose:
        p, r, up, f = M.basis(camera)
    out = []
    for o in camera_scene(material, odd):
        if o["shape"] == "mesh":
            c = np.asarray(o["vertices"], np.float64)
            o["vertices"] = np.float32(p + c[:, 0:1] * r + c[:, 1:2] * up - c[:, 2:3] * f) if pose else np.float32(c)
            if "normals" in o:
                c = np.asarray(o["normals"], np.float64)
                o["normals"] = np.float32(c[:, 0:1] * r + c[:, 1:2] * up - c[:, 2:3] * f) if pose else np.float32(c)
        elif "vertices" in o:
            c = np.asarray(o["vertices"], np.float64)
            c = np.float32(p + c[:, 0:1] * r + c[:, 1:2] * up - c[:, 2:3] * f) if pose else np.float32(c)
            o["vertices"] = tuple(tuple(float(x) for x in row) for row in c)
        else:
            c = np.asarray(o["centre"], np.float64)
            o["centre"] = tuple(float(x) for x in (np.float32(p + c[0] * r + c[1] * up - c[2] * f) if pose else np.float32(c)))
        out.append(o)
    return out


@functools.lru_cache(maxsize=None)
def case(camera_name, samples_half, material, odd):
    """The GPU test's inputs and the model's analysis of them: (u, v, sample, cam, plain, fragile, spread)."""
    u, v = MM.pixels()
    ss = np.full(len(u), SAMPLE, np.uint32)
    cam = PM.oracle_cam(SAMPLE)[::STRIDE]
    objs = world_scene(camera_name, material, odd)
    plain, fragile, spread = analyse(MM.stored(objs), corner_normals(objs), CAMERAS[camera_name], PM.case_options(samples_half),
                                     u, v, ss, cam, PM.ENV)
    return u, v, ss, cam, plain, fragile, spread
