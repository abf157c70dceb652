"""The float64 path model of tests/scene_model.py with triangles and parallelograms (pt_set_scene_ex) -- test infrastructure only.

It reuses scene_model's helpers (Philox, the camera basis, the perturbation, the self-hit rule, deviation, compare) and replaces
the two functions a polygon changes: the nearest hit and the path loop.  On a table of spheres and discs both are scene_model's own
expressions in the same order with the same random draws, so the result equals scene_model.trace exactly, perturbed runs included
(tests/test_scene_poly_model.py).

A polygon v0 + a e1 + b e2 is tested as include/ptmi.h states it (Moeller-Trumbore, two-sided).  Conditioning: the perturbed
runs multiply tv = o - v0, pv = cross(d, e2) and qv = cross(tv, e1), component by component, by 1 + delta, which moves a, b and
t by a few binary32 ulps of the TERMS they are summed from -- a ray within rounding of an edge (the shared edge of two walls) or
of the plane changes its hit among the runs and is fragile.  The ray that leaves a polygon can meet it again only through the
rounding of the hit point: _self_hit_risk_poly, the disc rule with the error of a Moeller-Trumbore t.

The cases of the GPU tests (tests/test_gpu_scene_polygons.py) are the tables at the end.
"""
import functools

import numpy as np

from ipu_path_trace_amd import ptmi
from tests import scene_model as M

SPHERE, DISC, TRIANGLE, PARALLELOGRAM = 0, 1, 2, 3
DIFFUSE, SPECULAR, REFRACTIVE, EMISSIVE = M.DIFFUSE, M.SPECULAR, M.REFRACTIVE, M.EMISSIVE
EPS = M.EPS
FLIPPED = 8          # added to a bounce's `choice` where a polygon's normal was turned to face the ray

MUTATIONS = ("no_normal_flip", "no_sum_test", "swap_edges_in_t", "no_eps")

_dot, _perturb = M._dot, M._perturb


def stored_scene_ex(objects):
    """The table as pt_set_scene_ex stores it, without a device: a sphere or disc as scene_model.stored_scene leaves it with
    vertex 0; a polygon with centre = v0, radius 0 and normal = c / sqrtf(dot(c, c)), c = cross(e1, e2), every operation a rounded
    binary32 and the sums left to right.  (On the GPU the tests take Renderer.scene_ex() instead.)"""
    t = ptmi.scene_array_ex(objects).copy()
    f = np.float32
    for o in t:
        if o["shape"] in (TRIANGLE, PARALLELOGRAM):
            v = o["vertex"].astype(f)
            e1, e2 = f(v[1] - v[0]), f(v[2] - v[0])
            c = np.array([f(f(e1[(k + 1) % 3] * e2[(k + 2) % 3]) - f(e1[(k + 2) % 3] * e2[(k + 1) % 3])) for k in range(3)], f)
            cc = f(f(f(c[0] * c[0]) + f(c[1] * c[1])) + f(c[2] * c[2]))
            o["centre"], o["radius"], o["normal"] = v[0], 0, c / np.sqrt(cc)
        else:
            o["vertex"] = 0
            if o["shape"] == DISC:
                n = o["normal"].astype(f)
                d = f(f(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                o["normal"] = n / np.sqrt(d)
            else:
                o["normal"] = 0
    return t


def _edges(ob):
    v = ob["vertex"].astype(np.float32)
    return np.float32(v[1] - v[0]).astype(np.float64), np.float32(v[2] - v[0]).astype(np.float64)   # e1, e2 are binary32 values


def poly_hit(shape, v0, e1, e2, o, d, mutation=None, rng=None):
    """include/ptmi.h's polygon test over arrays of rays: the distance, 0 for a miss."""
    with np.errstate(divide="ignore", invalid="ignore"):
        pv = _perturb(np.cross(d, e2), rng)
        det = pv @ e1
        inv = 1.0 / det
        tv = _perturb(o - v0, rng)
        a = _dot(tv, pv) * inv
        qv = _perturb(np.cross(tv, e1), rng)
        b = _dot(d, qv) * inv
        ok = (det != 0) & (a >= 0) & (a <= 1) & (b >= 0)
        if shape == TRIANGLE:
            if mutation != "no_sum_test":
                ok &= a + b <= 1
        else:
            ok &= b <= 1
        t = (_dot(qv, e1) if mutation == "swap_edges_in_t" else qv @ e2) * inv
        ok &= t > (0.0 if mutation == "no_eps" else EPS)
    return np.where(ok, t, 0.0)


def _nearest(scene, o, d, mutation, rng=None, centres=None):
    """scene_model._nearest with polygons: the same loop, the same draws for a table without them."""
    m = len(o)
    best = np.full(m, -1, dtype=np.int64)
    tbest = np.full(m, np.inf)
    dd = _dot(d, d)
    fb = _perturb(np.ones(m), rng)
    for i in range(len(scene)):
        ob = scene[i]
        c = ob["centre"].astype(np.float64) if centres is None else centres[:, i]
        r2 = float(ob["radius"]) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            if ob["shape"] in (TRIANGLE, PARALLELOGRAM):
                e1, e2 = _edges(ob)
                t = poly_hit(int(ob["shape"]), c, e1, e2, o, d, mutation, rng)
            elif ob["shape"] == DISC:
                nrm = ob["normal"].astype(np.float64)
                denom = d @ nrm
                t = _dot(c - o, nrm) / denom
                ok = (denom != 0) & (t > EPS)
                t = np.where(ok, t, 0.0)
                pc = o + d * t[:, None] - c
                t = np.where(_dot(pc, pc) <= r2, t, 0.0)
            else:
                oc = o - c
                b = _dot(oc, d)
                disc = b * b * fb - dd * (_dot(oc, oc) - r2)
                sq = np.sqrt(np.maximum(disc, 0.0))
                near, far = (-b - sq) / dd, (-b + sq) / dd
                t = np.where(disc >= 0, np.where(2 * near > EPS, near, np.where(2 * far > EPS, far, 0.0)), 0.0)
        # (the mutation that drops a polygon's epsilon drops it here too, or the scene's own test would hide it)
        better = (t > (0.0 if mutation == "no_eps" and ob["shape"] >= TRIANGLE else EPS)) & (t < tbest)
        best[better] = i
        tbest[better] = t[better]
    return best, tbest


def _abs_cross(a, b):
    """Per component, the sum of the magnitudes of the two products a cross product subtracts."""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _self_hit_risk_poly(o, d, t, hp, nrm, new_d, v0, e1, e2):
    """scene_model._self_hit_risk for a polygon, a bound from the number format alone (u = 2^-24 per rounding): the hit point
    o + d t carries 2 u sum |n_k hp_k| of its own along the normal and, along the ray, the error of t = N / det,
    N = dot(e2, cross(tv, e1)), det = dot(e1, cross(d, e2)).  Every term of N has gone through the rounding of tv, a product, the
    cross product's difference, the product by e2 and two sums: 6 u on the sum S_N of the terms' magnitudes; det likewise without
    the first, 5 u S_det; the quotient and the product by it add 2 u t:
        e_t = (6 u S_N + 5 u S_det t) / |det| + 2 u t.
    The leaving ray meets the plane again at off / cos(out): at risk where that can reach the intersection epsilon."""
    u = 2.0 ** -24
    e_pos = 2 * u * np.sum(np.abs(nrm * hp), axis=-1)
    cos_in = np.abs(_dot(nrm, d))
    cos_out = np.maximum(np.abs(_dot(nrm, new_d)), 1e-300)
    s_n = _dot(np.abs(e2), _abs_cross(o - v0, e1))
    s_det = _dot(np.abs(e1), _abs_cross(d, e2))
    det = np.maximum(np.abs(_dot(e1, np.cross(d, e2))), 1e-300)
    e_t = (6 * u * s_n + 5 * u * s_det * t) / det + 2 * u * t
    off = e_pos + e_t * cos_in
    return off / cos_out >= EPS


def trace(scene, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0), rng=None, mutation=None):
    """scene_model.trace over a stored ex table (stored_scene_ex / Renderer.scene_ex()): the same inputs and outputs; a bounce off
    a polygon whose normal was turned to face the ray adds FLIPPED to its `choice`."""
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
        edge1[i], edge2[i] = _edges(scene[i])
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
        best, t = _nearest(scene, o, d, mutation, rng, None if cpath is None else cpath[idx])
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
        if poly.any() and mutation != "no_normal_flip":        # two-sided: the normal faces the ray (glass flips below, as for every object)
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
            mm = np.where(xmajor, nn[:, 0], nn[:, 1])
            inv = 1.0 / np.sqrt(mm * mm + nn[:, 2] ** 2)
            aa, bb = nn[:, 2] * inv, mm * inv
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
                # in the frame the kernels trace in: under a pose the world coordinates carry the camera's position, which the
                # kernels' camera-space values do not
                pt = (lambda x: x) if frame is None else (lambda x: np.stack([(x - p) @ frame[0], (x - p) @ frame[1], -((x - p) @ frame[2])], -1))
                dr = (lambda x: x) if frame is None else (lambda x: np.stack([x @ frame[0], x @ frame[1], -(x @ frame[2])], -1))
                risk = np.where(poly, _self_hit_risk_poly(pt(o), dr(d), t, pt(hp), dr(nrm), dr(new_d), pt(cbest), dr(edge1[best]),
                                                          dr(edge2[best])), risk)
        out["risk"][idx] |= risk
        o, d = hp, _perturb(new_d, rng)
        if depth + 1 >= D:
            out["length"][idx] = D
    return out


def analyse(scene, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0), mutation=None):
    """scene_model.analyse over this module's trace: (plain result, fragile, spread)."""
    plain = trace(scene, camera, opt, u, v, sample, cam, env, mutation=mutation)
    n = len(u)
    rng = np.random.default_rng(0x5CE9E)
    K = M.K_RUNS
    tiled = trace(scene, camera, opt, np.tile(u, K), np.tile(v, K), np.tile(sample, K), np.tile(cam, (K, 1)), env, rng=rng,
                  mutation=mutation)
    fragile = plain["risk"].copy()
    spread = dict(dir=np.zeros(n), uv=np.zeros(n), throughput=np.zeros(n))
    for k in range(K):
        run = {key: val[k * n:(k + 1) * n] for key, val in tiled.items()}
        fragile |= (run["length"] != plain["length"]) | (run["escaped"] != plain["escaped"])
        fragile |= np.any(run["hits"] != plain["hits"], axis=1) | np.any(run["choice"] != plain["choice"], axis=1)
        for key, val in M.deviation(run, plain).items():
            spread[key] = np.maximum(spread[key], val)
    return plain, fragile, spread


compare = M.compare


def first_hit(scene, camera, cam):
    """The noise-free centre ray of every pixel (pt_feature_buffers) whose half-exact camera ray is cam[i]: (object id, depth,
    world normal facing the ray, well conditioned), float64, as tests/features_model.py::model64 forms them; a hit is well
    conditioned by that file's rule: disc / b^2 >= 1e-4 on a sphere, |dot(n, d)| >= 1e-4 on a disc or a polygon."""
    n = len(cam)
    d = np.stack([cam[:, 0].astype(np.float64), cam[:, 1].astype(np.float64), -np.ones(n)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros_like(d)
    if M._has_pose(camera):
        p, r, up, f = M.basis(camera)
        o = o + p
        d = d[:, 0:1] * r + d[:, 1:2] * up - d[:, 2:3] * f
    best, t = _nearest(scene, o, d, None)
    hit = best >= 0
    b = np.maximum(best, 0)
    depth = np.where(hit, t, 0.0)
    hp = o + d * depth[:, None]
    radial = hp - scene["centre"].astype(np.float64)[b]
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where((scene["shape"][b] >= DISC)[:, None], scene["normal"].astype(np.float64)[b],
                       radial / np.linalg.norm(radial, axis=-1, keepdims=True))
    cosine = _dot(nrm, d)
    nrm = np.where((cosine > 0)[:, None], -nrm, nrm)
    oc = o - scene["centre"].astype(np.float64)[b]
    bb = _dot(oc, d)
    disc = bb * bb - (_dot(oc, oc) - scene["radius"].astype(np.float64)[b] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        good = np.where(scene["shape"][b] >= DISC, np.abs(cosine) >= 1e-4, disc / (bb * bb) >= 1e-4)
    return np.where(hit, best, -1).astype(np.int32), depth, np.where(hit[:, None], nrm, 0.0), hit & good


# ---- the cases: scenes in CAMERA space (x right, y up, the view along -z), placed in front of each camera by its frame

W, H = 64, 48
SEED = M.SEED
AA_SCALE = M.AA_SCALE
DEPTH, ROULETTE = M.DEPTH, M.ROULETTE
ENV = M.ENV
EMISSION = (6.0, 4.5, 3.0)
# The pose stays near the origin and the lens small: the scenes are a fraction of a unit across (the cap on fragile paths), the
# model traces in world space, and its perturbations are relative to the world coordinates' size.
MOVED = dict(position=(0.3, 0.14, 0.4), look_at=(0.04, -0.06, -0.6), up=(0.1, 1.0, 0.2))
LENS = dict(lens_radius=0.03, focus_distance=0.6)
CAMERAS = {"none": None, "moved": dict(MOVED), "lens": dict(LENS), "lens_moved": dict(LENS, **MOVED)}
SAMPLES = (0, 7)


def _tri(v0, v1, v2, material, colour=(1.0, 1.0, 1.0)):
    return dict(shape=TRIANGLE, material=material, vertices=(v0, v1, v2), colour=colour)


def _par(v0, v1, v2, material, colour=(1.0, 1.0, 1.0)):
    return dict(shape=PARALLELOGRAM, material=material, vertices=(v0, v1, v2), colour=colour)


def _cornell():
    """A box open towards the camera, x in [-1, 1], y in [-1, 1], z in [-3.2, 0.4] (before the scaling at the end): five diffuse walls, an emissive ceiling lamp,
    a mirror, a glass and a diffuse sphere, and two triangles that form a wedge on the floor."""
    x0, x1, y0, y1, zf, zb = -1.0, 1.0, -1.0, 1.0, 0.4, -3.2
    white, red, green = (0.75, 0.75, 0.75), (0.75, 0.2, 0.2), (0.2, 0.75, 0.25)
    objs = [
        _par((x0, y0, zf), (x1, y0, zf), (x0, y0, zb), DIFFUSE, white),                 # 0 floor
        _par((x0, y1, zf), (x0, y1, zb), (x1, y1, zf), DIFFUSE, white),                 # 1 ceiling
        _par((x0, y0, zb), (x1, y0, zb), (x0, y1, zb), DIFFUSE, white),                 # 2 back wall
        _par((x0, y0, zf), (x0, y0, zb), (x0, y1, zf), DIFFUSE, red),                   # 3 left wall
        _par((x1, y0, zf), (x1, y1, zf), (x1, y0, zb), DIFFUSE, green),                 # 4 right wall
        _par((-0.4, 0.98, -1.6), (0.4, 0.98, -1.6), (-0.4, 0.98, -2.4), EMISSIVE, EMISSION),   # 5 the lamp, just under the ceiling
        M._sph((-0.5, -0.65, -2.5), 0.35, SPECULAR),                                    # 6 mirror
        M._sph((0.45, -0.7, -1.9), 0.3, REFRACTIVE, (0.95, 0.95, 0.9)),                 # 7 glass
        M._sph((0.1, -0.8, -2.7), 0.2, DIFFUSE, (0.3, 0.4, 0.9)),                       # 8 diffuse
        _tri((-0.9, -1.0, -1.4), (-0.3, -1.0, -1.7), (-0.6, -0.5, -1.7), DIFFUSE, (0.9, 0.8, 0.3)),   # 9, 10: a wedge on the floor,
        _tri((-0.3, -1.0, -1.7), (-0.7, -1.0, -2.1), (-0.6, -0.5, -1.7), SPECULAR),                   # sharing the edge to its apex
    ]
    # The box is turned a little about the y and then the x axis through its middle: a wall that faces the camera squarely has the
    # camera-space normal (0, 0, 1), and under a pose the rounding of R^T n alone would decide |n.x| > |n.y|, the branch of the
    # diffuse basis -- every diffuse hit on the back wall would be fragile.
    ay, ax = np.deg2rad(11.0), np.deg2rad(-7.0)
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    mid = np.array([0.0, 0.0, -1.4])

    def turn(q):
        return tuple(float(x) for x in (rx @ ry @ (np.asarray(q, np.float64) - mid) + mid))
    for ob in objs:
        if "vertices" in ob:
            ob["vertices"] = tuple(turn(q) for q in ob["vertices"])
        else:
            ob["centre"] = turn(ob["centre"])
    # the whole box at a fifth of that size (scene_model's crowd is scaled likewise): the intersection epsilon is absolute and binary32's
    # errors are relative, so a smaller scene leaves fewer bounces within rounding of it (the cap on fragile paths)
    for ob in objs:
        if "vertices" in ob:
            ob["vertices"] = tuple(tuple(0.2 * x for x in p) for p in ob["vertices"])
        else:
            ob["centre"] = tuple(0.2 * x for x in ob["centre"])
            ob["radius"] = 0.2 * ob["radius"]
    return objs


def _mixed32():
    """32 objects: polygons interleaved among concentric sphere pairs and a disc, declared out of depth order, a polygon seen from
    behind (index 2: its normal points away from the camera) and the nearest object last."""
    o = [None] * 32
    o[0] = _par((-2.5, -1.2, -3.0), (2.5, -1.2, -3.0), (-2.5, 2.0, -3.2), SPECULAR)                 # the farthest object first
    o[1] = M._sph((-0.3, -0.2, -1.25), 0.125, DIFFUSE, (0.9, 0.2, 0.2))                            # concentric pair
    o[2] = _tri((0.3, -0.4, -1.5), (0.9, 0.3, -1.6), (0.95, -0.45, -1.4), DIFFUSE, (0.3, 0.8, 0.4))   # wound to face away
    o[3] = M._sph((-0.3, -0.2, -1.25), 0.15, REFRACTIVE, (0.95, 0.95, 0.8))
    o[4] = M._dsc((0.0, -0.6, -1.8), (0.0, 1.0, 0.15), 1.2, DIFFUSE, (0.6, 0.6, 0.7))
    o[5] = M._sph((0.4, 0.3, -1.75), 0.09, DIFFUSE, (0.2, 0.4, 0.9))                               # a polygon between the two
    o[6] = _par((-0.9, 0.2, -2.0), (-0.4, 0.25, -2.1), (-0.85, 0.7, -2.0), EMISSIVE, EMISSION)     # spheres of a pair
    o[7] = M._sph((0.4, 0.3, -1.75), 0.125, REFRACTIVE, (0.8, 0.95, 0.9))
    o[31] = _tri((-0.15, -0.1, -0.55), (0.05, -0.12, -0.6), (-0.05, 0.08, -0.58), REFRACTIVE, (0.9, 0.9, 1.0))   # the nearest, last
    mats = (DIFFUSE, SPECULAR, REFRACTIVE)
    free = [i for i in range(32) if o[i] is None]
    for k, i in enumerate(free):                      # a lattice, the depth neither rising nor falling with the index
        z = -(0.9 + ((k * 7) % 16) * 0.1)
        x = (((k * 5) % 8) - 3.5) * 0.2 * -z
        y = (((k * 3) % 5) - 2.0) * 0.2 * -z
        s = 0.07 * -z
        col = (0.35 + 0.6 * ((k * 3) % 4) / 3.0, 0.35 + 0.6 * ((k * 5) % 7) / 6.0, 0.35 + 0.6 * (k % 5) / 4.0)
        if k % 3 == 0:
            o[i] = _tri((x - s, y - s, z), (x + s, y - s, z - 0.3 * s), (x, y + s, z + 0.2 * s), mats[k % 3 - 1], col)
        elif k % 3 == 1:
            o[i] = _par((x - s, y - s, z), (x - s, y + s, z + 0.4 * s), (x + s, y - s, z - 0.3 * s), mats[(k // 3) % 3], col)
        else:
            o[i] = M._sph((x, y, z), s, mats[(k // 3) % 3], col)
    return o


SCENES = {
    "triangle": [_tri((-1.6, -1.1, -3.0), (1.7, -0.9, -3.4), (0.1, 1.4, -2.6), DIFFUSE, (0.8, 0.5, 0.25))],
    "parallelogram": [_par((-1.2, -0.9, -3.2), (0.9, -1.0, -2.6), (-1.0, 0.8, -3.3), SPECULAR)],
    "cornell": _cornell(),
    "mixed32": _mixed32(),
}
assert len(SCENES["mixed32"]) == 32 and len(SCENES["cornell"]) == 11

# test A: every scene meets every camera; the sample precision alternates so that each camera kind runs both
CASES_A = [(s, c, (i + j) % 2 == 0) for i, s in enumerate(SCENES) for j, c in enumerate(CAMERAS)]
# test B: the singles with no camera and with lens + pose, cornell and mixed32 with all four
CASES_B = [(s, c, (i + j) % 2 == 1) for i, s in enumerate(SCENES) for j, c in enumerate(CAMERAS)
           if s in ("cornell", "mixed32") or c in ("none", "lens_moved")]


def world_scene(name, camera_name, extra=()):
    """The scene's objects (dicts, plus `extra`) placed in front of the camera: a camera-space point (x, y, z) is
    position + x r + y u - z f, rounded to the binary32 the library is given."""
    camera = CAMERAS[camera_name]
    objs = [dict(o) for o in list(SCENES[name]) + list(extra)]
    if M._has_pose(camera):
        p, r, up, f = M.basis(camera)

        def point(c):
            c = np.asarray(c, np.float64)
            return tuple(float(x) for x in np.float32(p + c[0] * r + c[1] * up - c[2] * f))
        for o in objs:
            if "vertices" in o:
                o["vertices"] = tuple(point(c) for c in o["vertices"])
                continue
            o["centre"] = point(o["centre"])
            if o["shape"] == DISC:
                nn = np.asarray(o["normal"], np.float64)
                o["normal"] = tuple(float(x) for x in np.float32(nn[0] * r + nn[1] * up - nn[2] * f))
    return objs


def case_options(samples_half):
    return M.options(max_path_length=DEPTH, roulette_depth=ROULETTE, samples_half=samples_half, seed=SEED)


def all_pixels():
    rr, cc = np.divmod(np.arange(W * H), W)
    return cc.astype(np.uint16), rr.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def oracle_cam(sample):
    """The half-exact camera rays of every pixel at one sample index, from the CPU oracle (they depend on the options only)."""
    from oracle import pt_oracle as O
    cfg = O.make_config(width=W, height=H, seed=SEED, aa_noise_scale=AA_SCALE)
    u, v = all_pixels()
    return np.array([list(O.trace_path(cfg, int(a), int(b), int(sample)).cam) for a, b in zip(u, v)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case_b(scene_name, camera_name, samples_half):
    """Test B's inputs and the model's analysis of them with the CPU's own copy of the stored table: (u, v, sample, cam, plain,
    fragile, spread) over all pixels and SAMPLES."""
    u, v = all_pixels()
    uu, vv = np.tile(u, len(SAMPLES)), np.tile(v, len(SAMPLES))
    ss = np.repeat(np.array(SAMPLES, np.uint32), len(u))
    cam = np.concatenate([oracle_cam(s) for s in SAMPLES])
    scene = stored_scene_ex(world_scene(scene_name, camera_name))
    plain, fragile, spread = analyse(scene, CAMERAS[camera_name], case_options(samples_half), uu, vv, ss, cam, ENV)
    return uu, vv, ss, cam, plain, fragile, spread
