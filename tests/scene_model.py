"""A float64 model of one path through a runtime scene, a runtime camera and the thin lens -- test infrastructure only.

Plain numpy in float64, written from include/ptmi.h and DESIGN.md sections 4.6 / 4.7, vectorised over paths.  It is NOT the
oracle: it knows no binary32 rounding and traces in WORLD space, where the kernels trace in camera space from host-made
per-object constants.  What it is compared with (tests/test_scene_model.py on the CPU, tests/test_gpu_scene_paths.py on the GPU)
therefore agrees with it only up to rounding, and the tolerance comes from the model alone:

  conditioning   every path is traced once plainly and K_RUNS more times with the hit distance, the hit point, the normal and
                 the new direction of every bounce, the lens origin and the camera ray's direction multiplied, component by
                 component, by 1 + delta, delta uniform in +-2^-21 (a few binary32 ulps per stage; a scalar factor on a whole
                 vector would not turn it, so every component draws its own; a sphere's hit distance also takes the factor on
                 the square in its discriminant, where binary32 cancels: _nearest).  A path any of whose discrete outcomes (hit
                 sequence, Fresnel choice, branch of the diffuse basis, length, escaped) differs among the runs, or which binary32
                 can make meet the object it has just left (_self_hit_risk), is FRAGILE and is not compared; for the others the
                 largest deviation of dir, uv (v mod 1) and throughput is the path's SPREAD.
  tolerance      |got - model| <= factor * (spread + 2e-6 * scale), scale = 1 for dir and uv, max(|T|, 1) for the throughput.
                 On the CPU, against the oracle on the built-in scene, the largest ratio over three option sets is R (below, a
                 literal); the GPU test uses the factor 2 R (runtime scenes have other curvatures and distances).

The cases of the GPU tests (scenes, cameras, pixels, samples, options) are the tables at the end: both test files import them.
"""
import functools

import numpy as np

from ipu_path_trace_amd import ptmi

SPHERE, DISC = 0, 1
DIFFUSE, SPECULAR, REFRACTIVE, EMISSIVE = 0, 1, 2, 3
EPS = 1e-5                 # intersection epsilon
LENS_BLOCK = 65            # Philox block of the lens sample (include/ptmi.h)
K_RUNS = 8
DELTA = 2.0 ** -21
FLOOR = 2e-6
FRAGILE_CAP = 0.10         # at most this share of a case's paths may be fragile: a condition on the cases, not a measurement

# Largest |oracle - model| / (spread + 2e-6 scale) over the non-fragile paths of 4096 random (u, v, sample) at 200 x 150 on the
# built-in scene, measured on the CPU (tests/test_scene_model.py::test_model_against_the_oracle_on_the_builtin_scene):
#   depth 4, half samples                 0.674   (7.6 % of the paths fragile)
#   depth 8, float samples, roulette 1    0.672   (6.8 %)
#   depth 8, refractive index 1.33        0.674   (8.0 %)
R = 0.68
GPU_FACTOR = 2.0 * R

MUTATIONS = ("skip_last", "prefer_later", "no_far_root", "one_sided_disc", "no_index_flip", "tint_on_mirror")


# ---- random words

def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters; returns the four words as uint64 arrays holding 32-bit values."""
    m32 = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & m32 for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _uniform(bits, half):
    return (bits >> np.uint64(21)).astype(np.float64) / 2048.0 if half else (bits >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


# ---- inputs

def options(max_path_length=8, roulette_depth=2, stop_prob=0.3, refractive_index=1.5, samples_half=True, seed=1):
    """The options a path depends on; stop_prob and refractive_index rounded to half as the library rounds them."""
    return dict(max_path_length=int(max_path_length), roulette_depth=int(roulette_depth), stop_prob=float(np.float16(stop_prob)),
                refractive_index=float(np.float16(refractive_index)), samples_half=bool(samples_half), seed=int(seed))


def basis(camera):
    """float64 frame of include/ptmi.h from the binary32 values the library is given: position, r, u, f."""
    p = np.array(np.float32(camera.get("position", (0, 0, 0))), dtype=np.float64)
    f = np.array(np.float32(camera.get("look_at", (0, 0, -1))), dtype=np.float64) - p
    f /= np.linalg.norm(f)
    r = np.cross(f, np.array(np.float32(camera.get("up", (0, 1, 0))), dtype=np.float64))
    r /= np.linalg.norm(r)
    return p, r, np.cross(r, f), f


def stored_scene(objects):
    """The table as pt_set_scene stores it, without a device: binary32 values, disc normals n / sqrtf(dot(n, n)) in binary32,
    sphere normals 0.  (On the GPU the tests take Renderer.scene() instead.)"""
    t = ptmi.scene_array(objects).copy()
    for o in t:
        if o["shape"] == DISC:
            n = o["normal"].astype(np.float32)
            d = np.float32(np.float32(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            o["normal"] = n / np.sqrt(d)
        else:
            o["normal"] = 0
    return t


def _has_pose(camera):
    return camera is not None and any(k in camera for k in ("position", "look_at", "up"))


# ---- the path

def _perturb(x, rng):
    return x if rng is None else x * (1.0 + rng.uniform(-DELTA, DELTA, x.shape))


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _nearest(scene, o, d, mutation, rng=None, centres=None):
    """Nearest hit over the table in declaration order: (object index or -1, distance).  Every object with t > EPS counts; a sphere
    takes its near root if that is > EPS / 2, else its far root; a disc is two-sided; the earlier object wins an exact tie.
    rng: a sphere's hit distance is perturbed where binary32 loses it, in the square b^2 of the discriminant
    b^2 - |d|^2 (|oc|^2 - r^2): a factor on the root alone misses the cancellation of a grazing hit.  (A ray that starts on the
    sphere itself is the business of _self_hit_risk.)"""
    m = len(o)
    best = np.full(m, -1, dtype=np.int64)
    tbest = np.full(m, np.inf)
    n = len(scene) - (1 if mutation == "skip_last" else 0)
    dd = _dot(d, d)
    fb = _perturb(np.ones(m), rng)                   # one draw per ray, not per object: an exact tie stays one
    for i in range(n):
        ob = scene[i]
        c = ob["centre"].astype(np.float64) if centres is None else centres[:, i]     # (per path: see trace)
        r2 = float(ob["radius"]) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            if ob["shape"] == DISC:
                nrm = ob["normal"].astype(np.float64)
                denom = d @ nrm
                t = _dot(c - o, nrm) / denom
                ok = (denom != 0) & (t > EPS)
                if mutation == "one_sided_disc":
                    ok &= denom < 0
                t = np.where(ok, t, 0.0)
                pc = o + d * t[:, None] - c
                t = np.where(_dot(pc, pc) <= r2, t, 0.0)
            else:
                oc = o - c
                b = _dot(oc, d)
                disc = b * b * fb - dd * (_dot(oc, oc) - r2)
                sq = np.sqrt(np.maximum(disc, 0.0))
                near, far = (-b - sq) / dd, (-b + sq) / dd
                if mutation == "no_far_root":
                    far = np.zeros(m)
                # the reference's sphere test compares the DOUBLED roots -b -+ sqrt(b^2 - 4c) with the epsilon and halves the one it
                # takes: a near root in (EPS / 2, EPS] is taken, and then fails the scene's t > EPS -- the far root is never tried
                t = np.where(disc >= 0, np.where(2 * near > EPS, near, np.where(2 * far > EPS, far, 0.0)), 0.0)
        better = (t > EPS) & ((t <= tbest) if mutation == "prefer_later" else (t < tbest))
        best[better] = i
        tbest[better] = t[better]
    return best, tbest


def _self_hit_risk(o, d, t, hp, nrm, new_d, radial, is_disc, radius):
    """Binary32 can let the ray that leaves a hit point meet the same object again: the hit point is off the surface by its own
    rounding, and the root that is zero in exact arithmetic becomes offset / cos(out).  A bound from the number format alone
    (u = 2^-24 per rounding): the hit point o + d t carries 2 u sum |n_k hp_k| of its own along the normal and, along the ray, the error of t -- 6 u t
    for a disc's quotient of two dot products, for a sphere the cancellation in b^2 - (|oc|^2 - r^2), 2 u (b^2 + |oc|^2 + r^2) / (2 sqrt(disc)) + 2 u t.  The path is at risk
    where the offset root can reach the intersection epsilon."""
    u = 2.0 ** -24
    e_pos = 2 * u * np.sum(np.abs(nrm * hp), axis=-1)            # the rounding of o + d t, component by component, along the normal
    cos_in = np.abs(_dot(nrm, d))
    cos_out = np.maximum(np.abs(_dot(nrm, new_d)), 1e-300)
    oc = o - (hp - radial)
    b, oc2 = _dot(oc, d), _dot(oc, oc)
    disc = np.maximum(b * b - (oc2 - radius ** 2), 1e-300)
    e_t = np.where(is_disc, 6 * u * t, u * (b * b + oc2 + radius ** 2) / np.sqrt(disc) + 2 * u * t)
    off = e_pos + e_t * cos_in                                  # distance of the hit point from the surface
    root = np.where(is_disc, off / cos_out, (2 * radius * off + 6 * u * radius ** 2) / (2 * radius * cos_out))
    # a ray that leaves a sphere OUTWARDS has its zero root as the far one, which counts only above EPS; one that goes INWARDS
    # (refraction, reflection inside glass) has it as the near one, and the doubled-root rule of _nearest lets a near root in
    # (EPS / 2, EPS] hide the far side of the sphere: there the outcome changes at EPS / 2
    inward = ~is_disc & (_dot(radial, new_d) < 0)
    return root >= np.where(inward, EPS / 2, EPS)


def _dir_to_uv(d):
    """PreProcessEscapedRays with azimuth 0: u = acos(y) / pi, v = atan2(z, x) / 2 pi in [0, 1]."""
    phi = np.arctan2(d[:, 2], d[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    return np.stack([np.arccos(np.clip(d[:, 1], -1, 1)) / np.pi, phi / (2 * np.pi)], -1)


def trace(scene, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0), rng=None, mutation=None):
    """Trace paths (u[i], v[i], sample[i]) whose half-exact camera ray is cam[i] = (camx, camy) through `scene` (a stored table)
    seen by `camera` (None, or a dict with any of position / look_at / up / lens_radius / focus_distance).  rng: perturb every
    stage (module docstring).  Returns a dict of arrays: length, escaped (0 dead, 1 environment, 2 emitter), dir (world), uv,
    throughput, radiance (under the constant environment env), hits [n, depth] (object index per bounce, -1 none) and choice
    [n, depth] (1 / 2 branch of the diffuse basis, 3 refracted, 4 mirrored by glass, 0 otherwise)."""
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
        w = philox(pixel, sample, LENS_BLOCK, 0x5054, k0, k1)
        x1, x2 = _uniform(w[0], half), _uniform(w[1], half)
        o = np.stack([a * np.sqrt(x1) * np.cos(2 * np.pi * x2), a * np.sqrt(x1) * np.sin(2 * np.pi * x2), np.zeros(n)], -1)
        o = _perturb(o, rng)
        d = F * focus - o
    else:
        o = np.zeros((n, 3))
        d = focus
    d = _perturb(d / np.linalg.norm(d, axis=-1, keepdims=True), rng)
    frame = None
    if _has_pose(camera):
        p, r, up, f = basis(camera)
        frame = (r, up, f)
        o = p + o[:, 0:1] * r + o[:, 1:2] * up - o[:, 2:3] * f
        d = d[:, 0:1] * r + d[:, 1:2] * up - d[:, 2:3] * f

    out = dict(length=np.zeros(n, np.uint32), escaped=np.zeros(n, np.uint32), dir=np.zeros((n, 3)), uv=np.zeros((n, 2)),
               throughput=np.zeros((n, 3)), radiance=np.zeros((n, 3)), hits=np.full((n, D), -1, np.int8),
               choice=np.zeros((n, D), np.int8), risk=np.zeros(n, bool))
    colour = scene["colour"].astype(np.float64)
    centre = scene["centre"].astype(np.float64)
    # Under a pose the kernels see every centre through one more binary32 stage, R^T (c - position) (fill_scene): the perturbed
    # runs move c - position by its own 1 + delta, one draw per path and per DISTINCT centre (concentric spheres stay concentric,
    # and an exact tie stays one).
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
        w = philox(pixel[idx], sample[idx], 1 + depth, 0x5054, k0, k1)
        rr = 1.0
        if depth >= opt["roulette_depth"]:                      # before the intersection
            dead = _uniform(w[0], half) <= stop
            out["length"][idx[dead]] = max(depth, 1)
            keep = ~dead
            idx, o, d, T, w = idx[keep], o[keep], d[keep], T[keep], tuple(x[keep] for x in w)
            rr = 1.0 / (1.0 - stop)
        best, t = _nearest(scene, o, d, mutation, rng, None if cpath is None else cpath[idx])
        hit = best >= 0
        out["hits"][idx, depth] = best
        shape = np.where(hit, scene["shape"][np.maximum(best, 0)], -1)
        mat = np.where(hit, scene["material"][np.maximum(best, 0)], -1)
        # the environment and the emitters end the path
        for sel, code in ((~hit, 1), (mat == EMISSIVE, 2)):
            if sel.any():
                j = idx[sel]
                Te = T[sel] * rr
                out["length"][j] = depth + 1
                out["escaped"][j] = code
                out["dir"][j] = d[sel]
                out["throughput"][j] = Te
                if code == 1:
                    out["uv"][j] = _dir_to_uv(d[sel])
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
        radial = hp - (centre[best] if cpath is None else cpath[idx, best])
        nrm = np.where((shape == DISC)[:, None], normal[best], radial / np.linalg.norm(radial, axis=-1, keepdims=True))
        nrm = _perturb(nrm, rng)
        new_d = np.zeros_like(d)
        choice = np.zeros(len(idx), np.int8)
        col = colour[best]

        m = mat == DIFFUSE                                      # light::diffuse: uniform hemisphere about n, weight colour cos
        if m.any():
            # the tangent frame of light::diffuse is chosen from the normal's COMPONENTS, so it belongs to the space the kernels
            # trace in: camera space.  The frame is built there and the direction brought back.
            nn = nrm[m] if frame is None else np.stack([nrm[m] @ frame[0], nrm[m] @ frame[1], -(nrm[m] @ frame[2])], -1)
            u1, u2 = _uniform(w[1][m], half), _uniform(w[2][m], half)
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
            choice[m] = np.where(xmajor, 2, 1)

        m = mat == SPECULAR
        if m.any():
            nn, di = nrm[m], d[m]
            vv = di - nn * (2.0 * _dot(di, nn))[:, None]
            new_d[m] = vv / np.linalg.norm(vv, axis=-1, keepdims=True)
            T[m] = T[m] * rr

        m = mat == REFRACTIVE                                   # Schlick; from inside the normal and the index flip
        if m.any():
            nn, di = nrm[m].copy(), d[m]
            uu = _uniform(w[1][m], half)
            r0 = ((1.0 - ri) / (1.0 + ri)) ** 2
            inside = _dot(nn, di) > 0
            nn[inside] = -nn[inside]
            eta = np.where(inside & (mutation != "no_index_flip"), ri, 1.0 / ri)     # n_from / n_to
            cost1 = -_dot(nn, di)
            cost2 = 1.0 - eta * eta * (1.0 - cost1 * cost1)
            rprob = r0 + (1.0 - r0) * (1.0 - cost1) ** 5
            refracted = (cost2 > 0) & (uu > rprob)
            bent = di * eta[:, None] + nn * (eta * cost1 - np.sqrt(np.maximum(cost2, 0.0)))[:, None]
            mirrored = di + nn * (2.0 * cost1)[:, None]
            vv = np.where(refracted[:, None], bent, mirrored)
            new_d[m] = vv / np.linalg.norm(vv, axis=-1, keepdims=True)
            tinted = refracted | (mutation == "tint_on_mirror")
            T[m] = T[m] * np.where(tinted[:, None], col[m], 1.0) * (1.15 * rr)
            choice[m] = np.where(refracted, 3, 4)

        out["choice"][idx, depth] = choice
        out["risk"][idx] |= _self_hit_risk(o, d, t, hp, nrm, new_d, radial, shape == DISC, scene["radius"][best].astype(np.float64))
        o, d = hp, _perturb(new_d, rng)
        if depth + 1 >= D:                                      # the stack is full
            out["length"][idx] = D
    return out


def _dv(a, b):
    """|a - b| of two v coordinates, mod 1."""
    e = np.abs(a - b)
    return np.minimum(e, np.abs(1.0 - e))


def deviation(a, b):
    """Per path, the largest component deviation of dir, uv (v mod 1) and throughput between two results (dicts or records)."""
    a_uv, b_uv = np.asarray(a["uv"], np.float64), np.asarray(b["uv"], np.float64)
    return dict(dir=np.max(np.abs(np.asarray(a["dir"], np.float64) - b["dir"]), axis=-1),
                uv=np.maximum(np.abs(a_uv[:, 0] - b_uv[:, 0]), _dv(a_uv[:, 1], b_uv[:, 1])),
                throughput=np.max(np.abs(np.asarray(a["throughput"], np.float64) - b["throughput"]), axis=-1))


def analyse(scene, camera, opt, u, v, sample, cam, env=(1.0, 1.0, 1.0)):
    """The plain run plus K_RUNS perturbed ones: (plain result, fragile [n] bool, spread dict of [n] per dir / uv / throughput)."""
    plain = trace(scene, camera, opt, u, v, sample, cam, env)
    n = len(u)
    rng = np.random.default_rng(0x5CE9E)
    tiled = trace(scene, camera, opt, np.tile(u, K_RUNS), np.tile(v, K_RUNS), np.tile(sample, K_RUNS), np.tile(cam, (K_RUNS, 1)),
                  env, rng=rng)
    fragile = plain["risk"].copy()
    spread = dict(dir=np.zeros(n), uv=np.zeros(n), throughput=np.zeros(n))
    for k in range(K_RUNS):
        run = {key: val[k * n:(k + 1) * n] for key, val in tiled.items()}
        fragile |= (run["length"] != plain["length"]) | (run["escaped"] != plain["escaped"])
        fragile |= np.any(run["hits"] != plain["hits"], axis=1) | np.any(run["choice"] != plain["choice"], axis=1)
        for key, val in deviation(run, plain).items():
            spread[key] = np.maximum(spread[key], val)
    return plain, fragile, spread


def compare(got, plain, fragile, spread):
    """`got` (path records, or a model result) against the model on its non-fragile paths: (discrete outcomes all equal, largest
    |got - model| / (spread + 2e-6 scale) over dir, uv and throughput).  Paths that ended dead report no dir / uv / throughput."""
    ok = ~fragile
    same = bool(np.array_equal(np.asarray(got["length"])[ok], plain["length"][ok]) and
                np.array_equal(np.asarray(got["escaped"])[ok], plain["escaped"][ok]))
    live = ok & (plain["escaped"] != 0) & (np.asarray(got["escaped"]) == plain["escaped"])
    dev = deviation(got, plain)
    scale = dict(dir=1.0, uv=1.0, throughput=np.maximum(np.max(np.abs(plain["throughput"]), axis=-1), 1.0))
    ratio = 0.0
    for key in ("dir", "uv", "throughput"):
        if live.any():
            ratio = max(ratio, float(np.max((dev[key] / (spread[key] + FLOOR * scale[key]))[live])))
    return same, ratio


# ---- the cases: scenes in CAMERA space (x right, y up, the view along -z), placed in front of each camera by its frame

W, H = 97, 61                    # neither a multiple of 64: 5917 pixels
SAMPLES = (0, 7)                 # test B
SEED = 11
AA_SCALE = 0.3
DEPTH, ROULETTE = 8, 2
ENV = (0.7, 1.1, 0.4)
EMISSION = (6.0, 4.5, 3.0)       # shared by the three emitters of `crowd`
MOVED = dict(position=(1.5, 0.7, 2.0), look_at=(0.2, -0.3, -3.0), up=(0.1, 1.0, 0.2))   # = tests/test_gpu_camera.py
LENS = dict(lens_radius=0.15, focus_distance=4.0)
CAMERAS = {"none": None, "moved": dict(MOVED), "lens": dict(LENS), "lens_moved": dict(LENS, **MOVED)}


def _sph(c, r, material, colour=(1.0, 1.0, 1.0)):
    return dict(shape=SPHERE, material=material, centre=c, radius=r, colour=colour)


def _dsc(c, n, r, material, colour=(1.0, 1.0, 1.0)):
    return dict(shape=DISC, material=material, centre=c, normal=n, radius=r, colour=colour)


def _crowd():
    """32 objects inside the view frustum that overlap on screen, declared out of depth order (index: what it is there for)."""
    o = [None] * 32
    o[0] = _dsc((0.0, 0.0, -12.0), (0.05, -0.1, 1.0), 5.0, SPECULAR)                     # a disc first, and the farthest object
    o[1] = _sph((-3.0, 1.0, -8.0), 1.0, DIFFUSE, (0.3, 0.9, 0.5))                         # ... followed by a sphere
    o[2] = _dsc((2.5, -1.0, -6.0), (0.2, 0.1, -1.0), 1.2, SPECULAR)                        # a disc that faces away from the camera
    o[3] = _sph((-1.2, -0.8, -5.0), 0.5, DIFFUSE, (0.9, 0.2, 0.2))                        # adjacent concentric pair (same_centre)
    o[4] = _sph((-1.2, -0.8, -5.0), 0.6, REFRACTIVE, (0.95, 0.95, 0.8))
    o[5] = _sph((1.5, 1.2, -7.0), 0.35, DIFFUSE, (0.2, 0.4, 0.9))                         # adjacent concentric triple
    o[6] = _sph((1.5, 1.2, -7.0), 0.5, REFRACTIVE, (0.8, 0.95, 0.9))
    o[7] = _sph((1.5, 1.2, -7.0), 0.65, REFRACTIVE, (0.9, 0.85, 0.95))
    o[8] = _sph((0.5, -1.5, -4.0), 0.45, DIFFUSE, (0.8, 0.7, 0.1))                        # concentric pair with a disc declared
    o[9] = _dsc((-1.6, 1.5, -5.0), (0.3, -0.2, 1.0), 0.7, DIFFUSE, (0.5, 0.5, 0.9))       # ... between them (same_centre = 0)
    o[10] = _sph((0.5, -1.5, -4.0), 0.6, REFRACTIVE, (0.9, 0.9, 0.9))
    o[12] = _sph((3.5, 2.0, -9.0), 0.8, EMISSIVE, EMISSION)
    o[18] = _dsc((-3.0, -2.0, -7.0), (0.4, 0.5, 1.0), 1.0, EMISSIVE, EMISSION)
    o[20] = _sph((-3.0, 1.0, -8.0), 1.0, DIFFUSE, (0.9, 0.1, 0.9))    # the centre (and radius) of object 1 again: an exact tie
    o[25] = _sph((0.2, 2.4, -6.5), 0.5, EMISSIVE, EMISSION)
    o[31] = _sph((0.3, 0.2, -2.2), 0.35, SPECULAR)                                       # the last object is the nearest
    mats = (DIFFUSE, SPECULAR, REFRACTIVE)
    free = [i for i in range(32) if o[i] is None]
    for k, i in enumerate(free):                     # a lattice, the depth neither rising nor falling with the index
        z = -(3.5 + ((k * 7) % 16) * 0.4)
        x = (((k * 5) % 8) - 3.5) * 0.22 * -z
        y = (((k * 3) % 5) - 2.0) * 0.22 * -z
        col = (0.35 + 0.6 * ((k * 3) % 4) / 3.0, 0.35 + 0.6 * ((k * 5) % 7) / 6.0, 0.35 + 0.6 * (k % 5) / 4.0)
        if k % 5 == 4:
            o[i] = _dsc((x, y, z), (0.3 * ((k % 3) - 1), 0.4, 1.0), 0.09 * -z, mats[k % 3], col)
        else:
            o[i] = _sph((x, y, z), 0.075 * -z, mats[k % 3], col)
    # the whole crowd at a quarter of that size: the intersection epsilon is absolute, so a smaller scene leaves fewer bounces within
    # rounding of it (the cap on fragile paths)
    for ob in o:
        ob["centre"] = tuple(0.25 * x for x in ob["centre"])
        ob["radius"] = 0.25 * ob["radius"]
    return o


SCENES = {
    "single_diffuse_sphere": [_sph((0.4, -0.3, -4.0), 1.3, DIFFUSE, (0.8, 0.5, 0.25))],
    "single_specular_disc": [_dsc((-0.5, 0.2, -4.5), (0.3, -0.2, 1.0), 2.0, SPECULAR)],
    "single_refractive_sphere": [_sph((0.3, 0.2, -3.5), 1.2, REFRACTIVE, (0.9, 0.8, 0.7))],
    "single_emissive_disc": [_dsc((0.6, -0.2, -5.0), (-0.2, 0.3, 1.0), 2.2, EMISSIVE, (3.0, 2.0, 1.0))],
    "crowd": _crowd(),
    # the camera sits inside a large glass sphere that holds a small diffuse one; an emitting shell lies beyond: far-root hits,
    # the index flip, and nothing reaches the environment
    "inside": [_sph((0.2, -0.1, -0.5), 3.0, REFRACTIVE, (0.9, 0.95, 0.85)), _sph((0.5, 0.3, -1.8), 0.5, DIFFUSE, (0.9, 0.6, 0.3)),
               _sph((0.0, 0.0, 0.0), 20.0, EMISSIVE, (2.0, 1.5, 1.0))],
}
# what each scene must show so that it is not vacuous: the outcomes that occur (0 dead, 1 environment, 2 emitter; a lone convex
# diffuse sphere or a lone disc ends every path within two segments, and nothing escapes from inside the shell) and the length
# that is reached.  crowd, the scene every code path meets in, has all three outcomes and length >= 4 as a whole.
EXPECT = {"single_diffuse_sphere": ({1}, 2), "single_specular_disc": ({1}, 2), "single_refractive_sphere": ({0, 1}, 4),
          "single_emissive_disc": ({1, 2}, 1), "crowd": ({0, 1, 2}, 4), "inside": ({0, 2}, 4)}
SINGLES = tuple(k for k in SCENES if k.startswith("single"))

# test A: every scene meets every camera; the sample precision alternates so that each camera kind runs both
CASES_A = [(s, c, (i + j) % 2 == 0) for i, s in enumerate(SCENES) for j, c in enumerate(CAMERAS)]
# test B: single with no camera and with lens + pose, crowd and inside with all four
CASES_B = [(s, c, (i + j) % 2 == 1) for i, s in enumerate(SCENES) for j, c in enumerate(CAMERAS)
           if not s.startswith("single") or c in ("none", "lens_moved")]


def world_scene(name, camera_name):
    """The scene's objects (dicts) placed in front of the camera: a camera-space point (x, y, z) is position + x r + y u - z f,
    rounded to the binary32 the library is given."""
    camera = CAMERAS[camera_name]
    objs = [dict(o) for o in SCENES[name]]
    if _has_pose(camera):
        p, r, up, f = basis(camera)
        for o in objs:
            c = np.asarray(o["centre"], np.float64)
            o["centre"] = tuple(float(x) for x in np.float32(p + c[0] * r + c[1] * up - c[2] * f))
            if o["shape"] == DISC:
                nn = np.asarray(o["normal"], np.float64)
                o["normal"] = tuple(float(x) for x in np.float32(nn[0] * r + nn[1] * up - nn[2] * f))
    return objs


def case_options(samples_half):
    return options(max_path_length=DEPTH, roulette_depth=ROULETTE, samples_half=samples_half, seed=SEED)


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
    scene = stored_scene(world_scene(scene_name, camera_name))
    plain, fragile, spread = analyse(scene, CAMERAS[camera_name], case_options(samples_half), uu, vv, ss, cam, ENV)
    return uu, vv, ss, cam, plain, fragile, spread
