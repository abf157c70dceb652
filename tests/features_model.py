"""Cases and yardsticks of tests/test_gpu_features.py -- test infrastructure only.

model64    depth, world normal and object index of every pixel's centre ray from tests/scene_model.py's float64 `_nearest`, on
           the world-space ray built from the half-rounded (camx, camy) and `basis`.
restate32  the kernel's expressions (csrc/pt_features.h, nearest_hit_primary, fill_scene) restated in numpy binary32: camera-space
           table, origin-folded constants, normalise as x * (1 / sqrt), the flip, the rotation to world space.
calibrate  the largest deviation of restate32 from model64 over the compared pixels of every case: what binary32 alone costs.
           The GPU test allows four times that (the device's sqrt and division may differ from numpy's by an ulp or two).
               python -m tests.features_model
           prints the figures the literals below were taken from.

A pixel is compared when both sides name the same object and the hit is not grazing:
    sphere  disc / b^2 >= 1e-4, with b = dot(oc, d) and disc = b^2 - (|oc|^2 - r^2): the square root of a cancelled difference
            loses the digits the cancellation took;
    disc    |dot(n, d)| >= 1e-4 (the quotient's denominator).
At most EXCLUDED_CAP of a case's hit pixels may be left out, a condition on the cases that restate32 is checked for here.
"""
import numpy as np

from ipu_path_trace_amd import ptmi
from tests import scene_model as M

F32 = np.float32
GRAZING = 1e-4
EXCLUDED_CAP = 0.05
FOV_DEGREES = 90.0
SIZES = ((64, 48), (33, 17))
POSE = dict(position=(0.4, 0.3, 0.8), look_at=(0.0, -0.6, -4.0), up=(0.05, 1.0, 0.1))      # for the built-in scene
CAMERAS = {"none": None, "posed": "pose", "posed_lens": "pose"}
LENS = dict(lens_radius=0.15, focus_distance=4.0)
CASES = [(s, c, w, h) for s in ("builtin", "crowd") for c in CAMERAS for (w, h) in SIZES]

# python -m tests.features_model (CPU, numpy binary32 against float64, all CASES):
#   largest |depth32 - depth64| / depth64 over compared pixels   9.82e-06
#   largest |normal32 - normal64| (component)                    1.09e-04
#   largest share of hit pixels excluded in one case             0.010   (with disc / b^2 >= 1e-3 the small spheres of crowd
#                                                                         lose 7 to 10 % of their pixels: over the cap)
DEPTH_DEV = 9.82e-06
NORMAL_DEV = 1.09e-04
DEPTH_TOL = 4 * DEPTH_DEV          # relative
NORMAL_TOL = 4 * NORMAL_DEV        # per component


def camera_of(scene, camera):
    """The pose (a dict for Renderer.set_camera, without the lens) of a case, or None."""
    if CAMERAS[camera] is None:
        return None
    return dict(POSE) if scene == "builtin" else dict(M.MOVED)


def objects_of(scene, camera):
    """The case's scene as a list of dicts / a SCENE_DTYPE array for Renderer.set_scene (None: the built-in scene untouched)."""
    if scene == "builtin":
        return None
    return M.world_scene("crowd", "moved" if CAMERAS[camera] else "none")


def stored(scene, camera):
    objs = objects_of(scene, camera)
    return ptmi.builtin_scene() if objs is None else M.stored_scene(objs)


def pixels(W, H):
    rr, cc = np.divmod(np.arange(W * H), W)
    return cc.astype(np.uint16), rr.astype(np.uint16)


def camera_rays(W, H):
    """The half-exact (camx, camy) of every pixel's centre ray, from the CPU oracle with no AA noise."""
    from oracle import pt_oracle as O
    cfg = O.make_config(width=W, height=H, aa_noise_scale=0.0, fov_degrees=FOV_DEGREES)
    u, v = pixels(W, H)
    return np.array([list(O.trace_path(cfg, int(a), int(b), 0).cam) for a, b in zip(u, v)], dtype=F32)


def model64(table, pose, cam):
    """(ids, depth, world normal, world ray, well conditioned) per pixel in float64."""
    n = len(cam)
    d = np.stack([cam[:, 0].astype(np.float64), cam[:, 1].astype(np.float64), -np.ones(n)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros((n, 3))
    if pose is not None:
        p, r, up, f = M.basis(pose)
        d = d[:, 0:1] * r + d[:, 1:2] * up - d[:, 2:3] * f
        o = o + p
    best, t = M._nearest(table, o, d, None)
    hit = best >= 0
    b = np.maximum(best, 0)
    depth = np.where(hit, t, 0.0)
    centre = table["centre"].astype(np.float64)[b]
    hp = o + d * depth[:, None]
    is_disc = table["shape"][b] == M.DISC
    radial = hp - centre
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.where(is_disc[:, None], table["normal"].astype(np.float64)[b], radial / np.linalg.norm(radial, axis=-1, keepdims=True))
    nrm = np.where((np.sum(nrm * d, -1) > 0)[:, None], -nrm, nrm)
    nrm = np.where(hit[:, None], nrm, 0.0)
    oc = o - centre
    bb = np.sum(oc * d, -1)
    disc = bb * bb - (np.sum(oc * oc, -1) - table["radius"].astype(np.float64)[b] ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        good = np.where(is_disc, np.abs(np.sum(table["normal"].astype(np.float64)[b] * d, -1)) >= GRAZING, disc / (bb * bb) >= GRAZING)
    return np.where(hit, best, -1).astype(np.int32), depth, nrm, d, hit & good


def _dot32(a, b):
    return F32(F32(a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def _normalise32(a):
    inv = F32(1.0) / np.sqrt(_dot32(a, a))
    return a * inv[..., None]


def restate32(table, pose, cam):
    """(ids, depth, world normal) per pixel by the kernel's binary32 expressions."""
    n = len(cam)
    eps = F32(M.EPS)
    d = _normalise32(np.stack([cam[:, 0], cam[:, 1], -np.ones(n, F32)], -1).astype(F32))
    centre, normal = table["centre"].astype(F32), table["normal"].astype(F32)
    frame = None
    if pose is not None:                                       # fill_scene: R^T (c - position), R^T n
        p, r, up, f = (x.astype(F32) for x in M.basis(pose))
        frame = (r, up, f)
        rel = centre - p
        centre = np.stack([_dot32(rel, r), _dot32(rel, up), F32(0) - _dot32(rel, f)], -1)
        normal = np.stack([_dot32(normal, r), _dot32(normal, up), F32(0) - _dot32(normal, f)], -1)
    best = np.full(n, -1, np.int32)
    tbest = np.full(n, np.inf, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i, ob in enumerate(table):
            r2 = F32(ob["radius"] * ob["radius"])
            if ob["shape"] == M.DISC:
                denom = _dot32(normal[i][None, :], d)
                tt = _dot32(centre[i], normal[i]) / denom
                pc = d * tt[:, None] - centre[i]
                t = np.where((denom != 0) & (tt > eps) & ~(_dot32(pc, pc) > r2), tt, F32(0))
            else:
                oc = F32(0) - centre[i]
                bq = F32(2) * _dot32(oc[None, :], d)
                c4 = F32(4) * F32(_dot32(oc, oc) - r2)
                disc = F32(bq * bq - c4)
                sq = np.sqrt(np.maximum(disc, F32(0)))
                s1, s2 = -bq + sq, -bq - sq
                t = np.where(disc < 0, F32(0), np.where(s2 > eps, s2 * F32(0.5), np.where(s1 > eps, s1 * F32(0.5), F32(0))))
            better = (t > eps) & (t < tbest)
            best[better] = i
            tbest[better] = t[better]
        hit = best >= 0
        b = np.maximum(best, 0)
        depth = np.where(hit, tbest, F32(0)).astype(F32)
        is_disc = table["shape"][b] == M.DISC
        nrm = np.where(is_disc[:, None], normal[b], _normalise32((d * depth[:, None] - centre[b]).astype(F32)))
        nrm = np.where((_dot32(nrm, d) > 0)[:, None], -nrm, nrm).astype(F32)
        if frame is not None:
            r, up, f = frame
            w = [F32(F32(nrm[:, 0] * r[k] + nrm[:, 1] * up[k]) - nrm[:, 2] * f[k]) for k in range(3)]
            nrm = _normalise32(np.stack(w, -1).astype(F32))
    return best, depth, np.where(hit[:, None], nrm, F32(0)).astype(F32)


def compare(got_ids, got_depth, got_normal, ids, depth, nrm, good):
    """(largest relative depth deviation, largest normal component deviation, share of hit pixels excluded) over the pixels
    whose index agrees with the model and whose hit is not grazing."""
    hit = ids >= 0
    sel = good & (np.asarray(got_ids).ravel() == ids)
    excluded = 1.0 - sel.sum() / max(int(hit.sum()), 1)
    if not sel.any():
        return 0.0, 0.0, excluded
    dd = np.abs(np.asarray(got_depth, np.float64).ravel()[sel] - depth[sel]) / depth[sel]
    dn = np.abs(np.asarray(got_normal, np.float64).reshape(-1, 3)[sel] - nrm[sel])
    return float(dd.max()), float(dn.max()), float(excluded)


def calibrate():
    worst = [0.0, 0.0, 0.0]
    for scene, camera, W, H in CASES:
        if camera == "posed_lens":
            continue                                           # the lens does not enter: the same arithmetic as "posed"
        table, pose, cam = stored(scene, camera), camera_of(scene, camera), camera_rays(W, H)
        ids, depth, nrm, _, good = model64(table, pose, cam)
        fig = compare(*restate32(table, pose, cam), ids, depth, nrm, good)
        print("%-8s %-6s %2d x %2d: hit %4d, depth %.3g, normal %.3g, excluded %.3f" % (scene, camera, W, H, (ids >= 0).sum(), *fig))
        worst = [max(a, b) for a, b in zip(worst, fig)]
    print("largest: depth %.3g (relative), normal %.3g (component), excluded %.3f" % tuple(worst))
    return worst


if __name__ == "__main__":
    calibrate()
