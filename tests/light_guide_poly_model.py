"""Polygon lamps of the emitter guide (pt_set_light_guide_ex, PT_LIGHT_GUIDE_POLYGONS) in numpy: a restatement of include/ptmi.h,
of the host table (csrc/ptmi_light_guide.h, build() with vertices) and of the device functions (csrc/pt_light_guide.h, PLAMPS).

It extends tests/light_guide_model.py: spheres and discs go through that module's functions unchanged, triangles and
parallelograms through the ones here, and `sample` / `mixture` / `one_bounce_moments` below are that module's loops over both.
Every function that takes `dtype` evaluates the header's expressions in that type, in the header's order (the project's rule: a
device result may differ from float64 by eight times what float32 numpy differs by on the same inputs).  The inside test of a
polygon's density is the tracer's own intersection, tests/scene_poly_model.py::poly_hit.

Objects are dicts as tests/scene_poly_model.py makes them: a polygon has "vertices" (v0, v1, v2), shape 2 | 3 or its name.
A polygon v0 + a e1 + b e2 has S = sqrtf(dot(c, c)), c = cross(e1, e2), all in binary32 (the value the stored normal m = c / S
was divided by), A_p = S (parallelogram) or 0.5 S (triangle) and the mass Y(colour) 2 A_p / pi.  Densities are in units of the
hemisphere's 1 / 2 pi: a uniform point of the area has 2 pi l^2 / (|m . w| A_p).

MUTATIONS are wrong versions of single steps; tests/test_light_guide_poly_model.py shows that each breaks a check.
"""
import numpy as np

from tests import light_guide_model as LM
from tests import scene_poly_model as PM

EPS = LM.EPS
TWO32 = LM.TWO32
TRIANGLE, PARALLELOGRAM = PM.TRIANGLE, PM.PARALLELOGRAM
MUTATIONS = ("no_fold", "area_not_halved", "t_not_squared", "reach_without_clamp")
_dot = LM._dot
KPI32 = np.float32(3.1415927410125732421875)


def is_polygon(o):
    return o["shape"] in ("triangle", "parallelogram", TRIANGLE, PARALLELOGRAM)


def is_triangle(o):
    return o["shape"] in ("triangle", TRIANGLE)


def frame32(o):
    """(v0, e1, e2, m, S) of a polygon in binary32, every operation rounded once and the sums left to right, as the host forms
    them (csrc/ptmi_scene.h, poly_frame / normalise_ex)."""
    f = np.float32
    v = np.array(o["vertices"], f)
    e1, e2 = f(v[1] - v[0]), f(v[2] - v[0])
    c = np.array([f(f(e1[(k + 1) % 3] * e2[(k + 2) % 3]) - f(e1[(k + 2) % 3] * e2[(k + 1) % 3])) for k in range(3)], f)
    cc = f(f(f(c[0] * c[0]) + f(c[1] * c[1])) + f(c[2] * c[2]))
    s = f(np.sqrt(cc))
    return v[0], e1, e2, f(c / s), s


def _poly(o, dtype):
    """The kernel's constants of a polygon as `dtype`: v0, e1, e2, m, A_p (all binary32 values) and kTwoPi."""
    v0, e1, e2, m, s = frame32(o)
    area = np.float32(0.5) * s if is_triangle(o) else s          # (exact)
    two_pi = np.float32(2.0) * KPI32 if dtype == np.float32 else dtype(2.0 * float(KPI32))
    return v0.astype(dtype), e1.astype(dtype), e2.astype(dtype), m.astype(dtype), dtype(area), dtype(two_pi)


# ---- the table

class Table(LM.Table):
    """light_guide_model.Table with polygons=True listing emissive polygons too, in declaration order with the spheres and discs
    (ptlight::build with vertices); polygons=False is that table itself, over the spheres and discs alone (the four-argument call)."""

    def __init__(self, objects, beta=0.5, polygons=True):
        self.polygons = bool(polygons)
        self.beta_thr = int(np.float64(np.float32(beta)) * TWO32)
        self.beta = self.beta_thr / TWO32
        self.index = [i for i, o in enumerate(objects) if LM._is_emitter(o) and (polygons or not is_polygon(o))][:32]
        self.n = len(self.index)
        mass = []
        for i in self.index:
            o = objects[i]
            c = [float(np.float32(x)) for x in o["colour"]]
            y = 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]
            if is_polygon(o):
                s = float(frame32(o)[4])
                m = y * 2.0 * (0.5 * s if is_triangle(o) else s) / np.pi
            else:
                r = float(np.float32(o["radius"]))
                m = y * (2.0 if LM._is_disc(o) else 4.0) * r * r
            mass.append(m if m > 0.0 and np.isfinite(m) else 0.0)
        self.mass = np.array(mass, np.float64)
        total = float(sum(mass))
        positive = [k for k, m in enumerate(mass) if m > 0.0]
        self.active = bool(positive) and total > 0.0 and np.isfinite(total)
        self.threshold = np.zeros(self.n, np.uint32)
        self.weight = np.zeros(self.n, np.uint64)
        self.n_draw = 0
        if self.active:                                           # light_guide_model.Table's own lines
            last = positive[-1]
            self.n_draw = last + 1
            cum, prev = 0.0, 0
            for k in range(self.n):
                c = 1 << 32
                if k < last:
                    cum += mass[k]
                    f = np.floor(TWO32 * (cum / total))
                    c = 0xffffffff if f >= TWO32 else int(f)
                    c = max(c, prev)
                self.weight[k] = c - prev
                self.threshold[k] = min(c, 0xffffffff)
                prev = c
        self.p = (self.weight.astype(np.float64) / TWO32).astype(np.float32)
        self.lists_polygon = any(is_polygon(objects[i]) for i in self.index)


def stored(objects):
    """light_guide_model.stored, polygons passed through (their constants are formed by frame32)."""
    return [dict(o) if is_polygon(o) else LM.stored([o])[0] for o in objects]


# ---- geometry

def eligible(o, x, n, dtype=np.float64, mutation=None):
    """(eligible, v, aux): a polygon's aux is the signed height (v0 - x) . m of its plane over x."""
    if not is_polygon(o):
        return LM.eligible(o, x, n, dtype)
    v0, e1, e2, m, _, _ = _poly(o, dtype)
    x, n = np.asarray(x, dtype), np.asarray(n, dtype)
    v = v0 - x
    hgt = _dot(v, m)
    d0 = _dot(v, n)
    d1 = _dot(np.broadcast_to(e1, n.shape), n)
    d2 = _dot(np.broadcast_to(e2, n.shape), n)
    zero = dtype(0)
    if mutation == "reach_without_clamp":
        reach = np.maximum(d1, d2) if is_triangle(o) else d1 + d2
    elif is_triangle(o):
        reach = np.maximum(zero, np.maximum(d1, d2))
    else:
        reach = np.maximum(zero, d1) + np.maximum(zero, d2)
    return (np.abs(hgt) > dtype(EPS)) & (d0 + reach > 0), v, hgt


def eligibility_margin(o, x, n):
    """light_guide_model.eligibility_margin for any emitter: the distance of (x, n) from a boundary of eligibility (float64), each
    test's |left - right| relative to the magnitude of the terms it adds up."""
    if not is_polygon(o):
        return LM.eligibility_margin(o, x, n)
    v0, e1, e2, m, _, _ = _poly(o, np.float64)
    x, n = np.asarray(x, np.float64), np.asarray(n, np.float64)
    ok, v, hgt = eligible(o, x, n)
    d0 = _dot(v, n)
    d1, d2 = _dot(np.broadcast_to(e1, n.shape), n), _dot(np.broadcast_to(e2, n.shape), n)
    reach = np.maximum(0, np.maximum(d1, d2)) if is_triangle(o) else np.maximum(0, d1) + np.maximum(0, d2)
    size = np.sum(np.abs(v * n), axis=-1) + np.sum(np.abs(e1 * n), axis=-1) + np.sum(np.abs(e2 * n), axis=-1)
    a = np.abs(np.abs(hgt) - EPS) / (np.sum(np.abs(v * m), axis=-1) + EPS)
    b = np.abs(d0 + reach) / size
    # the clamps themselves: a corner edge within rounding of the horizon changes reach by its own size only, continuously
    return np.minimum(a, b)


def hit(o, x, w, dtype=np.float64):
    """The tracer's polygon intersection of the rays (x, w): the distance, 0 for a miss (scene_poly_model.poly_hit in `dtype`)."""
    v0, e1, e2, _, _, _ = _poly(o, dtype)
    shape = TRIANGLE if is_triangle(o) else PARALLELOGRAM
    return PM.poly_hit(shape, v0, e1, e2, np.asarray(x, dtype), np.asarray(w, dtype)).astype(dtype)


def barycentric_margin(o, x, w):
    """The smallest of a, b, 1 - a, 1 - b (and 1 - a - b for a triangle) of the point where the ray (x, w) meets the polygon's
    plane (float64): how far a direction is from the polygon's edges, in its own coordinates.  inf where det == 0."""
    v0, e1, e2, _, _, _ = _poly(o, np.float64)
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pv = np.cross(w, e2)
        det = pv @ e1
        tv = x - v0
        a = _dot(tv, pv) / det
        b = _dot(w, np.cross(tv, e1)) / det
        parts = [a, b, 1 - a, 1 - b] + ([1 - a - b] if is_triangle(o) else [])
        mrg = np.min(np.abs(np.stack(parts)), axis=0)
    return np.where(det != 0, mrg, np.inf)


def density(o, x, v, aux, w, dtype=np.float64, mutation=None):
    """g_k(w) for any unit w, the inside test (the tracer's intersection) included."""
    if not is_polygon(o):
        return LM.density(o, x, v, aux, w, dtype)
    _, _, _, m, area, two_pi = _poly(o, dtype)
    if mutation == "area_not_halved" and is_triangle(o):
        area = area * dtype(2)
    w = np.asarray(w, dtype)
    t = hit(o, x, w, dtype)
    dn = _dot(np.broadcast_to(m, w.shape), w)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = (two_pi * (t if mutation == "t_not_squared" else t * t)) / (np.abs(dn) * area)
    return np.where((t != 0) & (dn != 0), g, dtype(0))


def draw(o, x, v, aux, x1, x2, dtype=np.float64, mutation=None):
    """(w, g): the direction drawn from an eligible emitter by (x1, x2) and that emitter's own term for it."""
    if not is_polygon(o):
        return LM.draw(o, x, v, aux, x1, x2, dtype)
    v0, e1, e2, _, area, two_pi = _poly(o, dtype)
    if mutation == "area_not_halved" and is_triangle(o):
        area = area * dtype(2)
    x = np.asarray(x, dtype)
    a, b = np.asarray(x1, dtype), np.asarray(x2, dtype)
    if is_triangle(o) and mutation != "no_fold":
        fold = a + b > dtype(1)
        a, b = np.where(fold, dtype(1) - a, a), np.where(fold, dtype(1) - b, b)
    y = v0 + (e1 * a[..., None] + e2 * b[..., None])
    e = y - x
    l2 = _dot(e, e)
    ln = np.sqrt(l2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = (two_pi * (l2 * ln)) / (np.abs(np.asarray(aux, dtype)) * area)
        return e * (dtype(1) / ln)[..., None], g


def sample(table, objects, x, n, g1, g2, g3, dtype=np.float64, mutation=None):
    """pt_light_guide_sample: (dir [N, 3], rank [N]; -1 and direction 0 where the selected emitter is not eligible)."""
    x, n = np.asarray(x, dtype), np.asarray(n, dtype)
    sel = table.select(g1)
    x1, x2 = LM._x12(g2, g3, dtype)
    out = np.zeros(x.shape, dtype)
    rank = np.full(len(x), -1, np.int64)
    for k in range(table.n_draw):
        mine = sel == k
        if not mine.any():
            continue
        o = objects[table.index[k]]
        ok, v, aux = eligible(o, x[mine], n[mine], dtype, mutation)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w, _ = draw(o, x[mine], v, aux, x1[mine], x2[mine], dtype, mutation)
        idx = np.flatnonzero(mine)[ok]
        out[idx] = w[ok]
        rank[idx] = k
    return out, rank


def mixture(table, objects, x, n, w, drawn=None, g_drawn=None, dtype=np.float64, mutation=None):
    """(sum over eligible k of p_k g_k(w), P_E), in declaration order; drawn / g_drawn: the rim rule, as light_guide_model.mixture."""
    x, n, w = np.asarray(x, dtype), np.asarray(n, dtype), np.asarray(w, dtype)
    total, pe = np.zeros(len(x), dtype), np.zeros(len(x), dtype)
    for k in range(table.n_draw):
        p = table.p[k].astype(dtype)
        if p == 0:
            continue
        o = objects[table.index[k]]
        ok, v, aux = eligible(o, x, n, dtype, mutation)
        g = density(o, x, v, aux, w, dtype, mutation)
        if drawn is not None:
            g = np.where(np.asarray(drawn) == k, np.asarray(g_drawn, dtype), g)
        pe = np.where(ok, pe + p, pe)
        total = np.where(ok, total + p * g, total)
    return total, pe


# ---- quadrature

def area_points(o, q):
    """q x q midpoints (a triangle: those of the parallelogram with a + b < 1, and the half cells on the diagonal at half weight):
    (points [M, 3], weights [M] summing to the polygon's float64 area)."""
    v0, e1, e2, _, _, _ = _poly(o, np.float64)
    t = (np.arange(q) + 0.5) / q
    a, b = (z.ravel() for z in np.meshgrid(t, t, indexing="ij"))
    cell = np.linalg.norm(np.cross(e1, e2)) / (q * q)
    wgt = np.full(len(a), cell)
    if is_triangle(o):
        s = a + b
        on = np.isclose(s, 1.0)
        keep = (s < 1.0) | on
        wgt = np.where(on, 0.5 * cell, cell)[keep]
        # the half cell on the diagonal: its centroid, a third of a cell edge towards v0
        a = np.where(on, a - 1.0 / (6 * q), a)[keep]
        b = np.where(on, b - 1.0 / (6 * q), b)[keep]
    return v0 + a[:, None] * e1 + b[:, None] * e2, wgt


def density_integral(o, x, n, q=64, mutation=None):
    """int over the polygon of g(w) dw / 2 pi by quadrature in area, dw = |m . w| dA / l^2: 1 for a density that is the law of
    a uniform point of the area (x off the plane; n any normal under which the polygon is eligible)."""
    pts, wgt = area_points(o, q)
    x = np.broadcast_to(np.asarray(x, np.float64), pts.shape)
    e = pts - x
    l2 = _dot(e, e)
    w = e / np.sqrt(l2)[:, None]
    _, _, _, m, _, _ = _poly(o, np.float64)
    ok, v, aux = eligible(o, x, np.broadcast_to(np.asarray(n, np.float64), pts.shape), mutation=mutation)
    g = density(o, x, v, aux, w, mutation=mutation)
    return float(np.sum(g * np.abs(w @ m) / l2 * wgt) / (2 * np.pi))


def one_bounce_moments(objects, x, n, colour, beta, sky=0.0, q=96, guided=True, polygons=True):
    """light_guide_model.one_bounce_moments with polygon lamps: moments of X = colour cos rr L_in(w) / den(w) of ONE diffuse
    bounce at each hit point x [N, 3] (normal n), nothing but the emitters in sight (they do not overlap as seen from x and
    nothing occludes them), a constant sky elsewhere, no environment guide: (mean, variance, fourth central moment, dead share).
    Each emitter's part of the hemisphere is integrated in its own parametrisation, dw / 2 pi = dx1 dx2 / g_k(w) -- for a triangle
    the folded draw covers the area twice, uniformly, which the same identity holds for.  An emitter the table does not list
    (polygons=False, or guided=False) is integrated in that parametrisation all the same, with p_k = 0."""
    objects = stored(objects)
    x = np.atleast_2d(np.asarray(x, np.float64))
    n = np.broadcast_to(np.asarray(n, np.float64), x.shape)
    full = Table(objects, beta, polygons=True)                   # every emitter, for the integration
    table = Table(objects, beta if guided else 0.0, polygons=polygons)
    b = table.beta if guided else 0.0
    prob = {table.index[k]: float(table.p[k]) for k in range(table.n_draw)} if table.active else {}
    x1, x2 = LM._grid(q)
    N = len(x)
    raw = np.zeros((N, 5))
    dead = np.zeros(N)
    pe_all = mixture(table, objects, x, n, n)[1] if table.active else np.zeros(N)
    q0 = 1.0 - b * pe_all
    lamp_cos = np.zeros((N, 5))
    for k in range(full.n):
        o = objects[full.index[k]]
        ok, v, aux = eligible(o, x, n)
        if not ok.any():
            continue
        E = float(np.float32(o["colour"][0]))
        pk = prob.get(full.index[k], 0.0)
        for i in np.flatnonzero(ok):
            xi = np.broadcast_to(x[i], (len(x1), 3))
            w, g = draw(o, xi, np.broadcast_to(v[i], (len(x1), 3)), np.broadcast_to(aux[i], (len(x1),)), x1, x2)
            cos = _dot(w, np.broadcast_to(n[i], (len(x1), 3)))
            up = cos > 0
            qw = q0[i] + b * pk * g
            cu = np.where(up, cos, 0.0)
            for j in range(1, 5):
                raw[i, j] += np.mean((colour * cu * E) ** j / qw ** (j - 1) / g)
                lamp_cos[i, j] += np.mean(cu ** j / g)
            dead[i] += b * pk * np.mean(~up)
    for j in range(1, 5):
        raw[:, j] += (colour * sky) ** j / q0 ** (j - 1) * (1.0 / (j + 1) - lamp_cos[:, j])
    m1, m2, m3, m4 = (raw[:, j].mean() for j in range(1, 5))
    var = m2 - m1 * m1
    mu4 = m4 - 4 * m3 * m1 + 6 * m2 * m1 * m1 - 3 * m1 ** 4
    return m1, var, mu4, dead.mean()


def rectangle_form_factor(x, corner, ex, ey, normal):
    """The configuration factor F of a rectangle (corner + s ex + t ey, ex perpendicular to ey) PARALLEL to the surface element at x
    with unit `normal` (the rectangle's plane at the distance h = (corner - x) . normal > 0): the sum over the four signed corner
    rectangles of F_corner = (1 / 2 pi) [A / sqrt(1 + A^2) atan(B / sqrt(1 + A^2)) + B / sqrt(1 + B^2) atan(A / sqrt(1 + B^2))],
    A = a / h, B = b / h, (a, b) the corner's offsets from the foot of the normal."""
    x, corner, ex, ey, normal = (np.asarray(z, np.float64) for z in (x, corner, ex, ey, normal))
    lx, ly = np.linalg.norm(ex), np.linalg.norm(ey)
    ux, uy = ex / lx, ey / ly
    rel = corner - x
    h = rel @ normal
    a0, b0 = rel @ ux, rel @ uy

    def corner_factor(a, b):
        A, B = a / h, b / h
        sa, sb = np.sqrt(1 + A * A), np.sqrt(1 + B * B)
        return (A / sa * np.arctan(B / sa) + B / sb * np.arctan(A / sb)) / (2 * np.pi)
    return (corner_factor(a0 + lx, b0 + ly) - corner_factor(a0, b0 + ly) - corner_factor(a0 + lx, b0) + corner_factor(a0, b0))
