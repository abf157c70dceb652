"""Emitter-guided diffuse sampling in numpy float64: a restatement of include/ptmi.h (pt_set_light_guide), of the host table
(csrc/ptmi_light_guide.h) and of the device functions (csrc/pt_light_guide.h).

Every function that takes `dtype` evaluates the header's expressions in that type, in the header's order, so that the float32
run against the float64 run shows what binary32 does to these formulas on given inputs (the project's rule: a device result may
differ from float64 by eight times that).

Objects are dicts as tests/scene_model.py makes them: shape ("sphere" | "disc" or the PT_SHAPE_* integers 0 | 1), material,
centre, radius, normal (disc), colour.  Densities are in units of the hemisphere's 1 / 2 pi.

THE RIM RULE (stated in csrc/pt_light_guide.h): a direction drawn from emitter k takes k's own term by construction -- `mixture`
with drawn = k -- and does not run k's inside test; the test is used for every other emitter, and for all of them when the
direction came from the hemisphere or the environment guide.

The denominator of a guided bounce, whichever branch gave w:
    den = (one_minus + alpha g_env(w)) + beta ((1 - P_E) + sum over eligible k of p_k g_k(w)),   T <- T (.) colour cos rr / den,
one_minus = float32(1 - (alpha_thr + beta_thr) / 2^32).
"""
import numpy as np

EPS = 1e-5
EMISSIVE = 3
TWO32 = 4294967296.0
MAX_BETA = float(np.float32(0.9))


def _is_disc(o):
    return o["shape"] in ("disc", 1)


def _is_emitter(o):
    return o["material"] in ("emissive", EMISSIVE)


# ---- the table

class Table:
    """Emitter rank -> object index, mass, threshold, integer weight (p 2^32) and float32 probability."""

    def __init__(self, objects, beta=0.5):
        self.beta_thr = int(np.float64(np.float32(beta)) * TWO32)
        self.beta = self.beta_thr / TWO32
        self.index = [i for i, o in enumerate(objects) if _is_emitter(o)][:32]
        self.n = len(self.index)
        mass = []
        for i in self.index:
            o = objects[i]
            c = [float(np.float32(x)) for x in o["colour"]]
            y = 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]
            r = float(np.float32(o["radius"]))
            m = y * (2.0 if _is_disc(o) else 4.0) * r * r
            mass.append(m if m > 0.0 and np.isfinite(m) else 0.0)
        self.mass = np.array(mass, np.float64)
        total = float(sum(mass))             # left to right, as the header sums
        positive = [k for k, m in enumerate(mass) if m > 0.0]
        self.active = bool(positive) and total > 0.0 and np.isfinite(total)
        self.threshold = np.zeros(self.n, np.uint32)
        self.weight = np.zeros(self.n, np.uint64)
        self.n_draw = 0
        if self.active:
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

    def select(self, g1):
        """Rank selected by each 32-bit word: the first k with g1 < threshold[k], else the last rank that can be drawn."""
        g1 = np.asarray(g1, np.uint32)
        sel = np.full(g1.shape, self.n_draw - 1, np.int64)
        for k in range(self.n_draw - 2, -1, -1):
            sel = np.where(g1 < self.threshold[k], k, sel)
        return sel


def one_minus(alpha_thr, beta_thr):
    return np.float32(1.0 - (float(alpha_thr) + float(beta_thr)) / TWO32)


# ---- geometry (the header's expressions, in its order)

def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _obj(o, dtype):
    c = np.array(o["centre"], np.float32).astype(dtype)
    r = np.float32(o["radius"]).astype(dtype)
    r2 = (np.float32(o["radius"]) * np.float32(o["radius"])).astype(dtype) if dtype == np.float32 else r * r
    m = None
    if _is_disc(o):
        m = np.array(o["normal"], np.float32)
        m = (m / np.sqrt(np.float32(_dot(m, m)))).astype(dtype) if dtype == np.float32 else m.astype(dtype) / np.sqrt(_dot(m.astype(dtype), m.astype(dtype)))
    return c, r, r2, m


def stored(objects):
    """The objects as the library stores them: binary32 values, disc normals normalised in binary32."""
    out = []
    for o in objects:
        q = dict(o)
        q["centre"] = tuple(float(np.float32(x)) for x in o["centre"])
        q["radius"] = float(np.float32(o["radius"]))
        if _is_disc(o):
            m = np.array(o["normal"], np.float32)
            m = m / np.sqrt(np.float32(_dot(m, m)))
            q["normal"] = tuple(float(x) for x in m)
        out.append(q)
    return out


def eligible(o, x, n, dtype=np.float64):
    """(eligible, v, aux): v = c - x; aux = |v|^2 (sphere) or the height (c - x) . m (disc)."""
    c, r, r2, m = _obj(o, dtype)
    x, n = np.asarray(x, dtype), np.asarray(n, dtype)
    v = c - x
    if m is not None:
        aux = _dot(v, m)
        nm = _dot(n, m)
        ok = (np.abs(aux) > dtype(EPS)) & (_dot(v, n) + r * np.sqrt(np.maximum(dtype(0), dtype(1) - nm * nm)) > 0)
        return ok, v, aux
    aux = _dot(v, v)
    return (aux > r2) & (_dot(v, n) + r > 0), v, aux


def eligibility_margin(o, x, n):
    """How far (x, n) is from a boundary of eligibility (float64): the smaller of the two tests' |left side - right side|, each
    relative to the magnitude of the terms it adds up -- what the rounding of those terms is proportional to."""
    c, r, r2, m = _obj(o, np.float64)
    v = c - np.asarray(x, np.float64)
    n = np.asarray(n, np.float64)
    vn = np.sum(np.abs(v * n), axis=-1)
    if m is not None:
        hgt = _dot(v, m)
        nm = _dot(n, m)
        a = np.abs(np.abs(hgt) - EPS) / (np.sum(np.abs(v * m), axis=-1) + EPS)
        b = np.abs(_dot(v, n) + r * np.sqrt(np.maximum(0.0, 1.0 - nm * nm))) / (vn + r)
        return np.minimum(a, b)
    d2 = _dot(v, v)
    return np.minimum(np.abs(d2 - r2) / (d2 + r2), np.abs(_dot(v, n) + r) / (vn + r))


def density(o, x, v, aux, w, dtype=np.float64):
    """g_k(w) for any unit w, the inside test included."""
    c, r, r2, m = _obj(o, dtype)
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if m is not None:
            dn = _dot(np.broadcast_to(m, w.shape), w)
            t = aux / dn
            pc = (x + w * t[..., None]) - c
            ok = (dn != 0) & (t > dtype(EPS)) & ~(_dot(pc, pc) > r2)
            return np.where(ok, (dtype(2) * (t * t)) / (np.abs(dn) * r2), dtype(0))
        s2 = r2 / aux
        cm = np.sqrt(dtype(1) - s2)
        a = v * (dtype(1) / np.sqrt(aux))[..., None]
        return np.where(_dot(w, a) >= cm, (dtype(1) + cm) / s2, dtype(0))


def inside_margin(o, x, v, aux, w):
    """Distance of w from the rim of emitter o in the units of the inside test (float64): w . a - cm, or R^2 - |p - c|^2."""
    c, r, r2, m = _obj(o, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if m is not None:
            dn = _dot(np.broadcast_to(m, np.shape(w)), w)
            t = aux / dn
            pc = (np.asarray(x, np.float64) + w * t[..., None]) - c
            return np.where(t > 0, np.abs(r2 - _dot(pc, pc)), np.inf)
        s2 = r2 / aux
        a = v / np.sqrt(aux)[..., None]
        return np.abs(_dot(w, a) - np.sqrt(1.0 - s2))


def _basis(n):
    """The hemisphere draw's basis about n (pt_trace.h::basis_about)."""
    xmajor = np.abs(n[..., 0]) > np.abs(n[..., 1])
    m = np.where(xmajor, n[..., 0], n[..., 1])
    one = n.dtype.type(1)
    inv = one / np.sqrt(m * m + n[..., 2] * n[..., 2])
    a, b = n[..., 2] * inv, m * inv
    z = np.zeros_like(a)
    rx = np.where(xmajor[..., None], np.stack([-a, z, b], -1), np.stack([z, a, -b], -1))
    return rx, np.cross(n, rx).astype(n.dtype)


def _x12(g2, g3, dtype):
    x1 = ((np.asarray(g2, np.uint32) >> 8).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)
    x2 = (np.asarray(g3, np.uint32) >> 8).astype(dtype) * dtype(2.0 ** -24)
    return x1, x2


def draw(o, x, v, aux, x1, x2, dtype=np.float64):
    """(w, g): the direction drawn from an eligible emitter by (x1, x2) and that emitter's own term for it."""
    c, r, r2, m = _obj(o, dtype)
    x = np.asarray(x, dtype)
    x1, x2 = np.asarray(x1, dtype), np.asarray(x2, dtype)
    ang = dtype(2 * np.pi) * x2
    sn, cs = np.sin(ang).astype(dtype), np.cos(ang).astype(dtype)
    if m is not None:
        rx, ry = _basis(np.broadcast_to(m, x.shape).astype(dtype))
        rho = r * np.sqrt(x1)
        y = c + (rx * (rho * cs)[..., None] + ry * (rho * sn)[..., None])
        e = y - x
        l2 = _dot(e, e)
        ln = np.sqrt(l2)
        g = (dtype(2) * (l2 * ln)) / (np.abs(aux) * r2)
        return e * (dtype(1) / ln)[..., None], g
    s2 = r2 / aux
    cm = np.sqrt(dtype(1) - s2)
    a = v * (dtype(1) / np.sqrt(aux))[..., None]
    rx, ry = _basis(a)
    ct = dtype(1) - (x1 * s2) / (dtype(1) + cm)
    st = np.sqrt(np.maximum(dtype(0), dtype(1) - ct * ct))
    h = np.stack([cs * st, sn * st, ct], -1)
    w = np.stack([_dot(np.stack([rx[..., i], ry[..., i], a[..., i]], -1), h) for i in range(3)], -1)
    return w, (dtype(1) + cm) / s2


def sample(table, objects, x, n, g1, g2, g3, dtype=np.float64):
    """pt_light_guide_sample: (dir [N, 3], rank [N]; -1 and direction 0 where the selected emitter is not eligible)."""
    x, n = np.asarray(x, dtype), np.asarray(n, dtype)
    sel = table.select(g1)
    x1, x2 = _x12(g2, g3, dtype)
    out = np.zeros(x.shape, dtype)
    rank = np.full(len(x), -1, np.int64)
    for k in range(table.n_draw):
        mine = sel == k
        if not mine.any():
            continue
        o = objects[table.index[k]]
        ok, v, aux = eligible(o, x[mine], n[mine], dtype)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w, _ = draw(o, x[mine], v, aux, x1[mine], x2[mine], dtype)
        idx = np.flatnonzero(mine)[ok]
        out[idx] = w[ok]
        rank[idx] = k
    return out, rank


def mixture(table, objects, x, n, w, drawn=None, g_drawn=None, dtype=np.float64):
    """(sum over eligible k of p_k g_k(w), P_E), in declaration order.  drawn [N]: the rank w was drawn from (-1: none), whose term
    is g_drawn by construction (the rim rule)."""
    x, n, w = np.asarray(x, dtype), np.asarray(n, dtype), np.asarray(w, dtype)
    total, pe = np.zeros(len(x), dtype), np.zeros(len(x), dtype)
    for k in range(table.n_draw):
        p = table.p[k].astype(dtype)
        if p == 0:
            continue
        o = objects[table.index[k]]
        ok, v, aux = eligible(o, x, n, dtype)
        g = density(o, x, v, aux, w, dtype)
        if drawn is not None:
            g = np.where(np.asarray(drawn) == k, np.asarray(g_drawn, dtype), g)
        pe = np.where(ok, pe + p, pe)
        total = np.where(ok, total + p * g, total)
    return total, pe


def denominator(table, objects, x, n, w, drawn=None, g_drawn=None, alpha=0.0, g_env=0.0, alpha_thr=0):
    """den of the header for directions w (float64); alpha g_env only with an environment guide."""
    s, pe = mixture(table, objects, x, n, w, drawn, g_drawn)
    return (float(one_minus(alpha_thr, table.beta_thr)) + alpha * g_env) + table.beta * ((1.0 - pe) + s)


# ---- one-bounce moments by quadrature over the branches

def _grid(q):
    t = (np.arange(q) + 0.5) / q
    a, b = np.meshgrid(t, t, indexing="ij")
    return a.ravel(), b.ravel()


def one_bounce_moments(objects, x, n, colour, beta, sky=0.0, q=96, guided=True):
    """Moments of X = colour cos rr L_in(w) / den(w) of ONE diffuse bounce at each hit point x [N, 3] (normal n [3] or [N, 3]),
    nothing but the emitters in sight (they do not overlap as seen from x and nothing occludes them), a constant sky `sky`
    elsewhere, no environment guide: (mean, variance, fourth central moment, dead share), averaged over the N points.

    The sampling density, in units of 1 / 2 pi, is q(w) = [w above the horizon] (1 - beta P_E) + beta sum_k p_k g_k(w): the
    hemisphere branch and the fallbacks give the first term, the emitters' draws the second, and a draw below the horizon is
    dead (X = 0).  E[X^j] = int over the upper hemisphere of (colour cos L_in)^j / q^(j-1) dw / 2 pi.  The part of the integral
    inside emitter k is taken in k's own parametrisation, dw / 2 pi = dx1 dx2 / g_k(w) (midpoint rule, q x q points); the rest of
    the hemisphere in closed form: int cos^j dw / 2 pi = 1 / (j + 1), minus the emitters' parts."""
    objects = stored(objects)
    x = np.atleast_2d(np.asarray(x, np.float64))
    n = np.broadcast_to(np.asarray(n, np.float64), x.shape)
    table = Table(objects, beta if guided else 0.0)
    b = table.beta if guided else 0.0
    x1, x2 = _grid(q)
    N = len(x)
    raw = np.zeros((N, 5))          # E[X^j], j = 1..4 in columns 1..4
    dead = np.zeros(N)
    pe_all = mixture(table, objects, x, n, np.broadcast_to(n, x.shape))[1]
    q0 = 1.0 - b * pe_all                                        # density outside every emitter, above the horizon
    lamp_cos = np.zeros((N, 5))                                  # int over the emitters' parts of cos^j dw / 2 pi
    for k in range(table.n):
        o = objects[table.index[k]]
        ok, v, aux = eligible(o, x, n)
        if not ok.any():
            continue
        E = float(np.float32(o["colour"][0]))
        for i in np.flatnonzero(ok):
            xi, ni = np.broadcast_to(x[i], (len(x1), 3)), np.broadcast_to(n[i], (len(x1), 3))
            w, g = draw(o, xi, np.broadcast_to(v[i], (len(x1), 3)), np.broadcast_to(aux[i], (len(x1),)), x1, x2)
            cos = _dot(w, ni)
            up = cos > 0
            pk = float(table.p[k]) if k < len(table.p) else 0.0
            qw = q0[i] + b * pk * g                               # (the emitters do not overlap)
            cu = np.where(up, cos, 0.0)
            for j in range(1, 5):
                raw[i, j] += np.mean((colour * cu * E) ** j / qw ** (j - 1) / g)
                lamp_cos[i, j] += np.mean(cu ** j / g)
            dead[i] += b * pk * np.mean(~up)
    for j in range(1, 5):
        raw[:, j] += (colour * sky) ** j / q0 ** (j - 1) * (1.0 / (j + 1) - lamp_cos[:, j])
    m1, m2, m3, m4 = (raw[:, j].mean() for j in range(1, 5))     # the mixture over the hit points
    var = m2 - m1 * m1
    mu4 = m4 - 4 * m3 * m1 + 6 * m2 * m1 * m1 - 3 * m1 ** 4
    return m1, var, mu4, dead.mean()


def sphere_lamp_mean(colour, L, centre, radius, x, n):
    """colour L s^2 cos(theta_c) / 2: the mean of one bounce under a sphere lamp wholly above the horizon of (x, n)."""
    v = np.asarray(centre, np.float64) - np.asarray(x, np.float64)
    d2 = _dot(v, v)
    return colour * L * (radius * radius / d2) * (_dot(v, np.asarray(n, np.float64)) / np.sqrt(d2)) / 2.0


# ---- one bounce under BOTH guides: an environment map L (nearest filter) guided by the table `env` (tests/env_guide_model.py)
# with probability alpha, and emitters guided with probability beta.

def _sky_raw_moments(env, L, normal, azimuth, base, sub):
    """int over cos > 0 of (cos L)^j / (base + alpha g_env)^(j-1) dw / 2 pi, j = 1..4, with dw / 2 pi = pi sin(theta) du dv: the
    midpoint rule with sub x sub points per texel of L [H, W] (the quadrature of env_guide_model with another constant term)."""
    H, W = L.shape
    nu, nv = H * sub, W * sub
    u, v = (np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv
    theta = np.pi * u
    n = np.asarray(normal, np.float64)
    out = np.zeros(5)
    Lr = np.repeat(L, sub, axis=0)
    phi = 2 * np.pi * v[None, :] - azimuth
    j_cell = (v * env.cols).astype(np.int64) % env.cols
    for a in range(0, nu, 256):
        b = min(nu, a + 256)
        st, ct = np.sin(theta[a:b])[:, None], np.cos(theta[a:b])[:, None]
        cos = np.maximum(n[0] * st * np.cos(phi) + n[1] * ct + n[2] * st * np.sin(phi), 0.0)
        i_cell = np.minimum((u[a:b] * env.rows).astype(np.int64), env.rows - 1)
        g = env.q[i_cell[:, None] * env.cols + j_cell[None, :]].astype(np.float64) / np.maximum(st, 1e-30)
        m = base + env.alpha * g
        f = cos * np.repeat(Lr[a:b], sub, axis=1)
        w = np.pi * st / (nu * nv)
        for j in range(1, 5):
            out[j] += np.sum(w * f ** j / m ** (j - 1))
    return out


def both_guides_moments(objects, x, n, colour, beta, env, L, azimuth=0.0, q=48, paths=1 << 20):
    """As one_bounce_moments, with the sky a map L [H, W] (one channel, nearest filter, world space = the frame of x) and an
    environment guide `env` (env_guide_model.Guide, alpha inside) set too: (mean, variance, fourth central moment, dead share).
    The sampling density, in units of 1 / 2 pi, is
        q(w) = [w above the horizon] (one_minus + beta (1 - P_E)) + alpha g_env(w) + beta sum_k p_k g_k(w),
    one_minus = float32(1 - (alpha_thr + beta_thr) / 2^32): exactly the denominator the bounce divides by.  The hemisphere is
    integrated on the map's own grid as if no emitter were there; inside each emitter, in its own parametrisation, the sky's
    integrand is taken out again and the emitter's put in.  n is one normal for all x; P_E must not vary over x."""
    from tests import env_guide_model as EG
    objects = stored(objects)
    x = np.atleast_2d(np.asarray(x, np.float64))
    n0 = np.asarray(n, np.float64)
    nb = np.broadcast_to(n0, x.shape)
    table = Table(objects, beta)
    b, a = table.beta, env.alpha
    om = float(one_minus(env.alpha_thr, table.beta_thr))
    pe = mixture(table, objects, x, nb, nb)[1]
    assert np.all(pe == pe[0])
    base = om + b * (1.0 - pe[0])
    sub, last = 2, None
    while True:                                                   # refined as env_guide_model.one_bounce_moments refines it
        sky = _sky_raw_moments(env, L, n0, azimuth, base, sub)
        var = sky[2] - sky[1] ** 2
        if last is not None and abs(sky[1] - last) < 0.1 * np.sqrt(var / paths):
            break
        if sub >= 64:
            raise RuntimeError("quadrature did not converge at %d points per texel" % sub)
        last, sub = sky[1], sub * 2
    x1, x2 = _grid(q)
    k1 = len(x1)
    raw = np.zeros((len(x), 5))
    dead = np.full(len(x), EG.dead_share(env, n0, azimuth))
    for k in range(table.n_draw):
        o = objects[table.index[k]]
        pk = float(table.p[k])
        E = float(np.float32(o["colour"][0]))
        ok, v, aux = eligible(o, x, nb)
        for i in np.flatnonzero(ok):
            w, g = draw(o, np.broadcast_to(x[i], (k1, 3)), np.broadcast_to(v[i], (k1, 3)), np.broadcast_to(aux[i], (k1,)), x1, x2)
            cu = np.maximum(_dot(w, nb[i]), 0.0)
            ge = EG.density(env, w, azimuth)[1]
            Lw = EG.nearest_texel(L[..., None], *EG.dir_to_uv(w, azimuth))[..., 0]
            q_out = base + a * ge
            q_in = q_out + b * pk * g
            for j in range(1, 5):
                raw[i, j] += np.mean(((colour * cu * E) ** j / q_in ** (j - 1) - (colour * cu * Lw) ** j / q_out ** (j - 1)) / g)
            dead[i] += b * pk * np.mean(~(cu > 0))
    for j in range(1, 5):
        raw[:, j] += colour ** j * sky[j]
    m1, m2, m3, m4 = (raw[:, j].mean() for j in range(1, 5))
    var = m2 - m1 * m1
    return m1, var, m4 - 4 * m3 * m1 + 6 * m2 * m1 * m1 - 3 * m1 ** 4, dead.mean()
