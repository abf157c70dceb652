"""Environment-guided diffuse sampling in numpy float64: a restatement of include/ptmi.h (pt_set_env_guide) -- the cell masses,
the alias table and the density made from its quantised form, the sampling and density functions of the kernels, the weight of
one guided bounce -- and the quadrature that predicts the moments of a one-bounce estimator.

Not the library's code, but the same rules in the same order of summation (texel by texel into the cells, cell by cell into the
total), so the alias table comes out entry for entry as the library builds it and a sampled cell can be compared exactly.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TWO32 = 4294967296.0
LUMA = np.array([0.0722, 0.7152, 0.2126])     # B, G, R


def sun_map(base=0.25, sun=4000.0):
    """The worked case of the issue: 64 wide, 32 high, radiance `base`, a 2 x 2-texel source of `sun` at rows and columns 15, 16."""
    img = np.full((32, 64, 3), base, F32)
    img[15:17, 15:17] = sun
    return img


def procedural_sun_map(width=512, height=256):
    """A smooth sky with a small hot sun and a dim ground: the render map of scripts/env_guide_bench.py and of the film tests."""
    r = (np.arange(height) + 0.5) / height
    c = (np.arange(width) + 0.5) / width
    sky = 0.4 + 0.6 * np.clip(1.0 - 2.0 * r, 0.0, 1.0)
    img = np.empty((height, width, 3), F64)
    img[..., 0] = (sky * 1.2)[:, None]
    img[..., 1] = (sky * 0.9)[:, None]
    img[..., 2] = (sky * 0.7)[:, None]
    img[r > 0.5] = (0.05, 0.06, 0.07)
    theta, phi = np.pi * r[:, None], 2 * np.pi * c[None, :]
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta) * np.ones_like(phi), np.sin(theta) * np.sin(phi)], -1)
    s = np.array([np.sin(np.pi * 0.3) * np.cos(2 * np.pi * 0.7), np.cos(np.pi * 0.3), np.sin(np.pi * 0.3) * np.sin(2 * np.pi * 0.7)])
    img += 3000.0 * np.exp((d @ s - 1.0) / 2e-4)[..., None] * np.array([0.8, 0.95, 1.0])
    return img.astype(F32)


def cell_masses(bgr, rows, cols):
    """Binary64 mass of every cell: luminance x sin(pi (r + 0.5) / height), texel (r, c) in cell (r rows // height, c cols // width)."""
    bgr = np.asarray(bgr, F64)
    H, W, _ = bgr.shape
    sn = np.array([math.sin(math.pi * (r + 0.5) / H) for r in range(H)])
    lum = ((0.0722 * bgr[..., 0] + 0.7152 * bgr[..., 1]) + 0.2126 * bgr[..., 2]) * sn[:, None]   # left to right, as the library
    i = (np.arange(H) * rows) // H
    j = (np.arange(W) * cols) // W
    mass = np.zeros((rows, cols), F64)
    np.add.at(mass, (i[:, None].repeat(W, 1), j[None, :].repeat(H, 0)), lum)   # unbuffered: texel by texel in row-major order
    return mass.reshape(-1)


def total_mass(mass):
    total = 0.0
    for m in mass:            # cell by cell, as the library sums it
        total += float(m)
    return total


def vose(mass):
    """Vose's alias method in binary64, thresholds quantised to 32 bits: cell k is kept when a word is < threshold[k]."""
    n = len(mass)
    p = mass / total_mass(mass) * n
    thr, alias = np.zeros(n, np.uint64), np.arange(n, dtype=np.uint64)
    small = [k for k in range(n) if p[k] < 1.0 and mass[k] > 0] + [k for k in range(n) if mass[k] == 0]
    large = [k for k in range(n) if p[k] >= 1.0]
    p = p.copy()
    while small and large:
        s, l = small.pop(), large[-1]
        thr[s] = min(int(np.floor(p[s] * TWO32)), 0xffffffff)
        alias[s] = l
        p[l] = (p[l] + p[s]) - 1.0
        if p[l] < 1.0:
            large.pop()
            small.append(l)
    for k in large + small:   # 1 up to rounding: the column keeps its own cell (an empty cell is never left: it would gain mass)
        assert mass[k] > 0
        thr[k], alias[k] = 0xffffffff, k
    return thr.astype(np.uint32), alias.astype(np.uint32)


def table_probability(thr, alias):
    """P(cell) the quantised table really draws: (threshold[cell] + sum over k with alias[k] = cell of (2^32 - threshold[k])) / (n 2^32)."""
    n = len(thr)
    acc = thr.astype(np.uint64).copy()
    np.add.at(acc, alias.astype(np.int64), (np.uint64(1 << 32) - thr.astype(np.uint64)))
    return acc.astype(F64) / (n * TWO32)


class Guide:
    """The tables of one guide: threshold, alias, P, q (float32, as the device holds it), alpha as used."""

    def __init__(self, bgr, rows, cols, alpha):
        self.rows, self.cols, self.n = rows, cols, rows * cols
        self.log2n = int(np.log2(self.n))
        self.mass = cell_masses(bgr, rows, cols)
        self.thr, self.alias = vose(self.mass)
        self.P = table_probability(self.thr, self.alias)
        self.q = (self.P * self.n / np.pi).astype(F32)
        self.alpha_thr = int(F64(alpha) * TWO32)
        self.alpha = self.alpha_thr / TWO32


def sample_cell(G, g1, g2):
    """k = g1 >> (32 - log2 n); the cell is k if g2 < threshold[k], else alias[k]."""
    g1, g2 = np.asarray(g1, np.uint64), np.asarray(g2, np.uint64)
    k = (g1 >> np.uint64(32 - G.log2n)).astype(np.int64) if G.log2n else np.zeros(len(g1), np.int64)
    return np.where(g2 < G.thr[k], k, G.alias[k].astype(np.int64))


def sample_uv(G, cell, g3, dtype=F64):
    """u = (i + ((g3 >> 16) + 0.5) / 65536) / rows, v = (j + ((g3 & 0xffff) + 0.5) / 65536) / cols, in `dtype`."""
    g3 = np.asarray(g3, np.uint32)
    i, j = (cell // G.cols).astype(dtype), (cell % G.cols).astype(dtype)
    hi, lo = (g3 >> np.uint32(16)).astype(dtype), (g3 & np.uint32(0xffff)).astype(dtype)
    u = (i + (hi + dtype(0.5)) / dtype(65536)) / dtype(G.rows)
    v = (j + (lo + dtype(0.5)) / dtype(65536)) / dtype(G.cols)
    return u, v


def direction(u, v, azimuth, dtype=F64):
    """theta = pi u, phi = 2 pi v - azimuth, (sin theta cos phi, cos theta, sin theta sin phi): the inverse of dir_to_uv."""
    u, v = np.broadcast_arrays(np.asarray(u, dtype), np.asarray(v, dtype))
    theta, phi = dtype(np.pi) * u, dtype(2 * np.pi) * v - dtype(azimuth)
    return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1).astype(dtype)


def dir_to_uv(d, azimuth, dtype=F64):
    """PreProcessEscapedRays: theta = acos(y), phi = atan2(z, x) + azimuth wrapped once into [0, 2 pi]; u = theta / pi, v = phi / 2 pi."""
    d = np.asarray(d, dtype)
    theta = np.arccos(np.clip(d[..., 1], -1, 1))
    phi = np.arctan2(d[..., 2], d[..., 0]) + dtype(azimuth)
    two_pi = dtype(2 * np.pi)
    phi = np.where(phi < 0, phi + two_pi, np.where(phi > two_pi, phi - two_pi, phi))
    return (theta / dtype(np.pi)).astype(dtype), (phi / two_pi).astype(dtype)


def cell_of(G, u, v):
    i = np.minimum((np.asarray(u) * G.rows).astype(np.int64), G.rows - 1)
    j = (np.asarray(v) * G.cols).astype(np.int64) % G.cols
    return i * G.cols + j


def density(G, d, azimuth, dtype=F64):
    """(cell, g) of world directions d: g = q[cell] / max(sqrt(1 - y^2), 1e-30)."""
    d = np.asarray(d, dtype)
    u, v = dir_to_uv(d, azimuth, dtype)
    cell = cell_of(G, u, v)
    sint = np.maximum(np.sqrt(np.maximum(dtype(1) - d[..., 1] * d[..., 1], 0)), dtype(1e-30))
    return cell, (G.q[cell].astype(dtype) / sint).astype(dtype)


def bounce_factor(G, cos, g, rr=1.0):
    """What one guided diffuse bounce multiplies T (.) colour by: cos rr / ((1 - alpha) + alpha g)."""
    return cos * rr / ((1.0 - G.alpha) + G.alpha * g)


def border_distance(G, u, v):
    """Distance of (u, v) to the nearest cell border, in u and in v (in units of u and v)."""
    fu, fv = np.asarray(u, F64) * G.rows, np.asarray(v, F64) * G.cols
    du = np.abs(fu - np.round(fu)) / G.rows
    dv = np.abs(fv - np.round(fv)) / G.cols
    return du, dv


def nearest_texel(bgr, u, v):
    """pt_set_env_map, PT_ENV_FILTER_NEAREST: texel (min(floor(u H), H - 1), floor(v W) mod W)."""
    H, W, _ = bgr.shape
    r = np.minimum(np.floor(np.clip(u, 0, 1) * H).astype(np.int64), H - 1)
    c = np.floor(np.clip(v, 0, 1) * W).astype(np.int64) % W
    return np.asarray(bgr)[r, c]


# ---- one-bounce estimator: hit (normal n, world space) -> one diffuse bounce -> escape into the map L.
# X / colour = cos L / m on the hemisphere, m = (1 - alpha) + alpha g (m = 1 unguided), drawn with density m / 2 pi there; the
# guide branch below the surface gives X = 0.  With d omega = 2 pi^2 sin(theta) du dv:
#   E[(X / colour)^k] = integral over cos > 0 of pi sin(theta) (cos L)^k / m^(k - 1) du dv.
def _raw_moments(G, L, normal, azimuth, sub):
    """Raw moments 1..4 (per channel of L [H, W]) by midpoint quadrature with sub x sub points per texel of L."""
    H, W = L.shape
    nu, nv = H * sub, W * sub
    u = (np.arange(nu) + 0.5) / nu
    v = (np.arange(nv) + 0.5) / nv
    theta = np.pi * u
    out = np.zeros(4)
    n = np.asarray(normal, F64)
    Lr = np.repeat(L, sub, axis=0)
    for a in range(0, nu, 256):                      # in bands of rows: memory
        b = min(nu, a + 256)
        st, ct = np.sin(theta[a:b])[:, None], np.cos(theta[a:b])[:, None]
        phi = 2 * np.pi * v[None, :] - azimuth
        cos = np.maximum(n[0] * st * np.cos(phi) + n[1] * ct + n[2] * st * np.sin(phi), 0.0)
        if G is None:
            m = 1.0
        else:
            i = np.minimum((u[a:b] * G.rows).astype(np.int64), G.rows - 1)
            j = (v * G.cols).astype(np.int64) % G.cols
            g = G.q[i[:, None] * G.cols + j[None, :]].astype(F64) / np.maximum(st, 1e-30)
            m = (1.0 - G.alpha) + G.alpha * g
        f = cos * np.repeat(Lr[a:b], sub, axis=1)
        w = np.pi * st / (nu * nv)
        for k in range(4):
            out[k] += np.sum(w * f ** (k + 1) / m ** k)
    return out


def one_bounce_moments(G, L, normal, azimuth=0.0, paths=1 << 20, max_sub=64):
    """(mean, variance, fourth central moment) of X / colour for one channel L [H, W] of a nearest-filtered map; G = None:
    unguided.  The quadrature is refined until doubling it changes the mean by less than a tenth of the standard error of
    `paths` samples."""
    sub, last = 2, None
    while True:
        m = _raw_moments(G, L, normal, azimuth, sub)
        var = m[1] - m[0] ** 2
        if last is not None and abs(m[0] - last) < 0.1 * np.sqrt(var / paths):
            break
        if sub >= max_sub:
            raise RuntimeError("quadrature did not converge at %d points per texel" % sub)
        last, sub = m[0], sub * 2
    mu = m[0]
    mu4 = m[3] - 4 * mu * m[2] + 6 * mu * mu * m[1] - 3 * mu ** 4
    return mu, var, mu4


def dead_share(G, normal, azimuth=0.0, sub=8):
    """Probability that a bounce takes the guide branch and points below the surface: alpha x P(cos <= 0 under the guide)."""
    nu, nv = G.rows * sub, G.cols * sub
    u, v = (np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv
    d = direction(u[:, None], v[None, :], azimuth)
    below = (d @ np.asarray(normal, F64)) <= 0
    cell = cell_of(G, u[:, None] * np.ones_like(v)[None, :], np.ones_like(u)[:, None] * v[None, :])
    return G.alpha * np.sum(G.P[cell] * below) / (sub * sub)


def furnace_second_moment(G, normals, azimuth=0.0, sub=2):
    """Mean over `normals` [k, 3] of E[(X / (c L))^2] = integral over cos > 0 of pi sin(theta) cos^2 / m du dv for a constant
    environment: the second moment of the guided furnace estimator (its mean is 1/2 whatever the guide)."""
    nu, nv = G.rows * sub, G.cols * sub
    u, v = (np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv
    d = direction(u[:, None], v[None, :], azimuth).reshape(-1, 3)
    st = np.sin(np.pi * u)[:, None].repeat(nv, 1).reshape(-1)
    i = np.minimum((u * G.rows).astype(np.int64), G.rows - 1)
    j = (v * G.cols).astype(np.int64) % G.cols
    g = G.q[(i[:, None] * G.cols + j[None, :]).reshape(-1)].astype(F64) / np.maximum(st, 1e-30)
    w = np.pi * st / (nu * nv) / ((1.0 - G.alpha) + G.alpha * g)
    total = 0.0
    normals = np.asarray(normals, F64)
    for a in range(0, len(normals), 64):
        cos = np.maximum(normals[a:a + 64] @ d.T, 0.0)
        total += np.sum((cos * cos) @ w)
    return total / len(normals)
