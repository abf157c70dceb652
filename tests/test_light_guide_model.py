"""The float64 model of emitter-guided sampling (tests/light_guide_model.py) against mathematics it does not assume.

The worked case of the feature: one shading point, a sphere lamp of radius 0.2 at distance 4, 30 degrees off the normal,
radiance 100, black sky, colour 1.  The model's figures: mean 0.108253 (= the closed form 100 x 0.0025 x cos 30 / 2 to 1e-9
relative); per-sample variance 9.3594 unguided, 0.011694 at beta = 0.5, 0.0013030 at beta = 0.9 (an independent numpy Monte Carlo of 4e6
samples gave 9.39, 0.0117, 0.0013).  That Monte Carlo also had a tilted disc lamp of radius 0.3 (mean 0.164403, variances 14.1 /
0.0274 / 0.0033) whose position and tilt are not on record, so it is NOT reproduced here; the disc lamp of these tests (radius 0.3
at (1.0, 0.5, 3.0), normal (0.3, 0.2, -1), radiance 100) gives mean 0.314314 and variances 29.355 / 0.10024 / 0.012116.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import light_guide_model as LG
from tests import scene_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipu_path_trace_amd", "csrc")

N = np.array([0.0, 0.0, 1.0])
X0 = np.zeros(3)
SPHERE = dict(shape="sphere", material="emissive", centre=(2.0, 0.0, 4.0 * np.cos(np.radians(30.0))), radius=0.2, colour=(100.0, 100.0, 100.0))
DISC = dict(shape="disc", material="emissive", centre=(1.0, 0.5, 3.0), radius=0.3, normal=(0.3, 0.2, -1.0), colour=(100.0, 100.0, 100.0))
STRADDLE = dict(shape="sphere", material="emissive", centre=(3.0, 0.0, 0.2), radius=0.5, colour=(10.0, 10.0, 10.0))


def _sphere_points(q):
    """A midpoint grid over the sphere of directions: (w [q * 2q, 3], weights that sum to 2 in units of 2 pi)."""
    z = -1.0 + (np.arange(q) + 0.5) * 2.0 / q
    phi = (np.arange(2 * q) + 0.5) * np.pi / q
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1.0 - zz * zz)
    w = np.stack([s * np.cos(pp), s * np.sin(pp), zz], -1).reshape(-1, 3)
    return w, np.full(len(w), (2.0 / q) * (np.pi / q) / (2.0 * np.pi))


@pytest.mark.parametrize("lamp", [SPHERE, DISC, STRADDLE, dict(SPHERE, radius=1.5), dict(DISC, radius=2.0, normal=(1.0, 0.0, -0.2))],
                         ids=["sphere", "disc", "straddling_sphere", "large_sphere", "grazing_disc"])
def test_each_eligible_density_integrates_to_one(lamp):
    """g_k is a density over the whole sphere of directions (the part below the horizon is where draws die): in units of
    1 / 2 pi, int g dw / 2 pi = 1.  Once on a direction grid, which sees the inside test, and once in the emitter's own
    parametrisation, where the Jacobian of the draw must be 1 / g."""
    ob = LG.stored([lamp])[0]
    ok, v, aux = LG.eligible(ob, X0[None], N[None])
    assert ok[0]
    w, wt = _sphere_points(1500)
    g = LG.density(ob, np.broadcast_to(X0, w.shape), np.broadcast_to(v[0], w.shape), np.broadcast_to(aux[0], (len(w),)), w)
    total = float(np.sum(g * wt))
    print("int g dw / 2 pi = %.5f" % total)
    assert abs(total - 1.0) < 2e-2                               # a step function on a grid of 4.5 M points
    # the draw's own term equals the density of the direction drawn (the rim rule changes nothing away from the rim) ...
    x1, x2 = LG._grid(64)
    k = len(x1)
    wd, gd = LG.draw(ob, np.broadcast_to(X0, (k, 3)), np.broadcast_to(v[0], (k, 3)), np.broadcast_to(aux[0], (k,)), x1, x2)
    ge = LG.density(ob, np.broadcast_to(X0, (k, 3)), np.broadcast_to(v[0], (k, 3)), np.broadcast_to(aux[0], (k,)), wd)
    np.testing.assert_allclose(np.linalg.norm(wd, axis=1), 1.0, rtol=1e-12)
    np.testing.assert_allclose(ge, gd, rtol=1e-9)
    # ... and the map (x1, x2) -> w has the Jacobian 1 / g: a finite-difference solid angle per cell
    h = 1e-5
    wa, _ = LG.draw(ob, np.broadcast_to(X0, (k, 3)), np.broadcast_to(v[0], (k, 3)), np.broadcast_to(aux[0], (k,)), x1 + h, x2)
    wb, _ = LG.draw(ob, np.broadcast_to(X0, (k, 3)), np.broadcast_to(v[0], (k, 3)), np.broadcast_to(aux[0], (k,)), x1, x2 + h)
    jac = np.abs(np.einsum("ij,ij->i", wd, np.cross(wa - wd, wb - wd))) / (h * h) / (2.0 * np.pi)
    np.testing.assert_allclose(jac, 1.0 / gd, rtol=2e-3)


def test_quadrature_mean_equals_the_analytic_mean():
    for beta in (0.0, 0.5, 0.9):
        mean = LG.one_bounce_moments([SPHERE], X0, N, 1.0, beta, q=512)[0]
        lamp = LG.stored([SPHERE])[0]                       # the binary32 values the library is given
        want = LG.sphere_lamp_mean(1.0, 100.0, lamp["centre"], lamp["radius"], X0, N)
        assert abs(mean - want) <= 1e-9 * want, (beta, mean, want)
    assert abs(want - 0.108253) < 1e-6


def test_worked_case():
    """The figures of the module docstring; an independent CPU Monte Carlo gave 9.39, 0.0117 and 0.0013."""
    m0, v0, _, d0 = LG.one_bounce_moments([SPHERE], X0, N, 1.0, 0.5, guided=False)
    m5, v5, _, d5 = LG.one_bounce_moments([SPHERE], X0, N, 1.0, 0.5)
    m9, v9, _, d9 = LG.one_bounce_moments([SPHERE], X0, N, 1.0, 0.9)
    print("sphere: mean %.6f variance %.5g / %.5g / %.5g" % (m0, v0, v5, v9))
    for m in (m0, m5, m9):
        assert abs(m - 0.108253) < 1e-6
    # the Monte Carlo estimates: 4e6 samples of an X that is 86.6 with probability 0.00125 put a standard error of
    # sqrt(86.6^4 x 0.00125 / 4e6) = 0.13 on the unguided variance (3 se allowed); the guided ones were quoted to two or three digits
    assert abs(v0 - 9.39) < 0.4 and abs(v5 - 0.0117) < 1e-4 and abs(v9 - 0.0013) < 1e-4
    v5_fine = LG.one_bounce_moments([SPHERE], X0, N, 1.0, 0.5, q=192)[1]
    assert abs(v5_fine - v5) < 1e-6 * v5                                                     # the quadrature has converged
    assert d0 == d5 == d9 == 0.0                                                             # wholly above the horizon
    # a lamp that straddles the horizon: the dead share is beta x the share of its draws that point below
    assert 0.0 < LG.one_bounce_moments([STRADDLE], X0, N, 1.0, 0.5)[3] < 0.5 * 0.5


@pytest.mark.parametrize("lamp", [SPHERE, DISC], ids=["sphere", "disc"])
def test_variance_ordering(lamp):
    v = [LG.one_bounce_moments([lamp], X0, N, 1.0, b, guided=g)[1] for b, g in ((0.5, False), (0.5, True), (0.9, True))]
    m = [LG.one_bounce_moments([lamp], X0, N, 1.0, b, guided=g)[0] for b, g in ((0.5, False), (0.5, True), (0.9, True))]
    print("means %s variances %s" % (m, v))
    assert v[0] > 100 * v[1] > 100 * v[2] > 0
    np.testing.assert_allclose(m, m[0], rtol=1e-9)


def test_table():
    objs = [dict(SPHERE), dict(shape="sphere", material="diffuse", centre=(0, 0, 9), radius=1.0, colour=(1, 1, 1)),
            dict(DISC, colour=(0.0, 0.0, 0.0)), dict(DISC, colour=(1.0, 2.0, 3.0)), dict(SPHERE, radius=0.1, colour=(0.0, 0.0, 0.0))]
    T = LG.Table(objs, 0.5)
    assert T.index == [0, 2, 3, 4] and T.active and T.n_draw == 3
    assert int(T.weight.sum()) == 1 << 32 and T.weight[1] == 0 and T.weight[3] == 0
    assert np.all(np.diff(T.threshold.astype(np.int64)) >= 0)
    y = 0.2126 * 1 + 0.7152 * 2 + 0.0722 * 3
    np.testing.assert_allclose(T.mass, [100 * 4 * float(np.float32(0.2)) ** 2, 0, y * 2 * float(np.float32(0.3)) ** 2, 0], rtol=1e-12)
    np.testing.assert_allclose(T.p.astype(np.float64), T.mass / T.mass.sum(), atol=2.0 ** -31)
    sel = T.select(np.array([0, T.threshold[0] - 1, T.threshold[0], 0xffffffff], np.uint32))
    assert list(sel) == [0, 0, 2, 2]
    assert not LG.Table(objs[1:3], 0.5).active and not LG.Table([], 0.5).active
    assert LG.Table(objs, 0.5).beta == 0.5 and float(LG.one_minus(0, T.beta_thr)) == 0.5


# ---- csrc/ptmi_light_guide.h itself, under the sanitizers, in a program of its own

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """light_guide_main, built with the sanitizers: nothing is loaded into Python."""
    out = str(tmp_path_factory.mktemp("light_guide") / "light_guide_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "light_guide_main.cpp")])
    return out


def test_table_and_rejections_under_the_sanitizers(exe):
    """Thresholds monotone, the integer weights sum to 2^32 and are what selection gives each rank, zero-mass emitters get
    p = 0, all-black or no emitters leave the guide inert, 32 emitters, every rejection names its field."""
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("scene", ["crowd", "single_emissive_disc", "single_diffuse_sphere", "mixed"])
def test_the_model_table_equals_the_header(exe, scene):
    if scene == "mixed":
        objs = [dict(SPHERE), dict(DISC, colour=(0.0, 0.0, 0.0)), dict(DISC, colour=(1.0, 2.0, 3.0)), dict(SPHERE, radius=0.1, colour=(0.0, 0.0, 0.0))]
    else:
        objs = M.SCENES[scene]
    lines = []
    for o in objs:
        disc = o["shape"] in ("disc", 1)
        mat = o["material"] if isinstance(o["material"], int) else {"diffuse": 0, "specular": 1, "refractive": 2, "emissive": 3}[o["material"]]
        vals = list(o["centre"]) + [o["radius"]] + list(o.get("normal", (0, 0, 0))) + list(o["colour"])
        lines.append("%d %d " % (1 if disc else 0, mat) + " ".join("%.9g" % np.float32(v) for v in vals))
    r = subprocess.run([exe, "table", "0.3"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = r.stdout.split("\n")
    n, n_draw, beta_thr, active = (int(x) for x in rows[0].split())
    T = LG.Table(objs, 0.3)
    assert (n, n_draw, beta_thr, bool(active)) == (T.n, T.n_draw, T.beta_thr, T.active)
    for k in range(n):
        idx, thr, weight, p, mass = rows[1 + k].split()
        assert int(idx) == T.index[k] and float(mass) == T.mass[k]
        if T.active:
            assert int(thr) == int(T.threshold[k]) and int(weight) == int(T.weight[k]) and np.float32(p) == T.p[k]


def test_both_guides_quadrature_reduces_to_the_single_guides():
    """The quadrature with an environment guide too (both_guides_moments): under a constant map and alpha = 0 it is
    one_bounce_moments; without a light branch (beta = 0) and with a black lamp it is env_guide_model's; and with both guides the
    mean does not move."""
    from tests import env_guide_model as EG
    sun = EG.sun_map()
    L = sun[..., 0].astype(np.float64)
    flat = np.full((8, 16, 3), 0.02, np.float32)
    x = np.array([[0.3, -0.2, 0.0], [-0.5, 0.4, 0.0]])
    got = LG.both_guides_moments([SPHERE], x, N, 0.8, 0.5, EG.Guide(flat, 8, 16, 0.0), flat[..., 0].astype(np.float64), q=64)
    want = LG.one_bounce_moments([SPHERE], x, N, 0.8, 0.5, sky=float(np.float32(0.02)), q=64)
    np.testing.assert_allclose(got[:3], want[:3], rtol=2e-4)
    black = dict(SPHERE, colour=(0.0, 0.0, 0.0))          # no mass: the light guide is inert and the table empty
    env = EG.Guide(sun, 32, 64, 0.5)
    got = LG.both_guides_moments([black], x, N, 1.0, 0.4, env, L)
    want = EG.one_bounce_moments(env, L, N)
    np.testing.assert_allclose(got[:2], want[:2], rtol=5e-3)
    both = LG.both_guides_moments([SPHERE], x, N, 1.0, 0.4, EG.Guide(sun, 32, 64, 0.3), L)
    none = LG.both_guides_moments([SPHERE], x, N, 1.0, 0.0, EG.Guide(sun, 32, 64, 0.0), L)
    assert abs(both[0] - none[0]) < 1e-3 * none[0] and both[1] < none[1] / 5
    assert abs(both[3] - EG.dead_share(EG.Guide(sun, 32, 64, 0.3), N)) < 1e-12
