"""The model of polygon lamps in the emitter guide (tests/light_guide_poly_model.py) against mathematics it does not assume, and
its MUTATIONS against these checks: each wrong version of a step must break one."""
import numpy as np
import pytest

from tests import light_guide_model as LM
from tests import light_guide_poly_model as LP

N = np.array([0.0, 1.0, 0.0])
X0 = np.array([0.1, 0.0, -0.2])
E = (10.0, 10.0, 10.0)
RECT = dict(shape="parallelogram", material="emissive", vertices=((-0.5, 3.0, -0.5), (0.5, 3.0, -0.5), (-0.5, 3.0, 0.5)), colour=E)
TRI = dict(shape="triangle", material="emissive", vertices=((-0.9, 0.4, -3.0), (0.9, 0.4, -3.0), (0.0, 0.45, -3.9)), colour=E)
SKEW = dict(shape="parallelogram", material="emissive", vertices=((1.0, 1.0, -1.0), (2.0, 1.5, -1.2), (1.2, 2.0, -0.4)), colour=E)
SLIVER = dict(shape="triangle", material="emissive", vertices=((0.0, 2.0, 0.0), (2.0, 2.5, 0.0), (2.0, 2.5, 0.01)), colour=E)
# the horizon of (X0, N) cuts this one: v0 is below it, the corner v1 above (d1 > 0 > d0)
STRADDLE = dict(shape="triangle", material="emissive", vertices=((3.0, -0.5, -0.4), (3.0, 0.7, -0.4), (3.0, -0.5, 0.4)), colour=E)
LAMPS = {"rect": RECT, "tri": TRI, "skew": SKEW, "sliver": SLIVER, "straddle": STRADDLE}


def _own_term_equals_density(lamp, mutation=None, q=32):
    x1, x2 = LM._grid(q)
    k = len(x1)
    x = np.broadcast_to(X0, (k, 3))
    ok, v, aux = LP.eligible(lamp, x, np.broadcast_to(N, (k, 3)), mutation=mutation)
    assert ok.all()
    wd, gd = LP.draw(lamp, x, v, aux, x1, x2, mutation=mutation)
    ge = LP.density(lamp, x, v, aux, wd, mutation=mutation)
    return wd, gd, ge


@pytest.mark.parametrize("name", list(LAMPS))
def test_density_integrates_to_one_over_the_lamp(name):
    """int over the lamp of g dw / 2 pi, by quadrature in AREA (dw = |m . w| dA / l^2): the density of the direction to a uniform
    point of the area integrates to 1 whatever part of the lamp is above the horizon."""
    total = LP.density_integral(LAMPS[name], X0, N, q=96)
    print("%s: int g dw / 2 pi = %.6f" % (name, total))
    assert abs(total - 1.0) < 5e-3        # points within rounding of an edge may miss: at most the boundary cells, 4 / q


@pytest.mark.parametrize("name", list(LAMPS))
def test_own_term_equals_the_density_at_the_drawn_direction(name):
    wd, gd, ge = _own_term_equals_density(LAMPS[name])
    np.testing.assert_allclose(np.linalg.norm(wd, axis=1), 1.0, rtol=1e-12)
    inside = ge > 0                        # a midpoint grid keeps away from the edges, but the fold puts points ON the diagonal
    assert inside.mean() > 0.95
    # l^3 / |hgt| against t^2 / |m . w|: equal but for the stored normal, a binary32 vector whose product with an edge is not
    # exactly 0 -- m . (a e1 + b e2) is at most 2^-24 sqrt(3) (|e1| + |e2|), here under 4e-7, against |hgt| >= 0.4
    np.testing.assert_allclose(ge[inside], gd[inside], rtol=2e-6)


def test_the_folded_draw_is_uniform_over_the_triangle():
    """Moments of the barycentric coordinates of the drawn points: over a triangle E[a] = E[b] = 1/3, E[a^2] = 1/6, E[a b] = 1/12,
    and no point leaves it."""
    v0, e1, e2 = (z.astype(np.float64) for z in LP.frame32(TRI)[:3])
    x1, x2 = LM._grid(400)
    k = len(x1)
    x = np.broadcast_to(X0, (k, 3))
    ok, v, aux = LP.eligible(TRI, x, np.broadcast_to(N, (k, 3)))
    wd, gd = LP.draw(TRI, x, v, aux, x1, x2)
    t = aux / (wd @ LP.frame32(TRI)[3].astype(np.float64))       # back to the point on the plane
    y = x + wd * t[:, None] - v0
    ab = np.linalg.lstsq(np.stack([e1, e2], 1), y.T, rcond=None)[0]
    a, b = ab[0], ab[1]
    assert a.min() > -1e-6 and b.min() > -1e-6 and (a + b).max() < 1 + 1e-6      # (the plane through the binary32 normal)
    for got, want in ((a.mean(), 1 / 3), (b.mean(), 1 / 3), ((a * a).mean(), 1 / 6), ((b * b).mean(), 1 / 6), ((a * b).mean(), 1 / 12)):
        assert abs(got - want) < 2e-3, (got, want)


def test_eligibility_is_some_corner_above_the_horizon():
    """eligible <=> |hgt| > eps and the highest corner (v . n over the four / three corners) is above the horizon."""
    rng = np.random.default_rng(5)
    for lamp in LAMPS.values():
        v0, e1, e2, m = (z.astype(np.float64) for z in LP.frame32(lamp)[:4])
        x = rng.uniform(-3, 3, (4000, 3))
        n = rng.normal(size=(4000, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        corners = [v0, v0 + e1, v0 + e2] + ([] if LP.is_triangle(lamp) else [v0 + e1 + e2])
        top = np.max(np.stack([np.einsum("ij,ij->i", c - x, n) for c in corners]), axis=0)
        hgt = (v0 - x) @ m
        want = (np.abs(hgt) > LP.EPS) & (top > 0)
        got = LP.eligible(lamp, x, n)[0]
        clear = np.abs(top) > 1e-9
        assert np.array_equal(got[clear], want[clear])
        assert 0.2 < got.mean() < 0.9


def test_table_masses_and_the_default():
    sphere = dict(shape="sphere", material="emissive", centre=(0, 0, 0), radius=0.5, colour=(2.0, 2.0, 2.0))
    black = dict(TRI, colour=(0.0, 0.0, 0.0))
    objs = [RECT, sphere, TRI, black, dict(RECT, material="diffuse")]
    T = LP.Table(objs, 0.5)
    assert T.index == [0, 1, 2, 3] and T.n_draw == 3 and T.lists_polygon
    y = 0.2126 * 10 + 0.7152 * 10 + 0.0722 * 10
    s_rect, s_tri = float(LP.frame32(RECT)[4]), float(LP.frame32(TRI)[4])
    np.testing.assert_allclose(T.mass, [y * 2 * s_rect / np.pi, 2.0 * (0.2126 + 0.7152 + 0.0722) * 4 * 0.25, y * 2 * 0.5 * s_tri / np.pi, 0.0],
                               rtol=1e-15)
    assert abs(s_rect - 1.0) < 1e-6 and abs(s_tri - np.linalg.norm(np.cross((1.8, 0, 0), (0.9, 0.05, -0.9)))) < 1e-6
    assert int(T.weight.sum()) == 1 << 32 and T.p[3] == 0 and abs(float(T.p.sum()) - 1) < 1e-6
    plain = LP.Table(objs, 0.5, polygons=False)                   # the four-argument call: the sphere alone, as before
    ref = LM.Table([sphere], 0.5)
    assert plain.index == [1] and not plain.lists_polygon and np.array_equal(plain.threshold, ref.threshold) and np.array_equal(plain.p, ref.p)


def test_quadrature_mean_is_the_configuration_factor():
    """One bounce under a parallel rectangular lamp: mean = colour E F / 2 (int cos dw / 2 pi over the lamp), F the point-to-parallel-rectangle configuration factor, for
    every beta; a triangle with half the area gives less than that and more than nothing; the guide cuts the variance."""
    x = np.array([[0.1, 0.0, -0.2], [0.7, 0.0, 0.4]])
    v = np.array(RECT["vertices"], np.float64)
    F = np.mean([LP.rectangle_form_factor(p, v[0], v[1] - v[0], v[2] - v[0], N) for p in x])
    var = []
    for beta, guided in ((0.5, False), (0.5, True), (0.9, True)):
        m1, v2, _, dead = LP.one_bounce_moments([RECT], x, N, 0.8, beta, q=128, guided=guided)
        assert abs(m1 - 0.8 * 10.0 * F / 2) < 1e-5 * m1 and dead == 0      # (the midpoint rule at q = 128: h^2 / 24 = 2.5e-6 times a second derivative of order 1)
        var.append(v2)
    print("rect lamp: F = %.6f, variance unguided %.4f, beta 0.5 %.4f, beta 0.9 %.4f" % (F, *var))
    assert var[0] > 4 * var[1] > 4 * var[2]
    half = dict(RECT, shape="triangle")
    mt = LP.one_bounce_moments([half], x, N, 0.8, 0.5, q=128)[0]
    assert 0.3 * m1 < mt < 0.7 * m1
    # not listed (the default of pt_set_light_guide): the unguided moments, whatever beta
    a = LP.one_bounce_moments([RECT], x, N, 0.8, 0.5, q=64, polygons=False)
    b = LP.one_bounce_moments([RECT], x, N, 0.8, 0.5, q=64, guided=False)
    np.testing.assert_allclose(a, b, rtol=1e-12)


def test_float32_error_of_the_formulas_is_small():
    """What the GPU test's bound is made of: float32 numpy against float64 numpy on the same inputs."""
    rng = np.random.default_rng(77)
    k = 1 << 12
    x = (rng.uniform(-1, 1, (k, 3)) * (0.5, 0.3, 0.5)).astype(np.float32)
    n = np.broadcast_to(N.astype(np.float32), (k, 3))
    g = rng.integers(0, 1 << 32, (3, k), dtype=np.uint64).astype(np.uint32)
    for lamp in (RECT, TRI):
        T = LP.Table([lamp], 0.5)
        d32, r32 = LP.sample(T, [lamp], x, n, g[0], g[1], g[2], np.float32)
        d64, r64 = LP.sample(T, [lamp], x, n, g[0], g[1], g[2], np.float64)
        assert np.array_equal(r32, r64) and (r64 == 0).all()
        err = np.abs(d32 - d64).max()
        print("float32 direction error %.2e" % err)
        assert 0 < err < 1e-5


# ---- each mutation breaks a check

def test_mutation_no_fold_leaves_the_triangle():
    wd, gd, ge = _own_term_equals_density(TRI, mutation="no_fold")
    assert (ge == 0).mean() > 0.4          # half the draws land outside: the density there is 0, not the own term


def test_mutation_area_not_halved_loses_half_the_mass():
    assert abs(LP.density_integral(TRI, X0, N, q=96, mutation="area_not_halved") - 0.5) < 5e-3
    assert abs(LP.density_integral(RECT, X0, N, q=96, mutation="area_not_halved") - 1.0) < 5e-3   # (a parallelogram is untouched)


def test_mutation_t_not_squared_is_no_density():
    assert abs(LP.density_integral(RECT, X0, N, q=96, mutation="t_not_squared") - 1.0) > 0.5
    wd, gd, ge = _own_term_equals_density(RECT, mutation="t_not_squared")
    assert not np.allclose(ge, gd, rtol=1e-3)


def test_mutation_reach_without_clamp_misses_a_visible_corner():
    """STRADDLE from X0: v0 and v2 are below the horizon of (X0, N), v1 above.  With d2 < 0 left unclamped a parallelogram's reach
    shrinks; for a triangle max(d1, d2) < 0 must not pull a visible v0 under."""
    par = dict(STRADDLE, shape="parallelogram", vertices=((3.0, -0.5, -0.4), (3.0, 0.4, -0.4), (3.0, -1.5, 0.4)))
    x, n = X0[None], N[None]
    assert LP.eligible(par, x, n)[0][0] and not LP.eligible(par, x, n, mutation="reach_without_clamp")[0][0]
    tri = dict(STRADDLE, vertices=((3.0, 0.2, -0.4), (3.0, -0.7, -0.4), (3.0, -0.5, 0.4)))
    assert LP.eligible(tri, x, n)[0][0] and not LP.eligible(tri, x, n, mutation="reach_without_clamp")[0][0]
    assert set(LP.MUTATIONS) == {"no_fold", "area_not_halved", "t_not_squared", "reach_without_clamp"}
