"""CPU: the float64 restraint reference (tests/restraint_ref.py) against finite differences - F = -grad E, and the virial
W = -dE/dlambda under a uniform scaling of positions and box-fractional references (flat-bottom atoms and references across a
periodic seam included)."""
import numpy as np
import pytest

from tests.restraint_ref import restraint_efw, scale_about, verlet_free


def _case(seed=3, n_atoms=40, n_res=25):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-5.0, 0.0, 2.0]), np.array([25.0, 28.0, 33.0])
    x = lo + rng.random((n_atoms, 3)) * (hi - lo)
    idx = rng.choice(n_atoms, n_res, replace=False)
    ref = x[idx] + rng.normal(0.0, 0.8, (n_res, 3))
    # five references across the seam: one box edge away from their atoms along x and z
    ref[:5] = x[idx[:5]] + np.array([0.4, -0.3, 0.2]) - np.where(x[idx[:5]] - lo > 0.5 * (hi - lo), 1.0, -1.0) * (hi - lo) * np.array([1, 0, 1])
    k = rng.uniform(0.5, 20.0, n_res)
    b = np.where(np.arange(n_res) % 3 == 0, 0.0, rng.uniform(0.0, 1.5, n_res))
    return x, idx, ref, k, b, lo, hi


@pytest.mark.parametrize("periodic", [(True, True, True), (True, False, True), (False, False, False)])
def test_force_is_minus_gradient(periodic):
    x, idx, ref, k, b, lo, hi = _case()
    e, f, _ = restraint_efw(x, idx, ref, k, b, lo, hi, periodic)
    assert e > 0
    h = 1e-5
    for i in idx[:12]:
        for a in range(3):
            xp = x.copy(); xp[i, a] += h
            xm = x.copy(); xm[i, a] -= h
            g = (restraint_efw(xp, idx, ref, k, b, lo, hi, periodic)[0] - restraint_efw(xm, idx, ref, k, b, lo, hi, periodic)[0]) / (2 * h)
            assert abs(-g - f[i, a]) <= 1e-6 * max(1.0, abs(e)), (i, a, -g, f[i, a])


def test_flat_bottom_inside_is_free_and_zero_distance_is_safe():
    x = np.zeros((3, 3)); x[1] = [0.3, 0, 0]; x[2] = [2.0, 0, 0]
    e, f, w = restraint_efw(x, [0, 1, 2], np.zeros((3, 3)), 5.0, [0.0, 0.5, 0.5])
    assert np.isfinite(f).all() and (f[:2] == 0).all()
    assert e == pytest.approx(5.0 * 1.5 ** 2) and f[2, 0] == pytest.approx(-2 * 5.0 * 1.5)
    assert w == pytest.approx(2.0 * f[2, 0])


@pytest.mark.parametrize("periodic", [(True, True, True), (True, False, True)])
def test_virial_is_minus_dE_dlambda(periodic):
    """Positions and periodic-axis references scale about box_lo with the box (fractional references); W = -dE/dlambda."""
    x, idx, ref, k, b, lo, hi = _case(seed=7)
    per = np.array(periodic)

    def energy(lam):
        lam_v = np.where(per, lam, 1.0)      # a non-periodic axis does not scale (absolute reference, absolute coordinates)
        xs = lo + lam_v * (x - lo)
        rs = lo + lam_v * (ref - lo)
        return restraint_efw(xs, idx, rs, k, b, lo, lo + lam_v * (hi - lo), periodic)[0]

    _, f, w = restraint_efw(x, idx, ref, k, b, lo, hi, periodic)
    h = 1e-6
    dedl = (energy(1 + h) - energy(1 - h)) / (2 * h)
    if all(periodic):
        assert w == pytest.approx(-dedl, rel=1e-6, abs=1e-8)
    else:       # only the periodic axes' part of W is the derivative
        d = x[idx] - ref
        L = hi - lo
        d -= np.where(per, np.round(d / L) * L, 0.0)
        w_per = float((d * f[idx])[:, per].sum())
        assert w_per == pytest.approx(-dedl, rel=1e-6, abs=1e-8)


def test_scale_about_matches_fractional_reference():
    lo, hi = np.array([1.0, 2.0, 3.0]), np.array([31.0, 22.0, 43.0])
    r = np.array([[5.0, 7.0, 40.0]])
    frac = (r - lo) / (hi - lo)
    c = 0.5 * (lo + hi); mu = 0.97
    lo2, hi2 = scale_about(lo, c, mu), scale_about(hi, c, mu)
    assert np.allclose(lo2 + frac * (hi2 - lo2), scale_about(r, c, mu), atol=1e-12)


def test_free_dynamics_conserves_energy():
    x, idx, ref, k, b, lo, hi = _case(seed=5)
    m = np.full(len(x), 12.0)
    v = np.random.default_rng(1).normal(0, 0.01, x.shape)
    per = (True, True, True)

    def tot(xx, vv):
        return restraint_efw(xx, idx, ref, k, b, lo, hi, per)[0] + 0.5 * (m[:, None] * vv ** 2).sum() / 418.4

    e0 = tot(x, v)
    x1, v1 = verlet_free(x, v, m, idx, ref, k, b, 0.0005, 400, lo, hi, per)
    assert abs(tot(x1, v1) - e0) < 1e-3 * max(1.0, abs(e0))
    free = np.setdiff1d(np.arange(len(x)), idx)
    assert np.allclose(x1[free], x[free] + 400 * 0.0005 * v[free], atol=1e-9)
