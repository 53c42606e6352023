"""BAR and MBAR estimators of molchanica_amd/alchemical.py on states with a known free energy (CPU only): harmonic wells
U_k = kappa_k x^2 / 2, sampled exactly, have Delta F = (kT / 2) ln(kappa_K / kappa_0)."""
import math

import numpy as np
import pytest

from molchanica_amd import alchemical as A

T = 300.0
KT = A.KB_KCAL_MOL_K * T


def harmonic_windows(kappas, lams, n, seed):
    """Windows of snapshot dicts as MdState.snapshots returns them: foreign_du[k] = U_k(x) - U_own(x)."""
    rng = np.random.default_rng(seed)
    kap = np.asarray(kappas, dtype=np.float64)
    out = []
    for i, lam in enumerate(lams):
        x = rng.normal(0.0, math.sqrt(KT / kap[i]), n)
        u = 0.5 * kap[None, :] * x[:, None] ** 2
        du = u - u[:, [i]]
        snaps = [dict(energy_data=dict(dh_dlambda=0.0, foreign_du=du[j], foreign_lambdas=np.asarray(lams))) for j in range(n)]
        out.append(A.collect_window(lam, snaps))
    return out


def test_kb_is_the_library_constant():
    assert A.KB_KCAL_MOL_K == 0.0019872041


def test_collect_window_keeps_the_foreign_energies():
    ws = harmonic_windows([1.0, 2.0, 4.0], [0.0, 0.5, 1.0], 50, 3)
    assert ws[1].foreign_du.shape == (50, 3) and np.array_equal(ws[1].foreign_lambdas, [0.0, 0.5, 1.0])
    assert (ws[1].foreign_du[:, 1] == 0.0).all()
    w = A.collect_window(0.2, [dict(energy_data=dict(dh_dlambda=1.0))])     # without foreign data: the TI window as before
    assert w.foreign_du is None and w.foreign_lambdas is None and w.mean_dh_dl == 1.0


@pytest.mark.parametrize("seed", [1, 2])
def test_bar_and_mbar_recover_the_harmonic_free_energy(seed):
    lams = np.linspace(0.0, 1.0, 7)
    kappas = 1.0 * (16.0 / 1.0) ** lams
    exact = 0.5 * KT * math.log(kappas[-1] / kappas[0])
    ws = harmonic_windows(kappas, lams, 1500, seed)
    bar, bar_sem = A.free_energy_bar_with_sem(ws, T)
    mbar, mbar_sem = A.free_energy_mbar_with_sem(ws, T)
    # 1500 independent samples per window, adjacent wells a factor 1.59 apart: the SEM is ~6e-3 kcal/mol; bound 0.02
    for est, sem in ((bar, bar_sem), (mbar, mbar_sem)):
        assert 0.0 < sem < 0.02, sem
        assert abs(est - exact) <= 4.0 * sem, (est, exact, sem)


def test_mbar_on_two_states_equals_bar():
    ws = harmonic_windows([1.0, 3.0], [0.0, 1.0], 800, 7)
    bar, bar_sem = A.free_energy_bar_with_sem(ws, T)
    mbar, mbar_sem = A.free_energy_mbar_with_sem(ws, T)
    assert abs(mbar - bar) <= 1e-8
    assert mbar_sem == pytest.approx(bar_sem, rel=1e-3)


def test_identical_states_give_zero():
    ws = harmonic_windows([2.0, 2.0, 2.0], [0.0, 0.5, 1.0], 300, 4)
    bar, bar_sem = A.free_energy_bar_with_sem(ws, T)
    mbar, mbar_sem = A.free_energy_mbar_with_sem(ws, T)
    assert abs(bar) < 1e-12 and abs(mbar) < 1e-12
    assert bar_sem < 1e-6 and mbar_sem < 1e-6


def test_missing_foreign_data_raises():
    ws = harmonic_windows([1.0, 2.0, 4.0], [0.0, 0.5, 1.0], 40, 5)
    bare = A.collect_window(0.5, [dict(energy_data=dict(dh_dlambda=0.0))] * 40)
    for f in (A.free_energy_bar_with_sem, A.free_energy_mbar_with_sem):
        with pytest.raises(A.AlchemicalError):
            f([ws[0], bare, ws[2]], T)
    # a window without a neighbour's lambda among its foreign lambdas
    short = harmonic_windows([1.0, 2.0], [0.0, 0.5], 40, 6)
    for f in (A.free_energy_bar_with_sem, A.free_energy_mbar_with_sem):
        with pytest.raises(A.AlchemicalError):
            f(short + [ws[2]], T)
    with pytest.raises(A.AlchemicalError):
        A.free_energy_mbar_with_sem([ws[0]], T)


def test_statistical_inefficiency_of_a_correlated_series():
    rng = np.random.default_rng(9)
    assert A.statistical_inefficiency(rng.normal(size=4000)) == pytest.approx(1.0, abs=0.3)
    # AR(1) with phi = 0.8: g = (1 + phi) / (1 - phi) = 9
    x = np.zeros(20000)
    e = rng.normal(size=x.size)
    for t in range(1, x.size):
        x[t] = 0.8 * x[t - 1] + e[t]
    assert A.statistical_inefficiency(x) == pytest.approx(9.0, rel=0.25)
    assert A.statistical_inefficiency(np.ones(10)) == 1.0
