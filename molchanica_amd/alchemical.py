"""Host-side bookkeeping of thermodynamic-integration windows, named after the `dynamics::alchemical` items
Molchanica imports (src/properties/water_sol.rs:19-21, 442, 516, 568): `LambdaWindow`, `collect_window`,
`free_energy_ti_with_sem`, `mean_coupled_interaction_kcal`.  Their bodies live in the absent crate; what is
built: sample mean and standard error of dH/dlambda per window (block averaging against correlation),
trapezoidal integration over lambda with the errors of the windows propagated in quadrature.

Beside TI, the windows' foreign-lambda energy differences (dU_k = U(lambda_k) - U(lambda) of every snapshot, mdx_set_foreign_lambdas)
feed two estimators without quadrature bias: BAR between adjacent windows (`free_energy_bar_with_sem`) and MBAR over all windows
(`free_energy_mbar_with_sem`).  Both first decorrelate every window's series (`statistical_inefficiency`, subsampling at its stride)
and report Delta F of decoupling, lambda 0 -> 1 (the TI sign), with the asymptotic standard error."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

KB_KCAL_MOL_K = 0.0019872041     # MDX_KB (include/mdx.h)


class AlchemicalError(ValueError):
    pass


@dataclass
class LambdaWindow:
    lam: float
    mean_dh_dl: float            # kcal/mol
    sem_dh_dl: float             # kcal/mol
    n_samples: int
    samples: list = field(default_factory=list, repr=False)
    foreign_lambdas: np.ndarray | None = field(default=None, repr=False)   # [K] the lambdas of the snapshots' foreign_du
    foreign_du: np.ndarray | None = field(default=None, repr=False)        # [n_samples, K] U(lambda_k) - U(lam), kcal/mol

    @property
    def lambda_(self):           # `window.lambda` in the reference; `lambda` is a Python keyword
        return self.lam


def _sem(xs, n_blocks=5):
    """Standard error of the mean from block averages (falls back to the plain SEM for short series)."""
    n = len(xs)
    if n < 2:
        return 0.0
    if n < 2 * n_blocks:
        m = sum(xs) / n
        return math.sqrt(sum((x - m) ** 2 for x in xs) / (n - 1) / n)
    size = n // n_blocks
    means = [sum(xs[b * size:(b + 1) * size]) / size for b in range(n_blocks)]
    m = sum(means) / n_blocks
    return math.sqrt(sum((x - m) ** 2 for x in means) / (n_blocks - 1) / n_blocks)


def collect_window(lam: float, snapshots) -> LambdaWindow:
    """`collect_window(lambda, &md.snapshots)`: the snapshots' `dh_dlambda` samples of one window."""
    xs = [float(s["energy_data"]["dh_dlambda"] if "energy_data" in s else s["dh_dlambda"]) for s in snapshots]
    if not xs:
        raise AlchemicalError("no snapshots in the window")
    if any(not math.isfinite(x) for x in xs):
        raise AlchemicalError("non-finite dH/dlambda sample")
    w = LambdaWindow(float(lam), sum(xs) / len(xs), _sem(xs), len(xs), xs)
    eds = [s["energy_data"] if "energy_data" in s else s for s in snapshots]
    if all("foreign_du" in e and "foreign_lambdas" in e for e in eds):
        lams = np.asarray(eds[0]["foreign_lambdas"], dtype=np.float64).reshape(-1)
        if any(not np.array_equal(np.asarray(e["foreign_lambdas"], dtype=np.float64).reshape(-1), lams) for e in eds):
            raise AlchemicalError("the snapshots of one window carry different foreign lambdas")
        w.foreign_lambdas = lams
        w.foreign_du = np.stack([np.asarray(e["foreign_du"], dtype=np.float64).reshape(-1) for e in eds])
    return w


def free_energy_ti_with_sem(windows) -> tuple[float, float]:
    """Trapezoidal integral of <dH/dlambda> over lambda and its standard error (kcal/mol)."""
    ws = sorted(windows, key=lambda w: w.lam)
    if len(ws) < 2:
        raise AlchemicalError("thermodynamic integration needs at least two windows")
    if any(b.lam <= a.lam for a, b in zip(ws, ws[1:])):
        raise AlchemicalError("duplicate lambda values")
    weights = []
    for k in range(len(ws)):
        lo = ws[k].lam - ws[k - 1].lam if k > 0 else 0.0
        hi = ws[k + 1].lam - ws[k].lam if k + 1 < len(ws) else 0.0
        weights.append(0.5 * (lo + hi))
    dg = sum(w * x.mean_dh_dl for w, x in zip(weights, ws))
    sem = math.sqrt(sum((w * x.sem_dh_dl) ** 2 for w, x in zip(weights, ws)))
    return dg, sem


def mean_coupled_interaction_kcal(snapshots):
    """Mean solute-environment interaction energy over the snapshots of a window (None without samples)."""
    xs = [float(s["energy_data"]["coupled_interaction"] if "energy_data" in s else s["coupled_interaction"]) for s in snapshots]
    return sum(xs) / len(xs) if xs else None


# ---- BAR / MBAR ----------------------------------------------------------------------------------------------------------------------

def statistical_inefficiency(x) -> float:
    """g = 1 + 2 sum_t (1 - t/N) C(t) of a time series, C the normalised autocorrelation, the sum stopped at the first C(t) <= 0
    past t = 3 (Chodera et al., J. Chem. Theory Comput. 3, 26 (2007)).  1 for a constant or too short series."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    if n < 3:
        return 1.0
    dx = x - x.mean()
    var = float(dx @ dx) / n
    if not var > 0.0:
        return 1.0
    g = 1.0
    for t in range(1, n - 1):
        c = float(dx[:n - t] @ dx[t:]) / ((n - t) * var)
        if c <= 0.0 and t > 3:
            break
        g += 2.0 * c * (1.0 - t / n)
    return max(1.0, g)


def _subsample(n: int, g: float) -> np.ndarray:
    """Indices of a series of n samples kept at stride g (every sample when g = 1)."""
    idx = np.unique(np.round(np.arange(0.0, n, max(1.0, g))).astype(np.int64))
    return idx[idx < n]


def _column(w: LambdaWindow, lam: float) -> int:
    if w.foreign_du is None or w.foreign_lambdas is None:
        raise AlchemicalError(f"window lambda={w.lam} carries no foreign-lambda energies (mdx_set_foreign_lambdas before sampling)")
    hit = np.flatnonzero(np.abs(w.foreign_lambdas - lam) <= 1e-9)
    if not hit.size:
        raise AlchemicalError(f"window lambda={w.lam} lacks the foreign lambda {lam}")
    return int(hit[0])


def _sorted_windows(windows) -> list:
    ws = sorted(windows, key=lambda w: w.lam)
    if len(ws) < 2:
        raise AlchemicalError("a free-energy estimate needs at least two windows")
    if any(b.lam <= a.lam for a, b in zip(ws, ws[1:])):
        raise AlchemicalError("duplicate lambda values")
    return ws


def _decorrelated(ws, cols_of) -> list:
    """Per window: the rows kept after subsampling at the largest statistical inefficiency of the columns the estimator reads."""
    out = []
    for i, w in enumerate(ws):
        cols = cols_of(i, w)
        du = w.foreign_du[:, cols]
        if not np.isfinite(du).all():
            raise AlchemicalError(f"non-finite foreign-lambda energy in window lambda={w.lam}")
        g = max([statistical_inefficiency(du[:, j]) for j in range(du.shape[1])] + [1.0])
        out.append(_subsample(du.shape[0], g))
    return out


def _log_expit(x):
    """log(1 / (1 + exp(x))), stable for either sign."""
    return -np.logaddexp(0.0, x)


def _bar_pair(w_f, w_r) -> tuple[float, float]:
    """Bennett's acceptance ratio in reduced units: w_f = beta dU(0 -> 1) sampled in state 0, w_r = beta dU(1 -> 0) sampled in state 1.
    -> (Delta f = f_1 - f_0, its asymptotic variance; Shirts et al., Phys. Rev. Lett. 91, 140601 (2003))."""
    nf, nr = w_f.shape[0], w_r.shape[0]
    if nf < 1 or nr < 1:
        raise AlchemicalError("BAR needs samples on both sides")
    m = math.log(nf / nr)

    def imbalance(df):      # log sum_F fermi(M + w_F - df) - log sum_R fermi(-M + w_R + df): increasing in df, 0 at the solution
        a = np.logaddexp.reduce(_log_expit(m + w_f - df))
        b = np.logaddexp.reduce(_log_expit(-m + w_r + df))
        return float(a - b)

    # bracket from the two exponential averages, widened until the sign changes
    lo = float(min(w_f.min(), -w_r.max())) - 1.0
    hi = float(max(w_f.max(), -w_r.min())) + 1.0
    while imbalance(lo) > 0.0:
        lo -= 2.0 * (hi - lo)
    while imbalance(hi) < 0.0:
        hi += 2.0 * (hi - lo)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if imbalance(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    df = 0.5 * (lo + hi)
    f_f = np.exp(_log_expit(m + w_f - df))
    f_r = np.exp(_log_expit(-m + w_r + df))
    var = (np.mean(f_f ** 2) / np.mean(f_f) ** 2) / nf + (np.mean(f_r ** 2) / np.mean(f_r) ** 2) / nr - 1.0 / nf - 1.0 / nr
    return df, max(float(var), 0.0)


def free_energy_bar_with_sem(windows, temperature: float) -> tuple[float, float]:
    """Delta F (kcal/mol) from the first to the last window by BAR between every pair of adjacent windows, and its standard error: the
    pairs' asymptotic variances add (the pairs share no samples' estimates beyond their windows, treated as independent).
    Every window needs the foreign lambdas of its neighbours; each window's series is decorrelated first."""
    if not temperature > 0.0:
        raise AlchemicalError("temperature must be > 0")
    ws = _sorted_windows(windows)
    beta = 1.0 / (KB_KCAL_MOL_K * temperature)

    def cols_of(i, w):
        return [_column(w, ws[j].lam) for j in (i - 1, i + 1) if 0 <= j < len(ws)]

    keep = _decorrelated(ws, cols_of)
    df = var = 0.0
    for i in range(len(ws) - 1):
        a, b = ws[i], ws[i + 1]
        w_f = beta * a.foreign_du[keep[i], _column(a, b.lam)]
        w_r = beta * b.foreign_du[keep[i + 1], _column(b, a.lam)]
        d, v = _bar_pair(w_f, w_r)
        df += d
        var += v
    return df / beta, math.sqrt(var) / beta


def _mbar_solve(u_kn, n_k, f0, tol=1e-12, max_iter=100000):
    """Self-consistent MBAR equations (Shirts & Chodera, J. Chem. Phys. 129, 124105 (2008)) in log-sum-exp form:
    f_i = -log sum_n exp(-u_in - log D_n),  log D_n = log sum_k N_k exp(f_k - u_kn);  f_0 = 0."""
    log_n = np.log(n_k.astype(np.float64))
    f = f0 - f0[0]
    for _ in range(max_iter):
        log_d = np.logaddexp.reduce(log_n[:, None] + f[:, None] - u_kn, axis=0)
        f_new = -np.logaddexp.reduce(-u_kn - log_d[None, :], axis=1)
        f_new -= f_new[0]
        if np.max(np.abs(f_new - f)) < tol:
            f = f_new
            break
        f = f_new
    log_d = np.logaddexp.reduce(log_n[:, None] + f[:, None] - u_kn, axis=0)
    return f, log_d


def free_energy_mbar_with_sem(windows, temperature: float) -> tuple[float, float]:
    """Delta F (kcal/mol) from the first to the last window by MBAR over all windows, and its standard error from the asymptotic
    covariance (Shirts & Chodera 2008, Eq. D8, through the thin SVD of the weight matrix).  Every window needs the foreign lambdas of
    every window; each window's series is decorrelated first."""
    if not temperature > 0.0:
        raise AlchemicalError("temperature must be > 0")
    ws = _sorted_windows(windows)
    beta = 1.0 / (KB_KCAL_MOL_K * temperature)
    lams = [w.lam for w in ws]
    keep = _decorrelated(ws, lambda i, w: [_column(w, l) for l in lams if l != w.lam])
    # u_kn: reduced energy of every kept sample in every state, relative to the state it was drawn in (a per-sample constant cancels)
    blocks = [beta * w.foreign_du[np.ix_(keep[i], [_column(w, l) for l in lams])].T for i, w in enumerate(ws)]
    u_kn = np.concatenate(blocks, axis=1)
    n_k = np.array([len(k) for k in keep], dtype=np.int64)
    # start from the BAR chain of adjacent windows (the fixed point then needs few sweeps)
    f0 = np.zeros(len(ws))
    off = np.concatenate([[0], np.cumsum(n_k)])
    for i in range(len(ws) - 1):
        d, _ = _bar_pair(u_kn[i + 1, off[i]:off[i + 1]] - u_kn[i, off[i]:off[i + 1]],
                         u_kn[i, off[i + 1]:off[i + 2]] - u_kn[i + 1, off[i + 1]:off[i + 2]])
        f0[i + 1] = f0[i] + d
    f, log_d = _mbar_solve(u_kn, n_k, f0)
    w_nk = np.exp(f[None, :] - u_kn.T - log_d[:, None])             # [N, K], every column sums to 1
    _, s, vt = np.linalg.svd(w_nk, full_matrices=False)
    v = vt.T
    inner = np.eye(len(ws)) - np.diag(s) @ v.T @ np.diag(n_k.astype(np.float64)) @ v @ np.diag(s)
    theta = v @ np.diag(s) @ np.linalg.pinv(inner, rcond=1e-10, hermitian=True) @ np.diag(s) @ v.T    # (one zero eigenvalue: f is fixed up to a constant)
    var = theta[0, 0] + theta[-1, -1] - 2.0 * theta[0, -1]
    return float(f[-1] - f[0]) / beta, math.sqrt(max(float(var), 0.0)) / beta
