"""Float64 statement of the position restraints of include/mdx.h (mdx_set_position_restraints):

    d   = x_i - r0_i            (minimum image along the periodic axes)
    E_i = k_i max(0, |d| - b_i)^2
    F_i = -2 k_i (|d| - b_i) d / |d|   for |d| > b_i, else 0
    W_i = d . F_i

On a periodic axis the reference is box-fractional: it scales with the box like an atom does."""
from __future__ import annotations

import numpy as np

ACC_CONV = 418.4


def _min_image(d, box_lo, box_hi, periodic):
    d = np.array(d, np.float64)
    if box_lo is None:
        return d
    L = np.asarray(box_hi, np.float64) - np.asarray(box_lo, np.float64)
    for a in range(3):
        if periodic[a]:
            d[:, a] -= np.round(d[:, a] / L[a]) * L[a]
    return d


def restraint_efw(x, idx, ref, k, b=None, box_lo=None, box_hi=None, periodic=(False, False, False)):
    """-> (E, F [N, 3], W): energy, force on every atom (zero on unrestrained ones), virial d . F."""
    x = np.asarray(x, np.float64)
    idx = np.asarray(idx, np.int64)
    n = idx.shape[0]
    ref = np.asarray(ref, np.float64).reshape(n, 3)
    k = np.broadcast_to(np.asarray(k, np.float64), (n,))
    b = np.zeros(n) if b is None else np.broadcast_to(np.asarray(b, np.float64), (n,))
    d = _min_image(x[idx] - ref, box_lo, box_hi, periodic)
    r = np.sqrt((d ** 2).sum(1))
    ex = r - b
    on = ex > 0
    e = float((k[on] * ex[on] ** 2).sum())
    fi = np.zeros((n, 3))
    fi[on] = (-2.0 * k[on] * ex[on] / r[on])[:, None] * d[on]
    F = np.zeros_like(x)
    np.add.at(F, idx, fi)
    w = float((d * fi).sum())
    return e, F, w


def scale_about(p, origin, lam):
    """Affine map of points about `origin` (what the barostat does about box_lo and set_cell + scaled positions do)."""
    o = np.asarray(origin, np.float64)
    return o + lam * (np.asarray(p, np.float64) - o)


def verlet_free(x, v, m, idx, ref, k, b, dt, n_steps, box_lo=None, box_hi=None, periodic=(False, False, False)):
    """Velocity Verlet of atoms that feel nothing but their restraints (free atoms move in straight lines):
    a = F 418.4 / m.  -> (x, v) after n_steps, unwrapped."""
    x = np.array(x, np.float64); v = np.array(v, np.float64)
    inv = ACC_CONV / np.asarray(m, np.float64)[:, None]
    _, f, _ = restraint_efw(x, idx, ref, k, b, box_lo, box_hi, periodic)
    for _ in range(n_steps):
        v += 0.5 * dt * f * inv
        x += dt * v
        _, f, _ = restraint_efw(x, idx, ref, k, b, box_lo, box_hi, periodic)
        v += 0.5 * dt * f * inv
    return x, v
