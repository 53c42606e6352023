"""Cells a real caller hands over: off the origin, orthorhombic (`SimBoxInit::Pad` gives a negative, non-dyadic `box_lo` and three
different edges; `new_cube` is centred on the origin).  The system generators all build `box_lo = (0, 0, 0)`; `placed` moves one
of their systems to a cell elsewhere, optionally with longer edges.  References and minimum images in a test take the cell from
`cell_of(md)` - the fp32 values the handle holds - never from `s.box_hi` alone.

`record` notes the worst ratio of a comparison to its bound (MDX_MARGINS_OUT names the file: profiles/cell_placement_margins.txt
was written that way); without the variable it does nothing."""
import dataclasses
import math
import os

import numpy as np

PAD = (-31.7, 12.3, -57.9)      # mixed signs, non-dyadic
NEG = (-88.1, -61.3, -70.7)     # every coordinate of a <= 26 A system is negative (all |x| < 100 A)


def placed(s, lo, grow=(0.0, 0.0, 0.0)):
    """A copy of `s` in the cell [lo, lo + (hi0 - lo0) + grow]: positions shifted (in fp64, rounded to fp32), everything else
    untouched.  grow > 0 leaves a vacuum slab along that axis - still a legitimate periodic system."""
    lo = np.asarray(lo, np.float64)
    lo0, hi0 = np.asarray(s.box_lo, np.float64), np.asarray(s.box_hi, np.float64)
    pos = (np.asarray(s.pos, np.float64) + (lo - lo0)).astype(np.float32)
    hi = lo + (hi0 - lo0) + np.asarray(grow, np.float64)
    return dataclasses.replace(s, pos=pos, box_lo=tuple(float(v) for v in lo), box_hi=tuple(float(v) for v in hi))


def cell_of(md):
    """-> (lo, L = hi - lo) as fp64, from the cell the handle holds."""
    lo, hi = md.cell()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return lo, hi - lo


def min_image(d, L):
    d = np.asarray(d, np.float64)
    return d - np.round(d / L) * L


def rms_dev(a, b, L):
    d = min_image(np.asarray(a, np.float64) - np.asarray(b, np.float64), L)
    return math.sqrt((d ** 2).sum(1).mean())


def force_ratios(f_gpu, f_orc, slack=None):
    """What tests.test_gpu_parity.assert_forces asserts, as ratios to its two bounds: (worst per-atom, rms)."""
    f_gpu = np.asarray(f_gpu, np.float64)
    err = np.linalg.norm(f_gpu - f_orc, axis=1)
    tol = 1e-4 * np.maximum(np.linalg.norm(f_orc, axis=1), 1.0)
    clean = np.ones(len(err), bool)
    if slack is not None:
        tol = tol + slack
        clean = slack == 0
    rms = math.sqrt(np.mean(err[clean] ** 2)) / math.sqrt(np.mean((f_orc[clean] ** 2).sum(1)))
    return float((err / tol).max()), rms / 2e-5


def energy_ratio(e_gpu, e_orc):
    from tests.test_gpu_parity import TERMS, energy_tolerance
    return max(abs(e_gpu[k] - e_orc[k]) / energy_tolerance(e_orc, k) for k in TERMS)


def approx_ratio(a, b, rel=0.0, abs_=0.0):
    """|a - b| over pytest.approx's bound max(rel |b|, abs)."""
    return abs(a - b) / max(rel * abs(b), abs_)


def record(what, **ratios):
    path = os.environ.get("MDX_MARGINS_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(f"{what}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in ratios.items()) + "\n")
