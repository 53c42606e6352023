"""The half-list pair kernel's i-force write-back ("the atomic budget"): a tile's i-forces leave as four contiguous
256-byte atomics through the wave's LDS strip instead of three strided ones (NB_IFORCE_ROWS, mdx_pair_dev.h iforce_add_rows).  That
changes the shape of the instructions, and neither a floating-point operand nor the word it is added to.

Each case (tests/atomic_path_child.py, one process per knob set): forces of the step loop's pair launch at fixed positions - the pruning
pass and the inner-list walk behind it - against the deterministic full-list kernel (nb_variant 2) on the same positions,
d = max |F_half - F_full| over the atoms; and the pruning pass against the walk, p = max |F_prune - F_walk|, within the same bound.  The
kernels sum the same pair forces in different orders (the half list through f32 atomics, in a run-dependent order), so d and p are
rounding.  Bound: 2 x the d the IDENTICAL child gave on the build before this change (PARENT_D below, recorded with the runs in
profiles/atomic_path_ab.txt); the factor is tests/test_gpu_jtail.py's: a maximum over ~1e4 atoms estimated from one sample, with
unchanged addition trees.  Each case runs twice: s = max |dF| between the two runs is printed beside d.

  tail0, tail4  one-wave units: a unit alone on its tile's rows, and four units per tile adding partial sums into the same rows
  wpt8          a multi-wave class (MDX_ONEPASS=0: the step loop's two-launch form, whose pair kernel has the new write-back): the tile's
                first wave adds the fixed-order sum of the eight waves (s_red)
  solvated      the general body, masked chunks"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "atomic_path_child.py")

KNOBS = {
    "tail0": dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL="0"),
    "tail4": dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL="4/1"),
    "wpt8": dict(MDX_WPT="8", MDX_ONEPASS="0"),
    "solvated": dict(MDX_WPT="1"),
}

# max |F_half - F_full| in kcal/mol/A of tests/atomic_path_child.py on the parent build, one MI355X run (profiles/atomic_path_ab.txt)
PARENT_D = {
    "tail0": {"prune": 9.9182e-05, "walk": 9.9182e-05},
    "tail4": {"prune": 9.9182e-05, "walk": 9.9182e-05},
    "wpt8": {"prune": 1.2207e-04, "walk": 1.2207e-04},
    "solvated": {"prune": 4.5776e-05, "walk": 4.5776e-05},
}
# (the same run's max |F_prune - F_walk|, printed beside p: the parent's own spread between its two half-list evaluations)
PARENT_P = {"tail0": 1.5259e-05, "tail4": 3.0518e-05, "wpt8": 6.1035e-05, "solvated": 1.5259e-05}


def run_child(which, path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_")}
    env.update(KNOBS[which], MDX_REBUILD_INNER="0")
    p = subprocess.run([sys.executable, CHILD, which, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "ATOMIC-PATH-OK" in p.stdout, tail
    print(tail)
    return np.load(path)


@pytest.mark.parametrize("which", ["tail0", "tail4", "wpt8", "solvated"])
def test_step_loop_forces_against_full_list(tmp_path, which):
    r1 = run_child(which, str(tmp_path / f"{which}_1.npz"))
    r2 = run_child(which, str(tmp_path / f"{which}_2.npz"))
    assert np.array_equal(r1["full"].view(np.uint32), r2["full"].view(np.uint32)), "the yardstick is deterministic"
    full = r1["full"].astype(np.float64)
    assert np.isfinite(full).all() and float(np.abs(full).max()) > 1.0
    worst = []
    for kind in ("prune", "walk"):
        a, b = r1[kind].astype(np.float64), r2[kind].astype(np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert float(np.abs(a).max()) > 1.0 and float(np.abs(b).max()) > 1.0
        d = max(float(np.abs(a - full).max()), float(np.abs(b - full).max()))
        s = float(np.abs(a - b).max())
        bound = 2.0 * PARENT_D[which][kind]
        print(f"{which} {kind}: d = max|F_half - F_full| {d:.4e}, run-to-run s {s:.4e}, parent d {PARENT_D[which][kind]:.4e}, bound {bound:.4e} kcal/mol/A")
        if not d <= bound:
            worst.append((kind, d, bound))
    # the pruning pass against the walk that follows it on the same positions, within the same bound
    p = max(float(np.abs(r["prune"].astype(np.float64) - r["walk"].astype(np.float64)).max()) for r in (r1, r2))
    bound = 2.0 * PARENT_D[which]["prune"]
    print(f"{which}: p = max|F_prune - F_walk| {p:.4e}, parent p {PARENT_P[which]:.4e}, bound {bound:.4e} kcal/mol/A")
    if not p <= bound:
        worst.append(("prune vs walk", p, bound))
    assert not worst, (which, worst)
