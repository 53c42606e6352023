"""The half-list pair kernel's chunk latch ("per chunk"): the one-wave kernels with the constant-sigma^2 body walk
their plain chunks two per trip with two sets of pipeline registers, so that the compiler's vector-memory wait comes once per two chunks
(mdx_nonbonded_impl.h, LATCH2); every chunk loop decodes its image shift through one helper (mdx_pair_dev.h image_shift_row).  Neither
changes a floating-point operand.  (The image-shift table the same change measured missed its bar as an arm of its own and is not in the
code, so there is no table to hold against the decode: profiles/walk_latch_ab.txt.)

test_half_list_against_full_list: as tests/test_gpu_jtail.py - forces of the half-list kernels at fixed positions (plain list, pruning
pass, inner-list walk) against the deterministic full-list kernel (nb_variant 2) on the same positions, a child process per case
(tests/walk_chunks_child.py), each case twice.  d = max |F_half - F_full| over the atoms is rounding: the two sum the same pair forces
in different orders, the half list through f32 atomics in a run-dependent order.  Bound: d <= 2 x the d the IDENTICAL child gave on the
build before this change (PARENT_D below, recorded with the runs in profiles/walk_latch_ab.txt); the factor covers a maximum over ~1e4
atoms estimated from one sample.  The full-list forces are the same bits in both runs.  The child reports which chunk loop ran: two sets
in water1, tail4 and opc (all three launches), one set in the multi-wave and general-body cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "walk_chunks_child.py")

# max |F_half - F_full| in kcal/mol/A of tests/walk_chunks_child.py on the parent build, one MI355X run (profiles/walk_latch_ab.txt)
PARENT_D = {
    "water1": {"plain": 9.9182e-05, "prune": 9.9182e-05, "walk": 9.9182e-05},
    "tail4": {"plain": 9.9182e-05, "prune": 9.9182e-05, "walk": 9.9182e-05},
    "water8": {"plain": 9.1553e-05, "prune": 1.2207e-04, "walk": 1.2207e-04},
    "solvated1": {"plain": 4.5776e-05, "prune": 4.5776e-05, "walk": 4.5776e-05},
    "solvated8": {"plain": 4.5776e-05, "prune": 4.5776e-05, "walk": 4.5776e-05},
    "opc": {"plain": 1.5020e-04, "prune": 4.1199e-04, "walk": 4.2343e-04},
}
KNOBS = {
    "water1": dict(MDX_WPT="1"),
    "tail4": dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL="4/1"),
    "water8": dict(MDX_WPT="8"),
    "solvated1": dict(MDX_WPT="1"),
    "solvated8": dict(MDX_WPT="8"),
    "opc": dict(MDX_WPT="1"),
}
# which launches of a case run the chunk loop with two register sets, in the child's order (plain, prune, walk)
TWO_SETS = {"water1": (True, True, True), "tail4": (True, True, True), "water8": (False, False, False),
            "solvated1": (False, False, False), "solvated8": (False, False, False), "opc": (True, True, True)}


def run_child(which, path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_")}
    env.update(KNOBS[which], MDX_REBUILD_INNER="0")
    p = subprocess.run([sys.executable, CHILD, which, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "WALK-CHUNKS-OK" in p.stdout, tail
    print(tail)
    return np.load(path)


@pytest.mark.parametrize("which", ["water1", "tail4", "water8", "solvated1", "solvated8", "opc"])
def test_half_list_against_full_list(tmp_path, which):
    r1 = run_child(which, str(tmp_path / f"{which}_1.npz"))
    r2 = run_child(which, str(tmp_path / f"{which}_2.npz"))
    assert np.array_equal(r1["full"].view(np.uint32), r2["full"].view(np.uint32)), "the yardstick is deterministic"
    full = r1["full"].astype(np.float64)
    assert np.isfinite(full).all() and float(np.abs(full).max()) > 1.0
    for r in (r1, r2):
        for want, got, kind in zip(TWO_SETS[which], r["two_sets"].tolist(), ("plain", "prune", "walk")):
            assert want is None or bool(got) == want, (which, kind, "two register sets" if got else "one register set")
    worst = []
    for kind in ("plain", "prune", "walk"):
        a, b = r1[kind].astype(np.float64), r2[kind].astype(np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        d = max(float(np.abs(a - full).max()), float(np.abs(b - full).max()))
        s = float(np.abs(a - b).max())
        bound = 2.0 * PARENT_D[which][kind]
        print(f"{which} {kind}: d = max|F_half - F_full| {d:.3e}, run-to-run s {s:.3e}, parent d {PARENT_D[which][kind]:.3e}, bound {bound:.3e} kcal/mol/A")
        if not d <= bound:
            worst.append((kind, d, bound))
    assert not worst, (which, worst)
