"""The half-list pair kernel's per-entry j-force tail ("per entry"): the last level of the reduction selects the
component first and adds once (mdx_pair_dev.h jforce_reduce8), the reaction accumulates with the sign it leaves with, the atomic's
address is a scalar base plus a lane offset, the eps strip has the position strip's stride.  Every one of them changes the instruction
count and none the floating-point operations or their operands.

test_reduction_bits: a test-only kernel (tests/cpp/jtail_reduce.hip, compiled here) runs the reduction as it was spelled before and the
helper on the same inputs; lanes ii < 3 of all eight j rows match bit for bit (see the file's head for the one thing that is not a bit:
the sign of a sum that is exactly zero, once the inputs arrive negated).

test_half_list_against_full_list: forces of the half-list kernels at fixed positions - plain list, pruning pass, inner-list walk -
against the deterministic full-list kernel (nb_variant 2) on the same positions, d = max |F_half - F_full| over the atoms.  The two sum
the same pair forces in different orders (and the half list through f32 atomics, in a run-dependent order), so d is rounding: a few
1e-5 kcal/mol/A.  Bound: d <= 2 x the d the IDENTICAL child gave on the build before this change (PARENT_D below, recorded with the
runs in profiles/jtail_ab.txt); the factor covers a maximum over ~1e4 atoms estimated from one sample - the addition trees are
unchanged, so nothing larger is expected.  Each case runs twice: s = max |dF| between the two runs is printed beside d."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "jtail_child.py")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# max |F_half - F_full| in kcal/mol/A of tests/jtail_child.py on the parent build, one MI355X run (profiles/jtail_ab.txt)
PARENT_D = {
    "water1": {"plain": 9.9182e-05, "prune": 9.9182e-05, "walk": 9.9182e-05},
    "water8": {"plain": 9.1553e-05, "prune": 1.2207e-04, "walk": 1.2207e-04},
    "solvated": {"plain": 4.5776e-05, "prune": 4.5776e-05, "walk": 4.5776e-05},
    "opc": {"plain": 1.5020e-04, "prune": 4.1199e-04, "walk": 4.2343e-04},
}
KNOBS = {"water1": "1", "water8": "8", "solvated": "1", "opc": "1"}


def test_reduction_bits(tmp_path):
    """One wave, 4096 rounds of random g[3] per lane: +-0, denormals, magnitudes 1e-30 .. 1e30.  No tolerance."""
    exe = str(tmp_path / "jtail_reduce")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "jtail_reduce.hip"), "-o", exe], check=True, timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout + p.stderr)
    assert p.returncode == 0 and "JTAIL-REDUCE-OK" in p.stdout, p.stdout + p.stderr


def run_child(which, path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_")}
    env.update(MDX_WPT=KNOBS[which], MDX_REBUILD_INNER="0")
    p = subprocess.run([sys.executable, CHILD, which, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "JTAIL-OK" in p.stdout, tail
    print(tail)
    return np.load(path)


@pytest.mark.parametrize("which", ["water1", "water8", "solvated", "opc"])
def test_half_list_against_full_list(tmp_path, which):
    r1 = run_child(which, str(tmp_path / f"{which}_1.npz"))
    r2 = run_child(which, str(tmp_path / f"{which}_2.npz"))
    assert np.array_equal(r1["full"].view(np.uint32), r2["full"].view(np.uint32)), "the yardstick is deterministic"
    full = r1["full"].astype(np.float64)
    assert np.isfinite(full).all() and float(np.abs(full).max()) > 1.0
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
