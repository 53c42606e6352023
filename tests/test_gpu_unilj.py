"""The pair kernel's constant-sigma^2 body (UNI): handles in which every atom with a Lennard-Jones well carries the
same sigma multiply by the one f32 value sigma_ij^2 can take instead of adding and squaring per pair.  The claim is "the same bits";
MDX_UNI_LJ=0 gives the general body back.  The knob is read once per process, so every arm runs in a child (tests/unilj_child.py).

Bounds.  The full-list kernel (nb_variant 2) has no atomics: on against off is compared bit for bit, no tolerance.  The half-list
bodies the bench line times add j-forces with f32 atomics in a run-dependent order, so two runs of ONE build already differ: the off
arm runs twice, s = max |dF| between the two, and on against off must stay within 4 s (the factor covers the tail of a maximum over
12 k atoms estimated from two samples).  Measured on an MI355X (profiles/unilj_ab.txt): water 12 k atoms s = 1.5e-5 kcal/mol/A
for each of the three samples, on against off 1.5e-5; rigid OPC with the Ewald table s = 5.7e-6 .. 7.6e-6, on against off 5.7e-6 .. 7.6e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "unilj_child.py")


def run_child(args, **knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_")}
    env.update(knobs)
    p = subprocess.run([sys.executable, CHILD] + [str(a) for a in args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "UNILJ-OK" in p.stdout, tail
    print(tail)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def bits_arms(tmp_path, which):
    out = {}
    for tag, knobs in (("off", dict(MDX_UNI_LJ="0")), ("on", {})):
        path = str(tmp_path / f"{which}_{tag}.npz")
        run_child(["bits", which, path], **knobs)
        out[tag] = np.load(path)
    return out["on"], out["off"]


def test_same_bits_water_box_full_list_across_a_rebuild(tmp_path):
    """water_box(16), 12,288 atoms, nb_variant 2, 20 steps with a list rebuild inside: positions, velocities and forces of the default arm
    are the bits of MDX_UNI_LJ=0, and the default arm ran the constant-sigma^2 body where the other did not."""
    on, off = bits_arms(tmp_path, "water")
    assert list(on["body"][:4]) == [1, 1, 1, 1] and on["body"][4] != 0, on["body"]       # eligible at create and at the end, step loop, last launch
    assert list(off["body"]) == [0, 0, 0, 0, 0], off["body"]
    for k in ("pos", "vel", "force"):
        assert same_bits(on[k], off[k]), (k, float(np.abs(on[k] - off[k]).max()))
    assert np.isfinite(on["force"]).all() and float(np.abs(on["force"]).max()) > 1.0


def test_refused_system_keeps_the_general_body_bit_for_bit(tmp_path):
    """small_solvated() has several LJ types: not eligible, and ten steps under nb_variant 2 are the bits of MDX_UNI_LJ=0."""
    on, off = bits_arms(tmp_path, "solvated")
    assert list(on["body"]) == [0, 0, 0, 0, 0] and list(off["body"]) == [0, 0, 0, 0, 0], (on["body"], off["body"])
    for k in ("pos", "vel", "force"):
        assert same_bits(on[k], off[k]), k


@pytest.mark.parametrize("which", ["water", "opc"])
def test_timed_bodies_on_against_off_within_the_spread_of_two_off_runs(tmp_path, which):
    """water: water_box(16), default variant, MDX_WPT=1 - the one-wave class and the merged dual-list body the bench line times; opc:
    opc_water_box(12), 6,912 sites, Ewald real space from the force table (coulomb_mode 2).  Forces of a plain force call, of a pruning
    pass and of an inner-list walk at fixed positions; the children assert through mdx_pair_launch_info / mdx_pair_body_info which
    instantiation and which body went out."""
    f = {}
    for tag, knobs in (("off1", dict(MDX_UNI_LJ="0")), ("off2", dict(MDX_UNI_LJ="0")), ("on", {})):
        path = str(tmp_path / f"{which}_{tag}.npz")
        run_child(["timed", which, path], MDX_WPT="1", MDX_REBUILD_INNER="0", **knobs)
        f[tag] = np.load(path)
    for kind in ("plain", "prune", "walk"):
        a, b, on = (f[t][kind].astype(np.float64) for t in ("off1", "off2", "on"))
        assert np.isfinite(on).all() and float(np.abs(on).max()) > 1.0
        s = float(np.abs(a - b).max())
        d = float(np.abs(on - a).max())
        print(f"{which} {kind}: s = max|dF| of two MDX_UNI_LJ=0 runs {s:.3e}, on against off {d:.3e} kcal/mol/A (bound 4 s = {4 * s:.3e})")
        assert d <= 4.0 * s, (which, kind, d, s)


def test_refusals_and_acceptances():
    """Several LJ types, a second oxygen type one ulp away on one molecule, the geometric rule, an alchemical window: not eligible, the
    general body; hydrogens with a sigma and no well: eligible; the window switched off again: eligible again."""
    run_child(["refusals"])
