"""The fused bonded + kick + drift pass (mdx_integrate.hip: bonded_integrate_kernel) on systems that reach what a box of one-parameter
water never does (tests/fused_cases.py; their properties and the window's resolving power: tests/test_fused_cases_host.py): shape codes
above 255, both arms of both bond selectors, hydrogens with two bonds, role-free and static atoms inside the fused class, one parameter
set per term, lists longer than the three records fetched up front, dihedrals and 1-4 pairs.  MDX_WPT8_BELOW and MDX_WPT are read once
per process, so each case runs in a child (tests/fused_cases_child.py); the flavour knobs are read per launch, per chunk or at create, so
all arms of a case run in that one child.

bits         nb_variant 2 (deterministic), mixed_solvent: positions, velocities and forces after bursts of (1, 16, 5, 48) steps are
             bit-identical with MDX_FUSED_TRIAD=0 and without; equal rebuild counts (>= 2) and fused launches (> 0); static atoms keep the
             bits they came with; a restraint on atom 1 makes the handle ineligible, clearing it eligible again with the same shape
             count, and the handle then follows one that never had a restraint bit for bit
window_full  nb_variant 2: the pass without the dual list's path lengths
window_half  the default half-list kernel with MDX_WPT=1, the arrangement bench.py times: the DUAL flavours
             Both: reaction field, skin 2.0, dt 0.0005.  Each arm, on a fresh handle, takes n steps from the system's state and must sit
             within bound(n) = 4 ulp_f32(largest |coordinate|) n of the fp64 oracle in every coordinate of every atom (minimum image); takes
             40 more steps (>= 1 rebuild); is read back; takes n more steps and must sit within bound(n) of the oracle started from the
             read-back state - the records role_fill_body wrote for the re-sorted slots.  Velocities: within omega bound(n), omega =
             sqrt(2 k_max 418.4 / m_min).  bound is the project's rounding rule (tests/test_gpu_restraints.py), not a measurement of the
             pass: the arm with MDX_FUSE_BONDED_INTEGRATE=0 (the separate bonded gather and kick + drift launches every small-system
             test exercises) is its control on these systems.

Arms (flavour = the template arguments <DUAL, PIPE, NODIH, POSRE, TRIAD> mdx_launch_bonded_integrate chooses), measured on an MI355X -
rebuilds, fused launches, max |dx| of the two windows in bounds; bound(4) = 6.10e-5 A, bound(8) = 1.22e-4 A:

bits         13,056 slots in 203 tiles; 6 rebuilds and 63 fused launches in both arms; 0 atoms differ; last_launch 1 / 0
window_full (without a dual list the launcher has one record flavour, the general one: MDX_FUSED_NODIH changes nothing there)
  arm                                flavour                            rebuilds  fused launches  |dx| window 1, window 2 (bounds)
  mixed triad                        <0,0,1,0,1>                        4         41              6.92e-6 A 0.113   6.90e-6 A 0.113
  mixed record                       <0,0,0,0,0>                        4         41              6.92e-6   0.113   6.90e-6   0.113
  mixed record, NODIH off            <0,0,0,0,0>                        4         41              6.92e-6   0.113   6.90e-6   0.113
  mixed separate launches (control)  bonded gather, kick + drift        4          0              6.92e-6   0.113   6.89e-6   0.113
  one bond too many, fused           <0,0,0,0,0>, tail loop             4         41              6.92e-6   0.113   6.89e-6   0.113
  one bond too many (control)        bonded gather, kick + drift        4          0              6.92e-6   0.113   6.88e-6   0.113
  chain in water, fused (n = 8)      <0,0,0,0,0>, tail loop, dihedrals  3         50              1.39e-5   0.114   1.27e-5   0.104
  chain in water (control)           bonded gather, kick + drift        3          0              1.39e-5   0.114   1.28e-5   0.105
window_half
  mixed triad                        <1,0,1,0,1>                        4         41              6.92e-6   0.113   6.89e-6   0.113
  mixed record                       <1,0,1,0,0>                        4         41              6.92e-6   0.113   6.89e-6   0.113
  mixed record, NODIH off            <1,0,0,0,0>                        4         41              6.92e-6   0.113   6.89e-6   0.113
  mixed separate launches (control)  bonded gather, kick + drift        4          0              6.92e-6   0.113   6.89e-6   0.113
  mixed triad, path split off        <1,0,1,0,1>, ref rows              4         41              6.92e-6   0.113   6.89e-6   0.113
  one bond too many, fused           <1,0,1,0,0>, tail loop             4         41              6.92e-6   0.113   6.83e-6   0.112
  one bond too many (control)        bonded gather, kick + drift        4          0              6.92e-6   0.113   6.84e-6   0.112
  chain in water, fused (n = 8)      <1,0,0,0,0>, tail loop, dihedrals  4         49              1.39e-5   0.114   1.27e-5   0.104
  chain in water (control)           bonded gather, kick + drift        3          0              1.39e-5   0.114   1.19e-5   0.097
Two of each arm's rebuilds fall between its windows.  Velocities: 0.076 .. 0.102 of omega bound(n) in every arm.  The control keeps the
rule on these systems (0.10-0.11 of the bound), so the bound stands as stated.  A 2 % parameter exchange moves an atom by 15 bounds or more
(tests/test_fused_cases_host.py): a wrong shape code, selector or parameter row in one water turns `bits` and that flavour's window red."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(case, wpt=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_")}
    env["MDX_WPT8_BELOW"] = "32"
    if wpt is not None:
        env["MDX_WPT"] = str(wpt)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_cases_child.py"), case], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-40:])
    print(tail)
    assert p.returncode == 0 and "FUSED-CASES-OK" in p.stdout, tail


def test_triad_flavour_gives_the_record_flavours_bits_with_twelve_thousand_shapes():
    _child("bits")


def test_every_flavour_follows_the_oracle_over_a_short_window_full_list():
    _child("window_full")


def test_every_flavour_follows_the_oracle_over_a_short_window_half_list():
    _child("window_half", wpt=1)
