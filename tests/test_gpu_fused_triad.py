"""The triad flavour of the fused bonded + kick + drift pass (mdx_integrate.hip: bonded_integrate_kernel<..., TRIAD>; handles whose
every role list is empty or one angle plus one or two bonds to its partners - mdx_triad_build, tests/test_triad_detect.py) against the
record flavour it replaces, on the smallest box that takes the pass: water_box(16) with MDX_WPT8_BELOW=32, as
tests/timed_body_child.py does.  The knob is read once per process, so each case runs in a child (tests/fused_triad_child.py).

bits        nb_variant 2 (deterministic): positions, velocities and forces after bursts of (1, 16, 5, 48) steps are bit-identical with
            MDX_FUSED_TRIAD=0 and without; equal rebuild counts (>= 2), fused launches > 0, mdx_fused_triad_info names each arm's flavour
half        the default half-list kernel, MDX_WPT=1, reaction field: rms(triad, record) < 4 rms(record, record) + 1e-5  (under the shifted
            cutoff two record runs of this 12 k-atom box fail that bound against each other in 7 % of the pairings: the child's docstring)
restraints  a position restraint makes the handle ineligible, clearing it eligible again, and the handle then follows one that never
            had a restraint bit for bit; a chain in water is not eligible"""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_triad_child.py"), case], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    print(tail)
    assert p.returncode == 0 and "FUSED-TRIAD-OK" in p.stdout, tail


def test_triad_flavour_gives_the_record_flavours_bits():
    _child("bits")


def test_triad_flavour_within_the_run_to_run_distance_of_the_half_list_kernel():
    _child("half", wpt=1)


def test_eligibility_follows_the_restraints_of_the_handle():
    _child("restraints")
