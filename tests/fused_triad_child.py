"""Child of tests/test_gpu_fused_triad.py: MDX_WPT8_BELOW (and MDX_WPT) are read once per process, so each case runs in one of its own.

usage: MDX_WPT8_BELOW=32 [MDX_WPT=1] python tests/fused_triad_child.py bits | half | restraints
water_box(16): 12,288 atoms, 206 tiles - with MDX_WPT8_BELOW=32 in the class whose step loop runs the fused bonded + kick + drift pass.
S is no multiple of the pass's 256-thread block, the tiles carry padding slots, a water's partners sit in other tiles, and from the
first rebuild on waters straddle the periodic faces.  MDX_FUSED_TRIAD is read per launch: both arms run in this process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402

DT = 0.0005
BURSTS = (1, 16, 5, 48)       # as tests/test_gpu_fused_step.py: rebuilds, pruning passes and chunk boundaries fall inside the 70 steps


def run(system, cfg, triad):
    """-> positions, velocities, forces, stats, the triad query after the last burst"""
    if triad:
        os.environ.pop("MDX_FUSED_TRIAD", None)
    else:
        os.environ["MDX_FUSED_TRIAD"] = "0"
    try:
        with md_state.MdState(system, cfg) as md:
            md.profile(1)       # (the per-kernel brackets count the fused launches: mdx_stats.fused_launches)
            assert md.fused_triad_info() == {"eligible": True, "shapes": 3, "last_launch": False}, md.fused_triad_info()
            for n in BURSTS:
                md.step(DT, None, n)
            return md.positions(), md.velocities(), md.forces(), md.stats(), md.fused_triad_info()
    finally:
        os.environ.pop("MDX_FUSED_TRIAD", None)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev(a, b, box):
    d = a.astype(np.float64) - b
    d -= np.rint(d / box) * box
    return np.abs(d).max(), np.sqrt((d ** 2).sum(1).mean())


def case_bits(water):
    """The deterministic full-list pair kernel (nb_variant 2): the triad flavour against the record flavour, bit for bit."""
    cfg = MdConfig(nb_variant=2)
    pt, vt, ft, st, it = run(water, cfg, True)
    pr, vr, fr, sr, ir = run(water, cfg, False)
    assert st["n_tiles"] == 206 and st["n_slots"] % 256 != 0 and st["n_slots"] > st["n_atoms"], st
    print("rebuilds", st["rebuild_count"], sr["rebuild_count"], "fused launches", st["fused_launches"], sr["fused_launches"], "query", it, ir)
    assert st["rebuild_count"] >= 2 and st["rebuild_count"] == sr["rebuild_count"]
    assert st["fused_launches"] > 0 and sr["fused_launches"] == st["fused_launches"]
    assert it == {"eligible": True, "shapes": 3, "last_launch": True}, it
    assert ir == {"eligible": True, "shapes": 3, "last_launch": False}, ir
    assert np.isfinite(pt).all() and np.isfinite(vt).all() and np.isfinite(ft).all()
    box = np.asarray(water.box_hi, np.float64) - np.asarray(water.box_lo, np.float64)
    print("positions max, rms", dev(pt, pr, box), "velocities max", np.abs(vt - vr).max(), "forces max", np.abs(ft - fr).max())
    assert same_bits(pt, pr), "positions differ"
    assert same_bits(vt, vr), "velocities differ"
    assert same_bits(ft, fr), "forces differ"


def case_half(water):
    """The default half-list kernel with one wave per tile (f32 atomics: the last bits vary run to run) - the arrangement bench.py times:
    the triad run sits as close to a record run as two record runs sit to each other.
    Reaction field (coulomb_mode 1), as in tests/test_gpu_fused_step.py: the force is continuous at the cutoff.  Under the shifted-potential
    default a pair that crosses the cutoff a step earlier in one run kicks a hydrogen by ~1 kcal/mol/A for a step, and on 12,288 atoms ONE
    such atom (2.4e-3 A) is the whole rms (2e-5): over 6 record and 4 triad runs the distances were 4.5e-6 .. 4.7e-5 A in both classes alike,
    and `rms12 < 4 rms23 + 1e-5` failed for 15 of 225 pairings of record runs with THEMSELVES (36 of 360 with a triad run) - a coin, not a
    check.  With the continuous force the same runs sit 1.2e-6 .. 2.3e-6 A apart, record-record and triad-record alike (0 of 360 fail), so
    the bound is 1.5e-5 .. 1.9e-5 A in absolute terms: tighter than anything it could resolve under the default."""
    assert os.environ.get("MDX_WPT") == "1"
    cfg = MdConfig(coulomb_mode=1)
    box = np.asarray(water.box_hi, np.float64) - np.asarray(water.box_lo, np.float64)
    p1, _, _, s1, i1 = run(water, cfg, True)
    p2, _, _, s2, i2 = run(water, cfg, False)
    p3, _, _, s3, i3 = run(water, cfg, False)
    assert s1["fused_launches"] > 0 and s1["rebuild_count"] >= 2 and s1["rebuild_count"] == s2["rebuild_count"] == s3["rebuild_count"]
    assert i1["last_launch"] and not i2["last_launch"] and not i3["last_launch"], (i1, i2, i3)
    mx12, rms12 = dev(p1, p2, box)
    mx23, rms23 = dev(p2, p3, box)
    print("rms12", rms12, "rms23", rms23, "max12", mx12, "max23", mx23)
    assert rms12 < 4.0 * rms23 + 1e-5, (rms12, rms23, mx12, mx23)


def case_restraints(water):
    """Eligibility follows the handle.  Two handles take the same 6 steps; one then gets a restraint on an oxygen (ineligible) and has it
    cleared again (eligible) before both take 20 more - the same bits, through the triad flavour; a handle that steps while restrained
    runs the record flavour of restrained handles.  (The restrained steps come last: they move the atoms, and the comparison needs two
    handles in the same state.)"""
    cfg = MdConfig(nb_variant=2)
    assert abs(float(water.mass[0]) - 15.999) < 0.1      # atom 0 is an oxygen
    with md_state.MdState(water, cfg) as a, md_state.MdState(water, cfg) as b:
        for md in (a, b):
            md.profile(1)
            md.step(DT, None, 6)
            assert md.fused_triad_info() == {"eligible": True, "shapes": 3, "last_launch": True}, md.fused_triad_info()
        a.set_position_restraints([0], k=5.0)
        assert a.fused_triad_info() == {"eligible": False, "shapes": 0, "last_launch": False}, a.fused_triad_info()
        a.clear_position_restraints()
        assert a.fused_triad_info() == {"eligible": True, "shapes": 3, "last_launch": False}, a.fused_triad_info()
        for md in (a, b):
            md.step(DT, None, 20)
            assert md.fused_triad_info()["last_launch"]
        assert same_bits(a.positions(), b.positions()) and same_bits(a.velocities(), b.velocities()) and same_bits(a.forces(), b.forces())
        n0 = a.stats()["fused_launches"]
        a.set_position_restraints([0], k=5.0)
        a.step(DT, None, 20)
        info, st = a.fused_triad_info(), a.stats()
        assert info == {"eligible": False, "shapes": 0, "last_launch": False}, info
        assert st["fused_launches"] > n0, "the restrained handle left the fused pass"
        assert a.step_count == 46 and np.isfinite(a.positions()).all() and np.isfinite(a.velocities()).all()
    with md_state.MdState(systems.small_solvated(), MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)) as md:      # a chain in water: dihedrals, 1-4 pairs
        assert md.fused_triad_info() == {"eligible": False, "shapes": 0, "last_launch": False}, md.fused_triad_info()


def main():
    assert os.environ.get("MDX_WPT8_BELOW") == "32"
    assert md_state.device_count() >= 1
    water = systems.water_box(16, seed=41)
    assert water.n_atoms == 12288
    {"bits": case_bits, "half": case_half, "restraints": case_restraints}[sys.argv[1]](water)
    print("FUSED-TRIAD-OK")


if __name__ == "__main__":
    main()
