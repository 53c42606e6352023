"""Child of tests/test_gpu_fused_cases.py: MDX_WPT8_BELOW (and MDX_WPT) are read once per process, so each case runs in one of its own.

usage: MDX_WPT8_BELOW=32 [MDX_WPT=1] python tests/fused_cases_child.py bits | window_full | window_half
The systems are those of tests/fused_cases.py (12 k atoms, ~205 tiles: with MDX_WPT8_BELOW=32 in the class whose step loop runs the fused
bonded + kick + drift pass).  The knobs that choose the pass's flavour are read per launch (MDX_FUSED_TRIAD, MDX_FUSED_NODIH), per chunk
(MDX_FUSE_BONDED_INTEGRATE) or at create (MDX_PATH_SPLIT): every arm of a case runs in this process, each on a handle of its own.

window_*: a handle steps n times from the system's own state and is compared with the fp64 oracle, atom by atom; it steps 40 more times
(the list is rebuilt, the slots are sorted anew, role_fill_body writes the records again), its state is read back, and the next n steps
are compared with the oracle started from that read-back state.  Every arm is printed before the first assertion is made."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig  # noqa: E402
from molchanica_amd import md_state  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import fused_cases as K  # noqa: E402

DT = 0.0005
BURSTS = (1, 16, 5, 48)       # as tests/fused_triad_child.py
BETWEEN = 40                   # steps between the two windows
KNOBS = ("MDX_FUSED_TRIAD", "MDX_FUSED_NODIH", "MDX_FUSE_BONDED_INTEGRATE", "MDX_PATH_SPLIT")

TRIAD = {}
RECORD = {"MDX_FUSED_TRIAD": "0"}
RECORD_DIH = {"MDX_FUSED_TRIAD": "0", "MDX_FUSED_NODIH": "0"}
SEPARATE = {"MDX_FUSE_BONDED_INTEGRATE": "0"}
TRIAD_NO_SPLIT = {"MDX_PATH_SPLIT": "0"}


@contextlib.contextmanager
def knobs(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
def run_bursts(system, cfg, env, shapes):
    with knobs(env), md_state.MdState(system, cfg) as md:
        md.profile(1)       # (the per-kernel brackets count the fused launches: mdx_stats.fused_launches)
        assert md.fused_triad_info() == {"eligible": True, "shapes": shapes, "last_launch": False}, md.fused_triad_info()
        for n in BURSTS:
            md.step(DT, None, n)
        return md.positions(), md.velocities(), md.forces(), md.stats(), md.fused_triad_info()


def case_bits():
    """The deterministic full-list pair kernel (nb_variant 2): the triad flavour against the record flavour, bit for bit, on a system
    with 12 k shapes; then eligibility through a restraint and back."""
    s = K.mixed_solvent()
    shapes = K.triad_shapes(s)["n_shapes"]
    cfg = MdConfig(nb_variant=2)
    pt, vt, ft, st, it = run_bursts(s, cfg, TRIAD, shapes)
    pr, vr, fr, sr, ir = run_bursts(s, cfg, RECORD, shapes)
    print("slots", st["n_slots"], "tiles", st["n_tiles"], "rebuilds", st["rebuild_count"], sr["rebuild_count"], "fused launches", st["fused_launches"],
          sr["fused_launches"], "query", it, ir)
    d = np.abs(K.min_image(pt.astype(np.float64) - pr, s))
    print("positions max", d.max(), "atoms that differ", int((d.max(1) > 0).sum()), "velocities max", np.abs(vt - vr).max(), "forces max", np.abs(ft - fr).max())
    assert st["n_slots"] > st["n_atoms"], st      # (padding slots: "no roles" records of role_fill_body; 13,056 slots here, 51 whole blocks)
    assert st["rebuild_count"] >= 2 and st["rebuild_count"] == sr["rebuild_count"]
    assert st["fused_launches"] > 0 and sr["fused_launches"] == st["fused_launches"]
    assert it == {"eligible": True, "shapes": shapes, "last_launch": True}, it
    assert ir == {"eligible": True, "shapes": shapes, "last_launch": False}, ir
    assert np.isfinite(pt).all() and np.isfinite(vt).all() and np.isfinite(ft).all()
    assert same_bits(pt, pr), "positions differ"
    assert same_bits(vt, vr), "velocities differ"
    assert same_bits(ft, fr), "forces differ"
    fixed = ~K.mobile(s)
    assert fixed.sum() == 24 and same_bits(pt[fixed], np.asarray(s.pos, np.float32)[fixed]), "a static atom moved"
    assert (vt[fixed] == 0).all()
    # the restraints of the handle (tests/fused_triad_child.py, case_restraints) on this system: atom 1 is the first water's oxygen
    assert abs(float(s.mass[1]) - 15.999) < 0.1
    with knobs(TRIAD), md_state.MdState(s, cfg) as a, md_state.MdState(s, cfg) as b:
        for md in (a, b):
            md.profile(1)
            md.step(DT, None, 6)
            assert md.fused_triad_info() == {"eligible": True, "shapes": shapes, "last_launch": True}, md.fused_triad_info()
        a.set_position_restraints([1], k=5.0)
        assert a.fused_triad_info() == {"eligible": False, "shapes": 0, "last_launch": False}, a.fused_triad_info()
        a.clear_position_restraints()
        assert a.fused_triad_info() == {"eligible": True, "shapes": shapes, "last_launch": False}, a.fused_triad_info()
        for md in (a, b):
            md.step(DT, None, 20)
            assert md.fused_triad_info()["last_launch"]
        assert same_bits(a.positions(), b.positions()) and same_bits(a.velocities(), b.velocities()) and same_bits(a.forces(), b.forces())
    print("restraints: eligible -> not -> eligible, then bit-identical over 20 steps")


# ---- window ---------------------------------------------------------------------------------------------------------------------------
class Arms:
    def __init__(self):
        self.failed = []
        self.first = {}      # (system name, n) -> the oracle's first window: computed once, shared by the arms, never written

    def oracle_first(self, system, cfg, n):
        key = (system.name, n)
        if key not in self.first:
            x, v, _ = oracle.step(system, cfg, DT, n, use_cells=True)
            x.setflags(write=False); v.setflags(write=False)
            self.first[key] = (x, v)
        return self.first[key]

    def check(self, ok, what):
        if not ok:
            self.failed.append(what)

    def run(self, label, system, cfg, n, env, fused, info_before, info_after):
        dual = cfg.nb_variant == 0      # the default half list walks a dual list: the pass's DUAL flavours
        bound, om = K.bound(system, n), K.omega(system)
        move = K.mobile(system)
        with knobs(env), md_state.MdState(system, cfg) as md:
            md.profile(1)
            self.check(md.fused_triad_info() == info_before, f"{label}: query at create {md.fused_triad_info()}")
            md.step(DT, None, n)
            x1, v1 = md.positions().astype(np.float64), md.velocities().astype(np.float64)
            r1 = md.stats()["rebuild_count"]
            md.step(DT, None, BETWEEN)
            xb, vb = md.positions(), md.velocities()
            r2 = md.stats()["rebuild_count"]
            md.step(DT, None, n)
            x2, v2 = md.positions().astype(np.float64), md.velocities().astype(np.float64)
            st, info = md.stats(), md.fused_triad_info()
        xr1, vr1 = self.oracle_first(system, cfg, n)
        xr2, vr2, _ = oracle.step(system, cfg, DT, n, pos=xb.astype(np.float64), vel=vb.astype(np.float64), use_cells=True)
        dx1, dx2 = np.abs(K.min_image(x1 - xr1, system)), np.abs(K.min_image(x2 - xr2, system))
        dv1, dv2 = np.abs(v1 - vr1)[move].max(), np.abs(v2 - vr2)[move].max()
        print(f"ARM {label:34s} rebuilds {st['rebuild_count']} ({r2 - r1} between the windows)  fused launches {st['fused_launches']:3d}  last_launch {int(info['last_launch'])}  "
              f"dx {dx1.max():.2e} {dx2.max():.2e} A = {dx1.max() / bound:.3f} {dx2.max() / bound:.3f} bound({n})  "
              f"dv {dv1:.2e} {dv2:.2e} A/ps = {dv1 / (om * bound):.3f} {dv2 / (om * bound):.3f} omega bound", flush=True)
        self.check(np.isfinite(x2).all() and np.isfinite(v2).all(), f"{label}: not finite")
        self.check(r2 - r1 >= 1, f"{label}: no rebuild between the windows")
        self.check((st["fused_launches"] > 0) if fused else (st["fused_launches"] == 0), f"{label}: fused launches {st['fused_launches']}")
        self.check(info == info_after, f"{label}: query {info}")
        self.check((st["prune_passes"] > 0 or st["n_inner_cluster_pairs"] > 0) == dual,
                   f"{label}: dual list, {st['prune_passes']} pruning passes, {st['n_inner_cluster_pairs']} inner cluster pairs")
        self.check(dx1.max() <= bound, f"{label}: first window {dx1.max():.3e} A > {bound:.3e} (atom {int(dx1.max(1).argmax())})")
        self.check(dx2.max() <= bound, f"{label}: second window {dx2.max():.3e} A > {bound:.3e} (atom {int(dx2.max(1).argmax())})")
        self.check(dv1 <= om * bound and dv2 <= om * bound, f"{label}: velocities {dv1:.3e} {dv2:.3e} A/ps > {om * bound:.3e}")
        self.check(same_bits(xb[~move], np.asarray(system.pos, np.float32)[~move]), f"{label}: a static atom moved")


def case_window(half):
    """half: the default half-list pair kernel with one wave per tile (the arrangement bench.py times; DUAL flavours of the pass);
    else nb_variant 2 (the pass's flavours without the dual list's path lengths)."""
    assert (os.environ.get("MDX_WPT") == "1") == half
    cfg = MdConfig(coulomb_mode=1, skin=2.0) if half else MdConfig(coulomb_mode=1, skin=2.0, nb_variant=2)
    arms = Arms()
    s = K.mixed_solvent()
    shapes = K.triad_shapes(s)["n_shapes"]

    def q(last):
        return {"eligible": True, "shapes": shapes, "last_launch": last}
    no = {"eligible": False, "shapes": 0, "last_launch": False}
    arms.run("mixed triad", s, cfg, 4, TRIAD, True, q(False), q(True))
    arms.run("mixed record", s, cfg, 4, RECORD, True, q(False), q(False))
    arms.run("mixed record, NODIH off", s, cfg, 4, RECORD_DIH, True, q(False), q(False))
    arms.run("mixed separate launches (control)", s, cfg, 4, SEPARATE, False, q(False), q(False))
    if half:
        arms.run("mixed triad, path split off", s, cfg, 4, TRIAD_NO_SPLIT, True, q(False), q(True))
    s2, _ = K.one_bond_too_many(s)
    arms.run("one bond too many, fused", s2, cfg, 4, TRIAD, True, no, no)
    arms.run("one bond too many (control)", s2, cfg, 4, SEPARATE, False, no, no)
    c = K.chain_in_water()
    arms.run("chain in water, fused", c, cfg, 8, TRIAD, True, no, no)
    arms.run("chain in water (control)", c, cfg, 8, SEPARATE, False, no, no)
    assert not arms.failed, "\n".join(arms.failed)


def main():
    assert os.environ.get("MDX_WPT8_BELOW") == "32"
    assert md_state.device_count() >= 1
    {"bits": case_bits, "window_full": lambda: case_window(False), "window_half": lambda: case_window(True)}[sys.argv[1]]()
    print("FUSED-CASES-OK")


if __name__ == "__main__":
    main()
