"""Cases of `mdx_refine_guests_flex` / `MdState.refine_guests_flex`, shared by tests/test_guest_flex_host.py (CPU) and
tests/test_gpu_guest_flex.py (GPU): the small complex's ligand as a flexible guest with the start poses of
tests/test_pose_flex_host.py, and the mixed library of tests/guest_cases.py with a `GuestFlex` per ligand and a 4-atom chain added.
Pure numpy host code."""
import functools

import numpy as np

from molchanica_amd import GuestFlex, GuestLigand, systems
from tests import guest_cases as gc
from tests import pose_flex_ref as F
from tests.test_pose_flex_host import ligand_case, start_poses

t = gc.pose_batch_module()
SUBSET = [20, 3, 11, 29, 7, 0, 16, 25]      # the 8 torsions of tests/test_gpu_pose_flex.py, out of order
CHAIN_SEED, CHAIN_POSES = 31, 16      # (lig50(31, 4) is the unbranched chain 0-1-2-3: one torsion, one dihedral term)


def terms_of(flex):
    """The dihedral terms of a GuestFlex as tests/pose_flex_ref.py takes them"""
    return (np.asarray(flex.dihedral_idx, np.int64).reshape(-1, 4), np.asarray(flex.dihedral_v, np.float32).astype(np.float64),
            np.asarray(flex.dihedral_phase, np.float32).astype(np.float64), np.asarray(flex.dihedral_n).astype(np.float64))


def sides_of(flex, count):
    return F.moving_sides(count, flex.bonds, flex.root, flex.torsion_bonds)


def box_of(s):
    return (np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)) if s.periodic else None


@functools.lru_cache(maxsize=None)
def small_flex_case():
    """-> (S, R, groups of R, (lo, hi), the ligand as a guest with the 16 start poses, torsion bonds [31, 2]).  The geometry is that of
    tests/test_pose_flex_host.py: R is S without the ligand, atom for atom, so R plus a pose of the guest IS S with that pose."""
    from oracle import oracle as orc
    orc.lib()
    S, R, gR, (lo, hi), lig = gc.small_case()
    s, lo2, hi2, bonds, tb, tors, terms = ligand_case()
    assert (lo2, hi2) == (lo, hi)
    poses = start_poses(S, orc.wrap(S, S.pos), lo, hi, tors)
    return S, R, gR, (lo, hi), lig.with_poses(poses), tb


def small_flex(n_tors):
    """The GuestFlex of the small complex's ligand with 0, 8 (SUBSET) or all 31 torsions"""
    S, R, gR, (lo, hi), lig, tb = small_flex_case()
    pick = {0: tb[:0], 8: tb[SUBSET], 31: tb}[n_tors]
    return GuestFlex.from_system(S, lo, hi, 0, pick)


@functools.lru_cache(maxsize=None)
def mixed_flex_case():
    """-> (env, groups, ligands, flex).  The mixed library of guest_cases.mixed_case() - ion, 2 atoms, an empty ligand, 7, 8, 9, 50, 64
    (its poses straddle pose 256 of the library), 65 and 256 atoms - with GuestFlex.from_system per ligand, and behind them a 4-atom
    chain (one torsion: the smallest ligand that has one) placed where the 7-atom ligand's poses carved the water away."""
    env, groups, gs, ligs = gc.mixed_case()
    flex = [GuestFlex.from_system(g, 0, g.n_atoms) for g in gs]
    chain = systems.lig50(CHAIN_SEED, 4)
    centre = ligs[3].poses.reshape(-1, 3).astype(np.float64).mean(0)
    start = np.asarray(chain.pos, np.float64) - np.asarray(chain.pos, np.float64).mean(0) + centre
    poses = t.rigid_poses(start, CHAIN_POSES, CHAIN_SEED, max_tr=0.5)
    ligs = list(ligs) + [GuestLigand.from_system(chain, 0, 4, poses=poses)]
    flex.append(GuestFlex.from_system(chain, 0, 4))
    return env, groups, ligs, flex
