"""What `mdx_pose_forces` is compared against, shared by tests/test_pose_forces_host.py (no GPU) and tests/test_gpu_pose_forces.py.

Reference: the fp64 oracle's forces on a copy of the system without bond, angle and dihedral terms (exclusions and 1-4 pairs kept) at
the pose's full coordinate set.  The host test pins that this is minus the gradient of the sum of the oracle's ligand row.

Per-atom tolerance: |dF_i| <= 1e-4 max(|F_i|, 1) + slack_i, slack = orc.cutoff_slack(rel=1e-5) - the bound of the parity tests.
Rigid tolerance, derived from it: |dF_net| <= sum_i tol_i, |d tau| <= sum_i |x_i - c| tol_i.
Two caps keep a comparison meaningful: at most MAX_DROPPED of 16 poses clash (< 1.0 A to the environment, `usable`), and at most
MAX_SLACK_ROWS of the compared ligand-atom rows carry non-zero slack.  The seeds and amplitudes below were chosen on the CPU for that."""
import dataclasses

import numpy as np

from tests.test_gpu_pose_batch import MAX_DROPPED, SEED_FLEX, SEED_SMALL, min_env_distance, rigid_poses, three_groups, whole  # noqa: F401

MAX_SLACK_ROWS = 0.02
# small rigid moves of the chain (molecule 0 of small_complex, 120 atoms in water at liquid density) and of one water
SEED_CHAIN, CHAIN_ROT, CHAIN_TR = 1, 0.02, 0.3
SEED_WATER, WATER_ROT, WATER_TR = 1, 0.3, 0.4


def nonbonded_only(s):
    """A copy of the system whose bonded terms are gone; exclusions and 1-4 pairs stay."""
    z = np.zeros
    return dataclasses.replace(s, bond_idx=z((0, 2), np.uint32), bond_k=z(0, np.float32), bond_r0=z(0, np.float32),
                               angle_idx=z((0, 3), np.uint32), angle_k=z(0, np.float32), angle_theta0=z(0, np.float32),
                               dihedral_idx=z((0, 4), np.uint32), dihedral_v=z(0, np.float32), dihedral_phase=z(0, np.float32),
                               dihedral_n=z(0, np.int32))


def four_groups(s):
    """receptor / ligand / solvent, and the first water as a group of its own (3)"""
    g = three_groups(s)
    g[int(s.mol_start[2]):int(s.mol_start[3])] = 3
    return g


def full_set(pos, lo, hi, pose):
    x = np.asarray(pos, np.float64).copy()
    x[lo:hi] = np.asarray(pose, np.float64)
    return x


def rigid_of(pose, f):
    """(net force, torque about the unweighted mean of the pose's coordinates), fp64"""
    x = np.asarray(pose, np.float64)
    f = np.asarray(f, np.float64)
    return np.concatenate([f.sum(0), np.cross(x - x.mean(0), f).sum(0)])


def reference(orc, s, cfg, pos, lo, hi, pose, use_cells=True):
    """-> (oracle forces on the range [count, 3], per-atom tolerance [count], slack [count])"""
    x = full_set(pos, lo, hi, pose)
    fo = orc.forces(nonbonded_only(s), cfg, pos=x, use_cells=use_cells)[0][lo:hi]
    slack = orc.cutoff_slack(s, cfg, pos=x.astype(np.float32), rel=1e-5)[lo:hi]
    return fo, 1e-4 * np.maximum(np.linalg.norm(fo, axis=1), 1.0) + slack, slack


def rigid_tolerance(pose, tol):
    x = np.asarray(pose, np.float64)
    return tol.sum(), (np.linalg.norm(x - x.mean(0), axis=1) * tol).sum()


def chain_poses(start, n=16):
    return rigid_poses(start, n, SEED_CHAIN, max_rot=CHAIN_ROT, max_tr=CHAIN_TR)


def water_poses(start, n=16):
    return rigid_poses(start, n, SEED_WATER, max_rot=WATER_ROT, max_tr=WATER_TR)


def caps(orc, s, cfg, pos, lo, hi, poses):
    """-> (poses dropped for a clash, rows with slack, rows compared, closest approach to the 1.0 A rule)"""
    d = min_env_distance(s, pos, lo, hi, poses)
    keep = d >= 1.0
    rows = slacked = 0
    for k in np.flatnonzero(keep):
        sl = orc.cutoff_slack(s, cfg, pos=full_set(pos, lo, hi, poses[k]).astype(np.float32), rel=1e-5)[lo:hi]
        rows += sl.size
        slacked += int((sl > 0).sum())
    return int((~keep).sum()), slacked, rows, float(np.abs(d - 1.0).min())
