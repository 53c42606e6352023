"""Cases of `mdx_screen_ligands` / `MdState.screen_ligands`, shared by tests/test_guest_screen_host.py (CPU) and
tests/test_gpu_guest_screen.py (GPU): systems with whole molecules removed, water carved away around a set of points, systems put
together from parts (the oracle's combined system: environment + guest as one more molecule), and the mixed library of the boundary
test.  Pure numpy / scipy host code."""
import functools
import importlib.util
import os

import numpy as np

from molchanica_amd import GuestLigand, MdSystem, systems
from molchanica_amd import topology as topo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def pose_batch_module():
    """tests/test_gpu_pose_batch.py as a module (rigid_poses, whole, usable, oracle_row, assert_row, small_configs, ...): reused, not copied."""
    spec = importlib.util.spec_from_file_location("pose_batch_gpu_tests", os.path.join(ROOT, "tests", "test_gpu_pose_batch.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


def _csr_pairs(s):
    off = s.excl_offsets.astype(np.int64)
    ii = np.repeat(np.arange(s.n_atoms, dtype=np.int64), np.diff(off))
    jj = s.excl_idx.astype(np.int64)
    m = ii < jj
    return np.stack([ii[m], jj[m]], 1)


def _mol_of_atom(s):
    ms = np.asarray(s.mol_start, np.int64)
    return np.searchsorted(ms, np.arange(s.n_atoms), side="right") - 1


def without_molecules(s: MdSystem, drop) -> MdSystem:
    """`s` without the molecules (indices into mol_start) of `drop`: every per-atom array cut, every index array - bonds, angles,
    dihedrals, the exclusion CSR, 1-4 pairs, mol_start, constraints, virtual sites - remapped.  A term that names a dropped atom must
    name only dropped atoms (whole molecules leave)."""
    s.normalise()
    n = s.n_atoms
    mol = _mol_of_atom(s)
    keep_mol = np.ones(len(s.mol_start), bool)
    keep_mol[np.asarray(list(drop), np.int64)] = False
    keep = keep_mol[mol]
    new = np.full(n, -1, np.int64)
    new[keep] = np.arange(int(keep.sum()))

    def terms(idx, *params):
        idx = np.asarray(idx, np.int64).reshape(-1, idx.shape[1])
        k = keep[idx]
        assert (k.all(1) | (~k).all(1)).all(), "a term links a kept molecule to a dropped one"
        sel = k.all(1)
        return (new[idx[sel]].astype(np.uint32),) + tuple(np.asarray(p)[sel] for p in params)

    bond_idx, bond_k, bond_r0 = terms(s.bond_idx, s.bond_k, s.bond_r0)
    angle_idx, angle_k, angle_t0 = terms(s.angle_idx, s.angle_k, s.angle_theta0)
    dih_idx, dih_v, dih_p, dih_n = terms(s.dihedral_idx, s.dihedral_v, s.dihedral_phase, s.dihedral_n)
    (p14,) = terms(s.pairs14_idx)
    cons_idx, cons_len = terms(s.constraint_idx, s.constraint_len)
    vs_idx, vs_w = terms(s.vsite_idx, s.vsite_w)
    (ex,) = terms(_csr_pairs(s))
    off, idx = topo.csr_from_pairs(int(keep.sum()), ex)
    ms = np.asarray(s.mol_start, np.int64)
    return MdSystem(
        pos=s.pos[keep], mass=s.mass[keep], charge=s.charge[keep], lj_type=s.lj_type[keep], lj_sigma=s.lj_sigma.copy(), lj_eps=s.lj_eps.copy(),
        vel=None if s.vel is None else s.vel[keep], flags=None if s.flags is None else s.flags[keep],
        bond_idx=bond_idx, bond_k=bond_k, bond_r0=bond_r0, angle_idx=angle_idx, angle_k=angle_k, angle_theta0=angle_t0,
        dihedral_idx=dih_idx, dihedral_v=dih_v, dihedral_phase=dih_p, dihedral_n=dih_n, excl_offsets=off, excl_idx=idx, pairs14_idx=p14,
        mol_start=new[ms[keep_mol]].astype(np.uint32), constraint_idx=cons_idx, constraint_len=cons_len, vsite_idx=vs_idx, vsite_w=vs_w,
        periodic=s.periodic, box_lo=s.box_lo, box_hi=s.box_hi, name=s.name + "-cut").normalise()


def only_molecules(s: MdSystem, keep) -> MdSystem:
    keep = set(int(k) for k in keep)
    return without_molecules(s, [m for m in range(len(s.mol_start)) if m not in keep])


def is_water(s: MdSystem) -> np.ndarray:
    """Per molecule: three atoms, the first with a well and a negative charge, the others without a well (flexible TIP3P as `systems` makes it)."""
    s.normalise()
    ms = np.append(np.asarray(s.mol_start, np.int64), s.n_atoms)
    size = np.diff(ms)
    eps = s.lj_eps[s.lj_type]
    out = size == 3
    first = ms[:-1]
    ok = np.flatnonzero(out)
    out[ok] = (eps[first[ok]] > 0) & (s.charge[first[ok]] < 0) & (eps[first[ok] + 1] == 0) & (eps[first[ok] + 2] == 0)
    return out


def carved_molecules(s: MdSystem, points, r: float) -> np.ndarray:
    """The water molecules of `s` with an atom within r of any of `points` (minimum image on a periodic system)."""
    from scipy.spatial import cKDTree
    s.normalise()
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    pos = np.asarray(s.pos, np.float64)
    if s.periodic:
        lo = np.asarray(s.box_lo, np.float64)
        box = np.asarray(s.box_hi, np.float64) - lo
        wrap = lambda x: np.mod(np.mod(x - lo, box), box)      # (twice: a tiny negative remainder rounds to `box` itself)
        tree, q = cKDTree(wrap(pts), boxsize=box), wrap(pos)
    else:
        tree, q = cKDTree(pts), pos
    d, _ = tree.query(q, k=1)
    mol = _mol_of_atom(s)
    hit = np.zeros(len(s.mol_start), bool)
    hit[mol[d < r]] = True
    return np.flatnonzero(hit & is_water(s))


def carve(s: MdSystem, points, r: float) -> MdSystem:
    """`s` without every water molecule that has an atom within r of any of `points`."""
    return without_molecules(s, carved_molecules(s, points, r))


def concat_systems(parts, like: MdSystem) -> MdSystem:
    """The systems of `parts` one behind the other as one system in the cell of `like`: LJ tables and all index arrays shifted."""
    parts = [p.normalise() for p in parts]
    a0 = np.cumsum([0] + [p.n_atoms for p in parts])
    t0 = np.cumsum([0] + [int(p.lj_sigma.size) for p in parts])

    def cat(f, shift=None):
        if shift is None:
            return np.concatenate([np.asarray(getattr(p, f)) for p in parts])
        return np.concatenate([np.asarray(getattr(p, f)).astype(np.int64) + shift[k] for k, p in enumerate(parts)])

    ex = np.concatenate([_csr_pairs(p) + a0[k] for k, p in enumerate(parts)])
    off, idx = topo.csr_from_pairs(int(a0[-1]), ex)
    vel = None if any(p.vel is None for p in parts) else cat("vel")
    flags = None if all(p.flags is None for p in parts) else np.concatenate(
        [np.zeros(p.n_atoms, np.uint8) if p.flags is None else p.flags for p in parts])
    mol_start = np.concatenate([(np.asarray(p.mol_start, np.int64) if p.mol_start is not None else np.zeros(1, np.int64)) + a0[k]
                                for k, p in enumerate(parts)])
    return MdSystem(
        pos=cat("pos"), mass=cat("mass"), charge=cat("charge"), lj_type=cat("lj_type", t0), lj_sigma=cat("lj_sigma"), lj_eps=cat("lj_eps"),
        vel=vel, flags=flags, bond_idx=cat("bond_idx", a0), bond_k=cat("bond_k"), bond_r0=cat("bond_r0"),
        angle_idx=cat("angle_idx", a0), angle_k=cat("angle_k"), angle_theta0=cat("angle_theta0"),
        dihedral_idx=cat("dihedral_idx", a0), dihedral_v=cat("dihedral_v"), dihedral_phase=cat("dihedral_phase"), dihedral_n=cat("dihedral_n"),
        excl_offsets=off, excl_idx=idx, pairs14_idx=cat("pairs14_idx", a0), mol_start=mol_start.astype(np.uint32),
        constraint_idx=cat("constraint_idx", a0), constraint_len=cat("constraint_len"), vsite_idx=cat("vsite_idx", a0), vsite_w=cat("vsite_w"),
        periodic=like.periodic, box_lo=like.box_lo, box_hi=like.box_hi, name=like.name + "+guest").normalise()


def combined(env: MdSystem, env_groups, guest_sys: MdSystem, front=False):
    """The oracle's system for a guest row: `env` with the guest appended as one more molecule (front: put first instead) and one more
    group.  -> (system, group of every atom, n_groups, (lo, hi) of the guest, index of the environment's atoms)."""
    g = np.asarray(env_groups, np.uint8)
    G = int(g.max()) + 1
    ne, ng = env.n_atoms, guest_sys.n_atoms
    if front:
        s = concat_systems([guest_sys, env], env)
        return s, np.concatenate([np.full(ng, G, np.uint8), g]), G + 1, (0, ng), np.arange(ng, ng + ne)
    s = concat_systems([env, guest_sys], env)
    return s, np.concatenate([g, np.full(ng, G, np.uint8)]), G + 1, (ne, ne + ng), np.arange(ne)


def guest_oracle_row(orc, env, env_groups, env_pos, guest_sys, pose, cfg, use_cells=True, front=False):
    """Row [M[L][0..G-1], M[L][L]] and its gross sums of the guest at `pose` beside the environment at `env_pos`: `orc.between_mols`
    on the combined system."""
    s, g, n, (lo, hi), env_at = combined(env, env_groups, guest_sys, front)
    x = np.empty((s.n_atoms, 3), np.float64)
    x[env_at] = np.asarray(env_pos, np.float64)
    x[lo:hi] = np.asarray(pose, np.float64)
    mo, gr = orc.between_mols(s, cfg, g, n, pos=x, use_cells=use_cells)
    L = n - 1
    return mo[L], gr[L]


def min_distance(env: MdSystem, env_pos, poses) -> np.ndarray:
    """Closest guest - environment distance of every pose (minimum image), fp64 on the CPU."""
    t = pose_batch_module()
    s = env
    return t.min_env_distance(s, np.asarray(env_pos, np.float64), len(env_pos), len(env_pos), poses)


# ---- the small complex: receptor + solvent resident, the ligand a guest ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case():
    """S = small_complex(), R = S without its ligand (molecule 1), the ligand as a guest, groups of R: receptor 0, solvent 1."""
    t = pose_batch_module()
    S = systems.small_complex()
    lo, hi = t.ligand_range(S)
    R = without_molecules(S, [1])
    gR = np.ones(R.n_atoms, np.uint8)
    gR[:int(R.mol_start[1])] = 0
    return S, R, gR, (lo, hi), GuestLigand.from_system(S, lo, hi)


def s_positions(pos_r, lo, pose):
    """Coordinates of S from those of R and the ligand's pose (the ligand sits at [lo, lo + count) of S)."""
    pos_r = np.asarray(pos_r)
    return np.concatenate([pos_r[:lo], np.asarray(pose, pos_r.dtype), pos_r[lo:]])


# ---- the mixed library: every boundary of the kernel in one call -------------------------------------------------------------------------------
MIXED_SIZES = (2, 7, 8, 9, 50, 64, 65, 256)
MIXED_SEED = 31
CARVE_R, CLEARANCE = 2.5, 1.5
# poses per ligand, library order: ion, lig2, an EMPTY copy of lig7, lig7, lig8, lig9, lig50, lig64, lig65, lig256.  Cumulative:
# 24 48 48 88 128 168 216 266 290 302 - the 64-atom ligand's poses 216 .. 265 straddle the chunk boundary at pose 256.
MIXED_POSES = (24, 24, 0, 40, 40, 40, 48, 50, 24, 12)


def ion_system() -> MdSystem:
    """One sodium-like atom: a guest with no pair at all."""
    return MdSystem(pos=np.zeros((1, 3)), mass=[22.99], charge=[1.0], lj_type=[0], lj_sigma=[2.44], lj_eps=[0.0874], mol_start=[0],
                    name="ion").normalise()


@functools.lru_cache(maxsize=None)
def mixed_case():
    """-> (env, env_groups, guest systems, GuestLigands with their poses).  The environment is water_box(n_side=10) carved at CARVE_R
    around every atom of every pose; its waters are in two groups alternating by molecule, so that the group key changes inside a
    wave's walk.  The 256-atom guest sits at the box centre, the others about points 10 A from it along the cube's diagonals."""
    t = pose_batch_module()
    box = systems.water_box(n_side=10)
    L = float(box.box_hi[0])
    gs = [ion_system(), systems.lig50(MIXED_SEED, 2), systems.lig50(MIXED_SEED + 1, 7)]
    gs += [systems.lig50(MIXED_SEED + 1 + k, n) for k, n in enumerate(MIXED_SIZES[1:])]
    assert len(gs) == len(MIXED_POSES)
    corners = [np.array([sx, sy, sz], np.float64) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    ligs, k = [], 0
    for m, (g, n) in enumerate(zip(gs, MIXED_POSES)):
        c = np.full(3, L / 2)
        if g.n_atoms != 256 and n:
            c = c + 10.0 * corners[k]
            k += 1
        start = np.asarray(g.pos, np.float64) - np.asarray(g.pos, np.float64).mean(0) + c
        poses = t.rigid_poses(start, n, MIXED_SEED + 100 + m) if n else None
        ligs.append(GuestLigand.from_system(g, 0, g.n_atoms, poses=poses))
    pts = np.concatenate([l.poses.reshape(-1, 3) for l in ligs if l.poses is not None])
    env = carve(box, pts, CARVE_R)
    groups = (np.arange(env.n_atoms) // 3 % 2).astype(np.uint8)
    return env, groups, gs, ligs
