"""Systems for the fused bonded + kick + drift pass (mdx_integrate.hip: bonded_integrate_kernel) beyond pure TIP3P water, and a plain
host mirror of the two tables that feed it.  Shared by tests/test_fused_cases_host.py (CPU) and tests/fused_cases_child.py (GPU).

mixed_solvent      water_box(16) with 32 waters turned into monatomic ions (atom 0, a middle atom and the last atom among them: no roles,
                   shape code 0), 8 static waters, per-water bond and angle parameters (one shape per atom: codes far above 255), the
                   terms of a water written in three orders (both arms of each second-bond selector) and an H-H bond on every fourth
                   water, before or behind the O-H bonds (hydrogens with two bonds, in both orders)
one_bond_too_many  ... plus one bond from a hydrogen to the next water's oxygen: not a triad handle any more, and two role lists longer
                   than the three records the pass fetches up front (the record flavours' tail loop)
chain_in_water     small_solvated(n_chain=120, box=49.65): dihedrals, 1-4 pairs, lists of up to 20 roles - the general flavour

role_tables        mdx_create's caller-order role lists (mdx_api.hip, add_term): per atom the angles before the bonds, each kind in term
                   order; record = (partners in term order without the atom itself, kind | role << 4 | set << 8); parameter sets numbered
                   by first appearance of the (kind, bit pattern) while dihedrals, angles, bonds and 1-4 pairs are walked in that order
triad_shapes       mdx_triad_build's (mdx_hostutil.cpp) eligibility, per-atom codes (in order of first appearance, atom by atom), shape
                   words and 8-byte records"""
import copy
import math

import numpy as np

from molchanica_amd import systems, topology
from molchanica_amd._abi import ATOM_GHOST, ATOM_STATIC, MdConfig

KIND_BOND, KIND_ANGLE, KIND_DIHEDRAL, KIND_PAIR14 = 0, 1, 2, 3      # ROLE_* of mdx_internal.h
FUSED_PRE = 3                  # records the record flavours fetch up front (mdx_integrate.hip)
ROLES_PER_SLOT_MAX = 2.6       # mdx_bonded_integrate_ok
N_IONS, N_STATIC_WATERS = 32, 8
ION_TYPES = ((2.44, 0.087, 22.99, 1.0), (3.1, 0.1, 35.45, -1.0))       # sigma A, eps kcal/mol, mass, charge


def _distinct_f32(rng, n, centre, rel):
    """n uniform draws from centre (1 +- rel) whose f32 values are pairwise distinct"""
    x = rng.uniform(centre * (1.0 - rel), centre * (1.0 + rel), n).astype(np.float32)
    while True:
        _, first = np.unique(x, return_index=True)
        dup = np.setdiff1d(np.arange(n), first)
        if dup.size == 0:
            return x
        x[dup] = rng.uniform(centre * (1.0 - rel), centre * (1.0 + rel), dup.size).astype(np.float32)


def mixed_solvent(n_side=16, seed=41, angle_k_rel=0.2):
    """-> MdSystem with .case_info: ions / static_waters / waters (molecule numbers of water_box), first_atom (molecule -> its first
    atom here, -1 for none), hh (molecules with an H-H bond), bond_of (molecule -> indices into bond_idx of its (O,H1), (O,H2) bonds)"""
    base = systems.water_box(n_side, seed)
    t = systems.TIP3P
    W = n_side ** 3
    rng = np.random.default_rng(seed + 1000)
    fixed_ions = [0, W // 2, W - 1]
    rest = np.setdiff1d(np.arange(W), fixed_ions)
    pick = rng.choice(rest, N_IONS - len(fixed_ions) + N_STATIC_WATERS, replace=False)
    ions = np.sort(np.concatenate([fixed_ions, pick[:N_IONS - len(fixed_ions)]]))
    static = np.sort(pick[N_IONS - len(fixed_ions):])
    is_ion = np.zeros(W, bool); is_ion[ions] = True
    is_static = np.zeros(W, bool); is_static[static] = True
    waters = np.flatnonzero(~is_ion)
    nw = waters.size
    bk = _distinct_f32(rng, 2 * nw, 450.0, 0.2).reshape(nw, 2)
    br = _distinct_f32(rng, 2 * nw, 0.9572, 0.04).reshape(nw, 2)
    ak = _distinct_f32(rng, nw, t["k_theta"], angle_k_rel)
    at = _distinct_f32(rng, nw, t["theta"], 0.03)
    hh_k = _distinct_f32(rng, nw, 40.0, 0.2)
    hh_r = _distinct_f32(rng, nw, 1.5139, 0.02)

    pos0, vel0 = np.asarray(base.pos, np.float64), np.asarray(base.vel, np.float64)
    pos, vel, mass, charge, ljt, flags, mol_start = [], [], [], [], [], [], []
    first_atom = np.full(W, -1, np.int64)
    bonds, bond_k, bond_r0, front, front_k, front_r0, back, back_k, back_r0 = ([] for _ in range(9))
    angles, angle_k, angle_t0, excl, hh = [], [], [], [], []
    bond_of = {}
    n, n_ion, iw = 0, 0, 0
    for w in range(W):
        mol_start.append(n)
        first_atom[w] = n
        if is_ion[w]:
            sig, eps, m, q = ION_TYPES[n_ion % 2]
            pos.append(pos0[3 * w]); vel.append(0.5 * vel0[3 * w]); mass.append(m); charge.append(q); ljt.append(2 + n_ion % 2); flags.append(0)
            n_ion += 1
            n += 1
            continue
        o, h1, h2 = n, n + 1, n + 2
        for a in range(3):
            pos.append(pos0[3 * w + a]); mass.append(base.mass[3 * w + a]); charge.append(base.charge[3 * w + a]); ljt.append(base.lj_type[3 * w + a])
            vel.append(np.zeros(3) if is_static[w] else vel0[3 * w + a]); flags.append(ATOM_STATIC if is_static[w] else 0)
        order = w % 3
        k1, k2, r1, r2 = bk[iw, 0], bk[iw, 1], br[iw, 0], br[iw, 1]       # (O,H1) and (O,H2)
        bond_of[w] = (len(bonds) + (1 if order == 1 else 0), len(bonds) + (0 if order == 1 else 1))      # (indices before the H-H bonds in front are counted)
        if order == 0:
            bonds += [(o, h1), (o, h2)]; bond_k += [k1, k2]; bond_r0 += [r1, r2]; angles.append((h1, o, h2))
        elif order == 1:
            bonds += [(o, h2), (o, h1)]; bond_k += [k2, k1]; bond_r0 += [r2, r1]; angles.append((h1, o, h2))
        else:
            bonds += [(h1, o), (o, h2)]; bond_k += [k1, k2]; bond_r0 += [r1, r2]; angles.append((h2, o, h1))
        angle_k.append(ak[iw]); angle_t0.append(at[iw])
        if w % 4 == 0:
            hh.append(w)
            if w % 8 == 0:
                front.append((h1, h2)); front_k.append(hh_k[iw]); front_r0.append(hh_r[iw])
            else:
                back.append((h1, h2)); back_k.append(hh_k[iw]); back_r0.append(hh_r[iw])
        excl += [(o, h1), (o, h2), (h1, h2)]
        iw += 1
        n += 3
    nf = len(front)
    off, idx = topology.csr_from_pairs(n, np.asarray(excl))
    box = np.asarray(base.box_hi, np.float64)
    s = systems.MdSystem(
        pos=np.asarray(pos), mass=np.asarray(mass, np.float32), charge=np.asarray(charge), lj_type=np.asarray(ljt),
        lj_sigma=[t["o_sigma"], 0.0, ION_TYPES[0][0], ION_TYPES[1][0]], lj_eps=[t["o_eps"], 0.0, ION_TYPES[0][1], ION_TYPES[1][1]],
        vel=np.asarray(vel), flags=np.asarray(flags, np.uint8),
        bond_idx=np.asarray(front + bonds + back), bond_k=np.asarray(front_k + bond_k + back_k, np.float32),
        bond_r0=np.asarray(front_r0 + bond_r0 + back_r0, np.float32),
        angle_idx=np.asarray(angles), angle_k=np.asarray(angle_k, np.float32), angle_theta0=np.asarray(angle_t0, np.float32),
        excl_offsets=off, excl_idx=idx, mol_start=np.asarray(mol_start),
        periodic=True, box_lo=(0, 0, 0), box_hi=tuple(box), name=f"mixed{n}",
    ).normalise()
    s.case_info = dict(ions=ions, static_waters=static, waters=waters, first_atom=first_atom, hh=np.asarray(hh),
                       bond_of={w: (a + nf, b + nf) for w, (a, b) in bond_of.items()}, angle_of={int(w): i for i, w in enumerate(waters)})
    return s


def one_bond_too_many(system):
    """`system` (a mixed_solvent) plus one bond from H1 of a water that has an H-H bond to the oxygen of the next molecule, at the
    length it has now: that hydrogen (angle, O-H, H-H, the new bond) and that oxygen (angle, two O-H, the new bond) carry four records
    -> (MdSystem, the two atoms)"""
    ci = system.case_info
    plain = np.zeros(ci["first_atom"].size + 1, bool)
    plain[ci["waters"]] = True
    plain[ci["static_waters"]] = False
    w = next(int(w) for w in ci["hh"] if w > ci["first_atom"].size // 2 and plain[w] and plain[w + 1])
    h1, o2 = int(ci["first_atom"][w]) + 1, int(ci["first_atom"][w + 1])
    box = np.asarray(system.box_hi, np.float64) - np.asarray(system.box_lo, np.float64)
    d = np.asarray(system.pos[h1], np.float64) - np.asarray(system.pos[o2], np.float64)
    d -= np.rint(d / box) * box
    s = copy.copy(system)
    s.bond_idx = np.concatenate([system.bond_idx, np.asarray([[h1, o2]], np.uint32)])
    s.bond_k = np.concatenate([system.bond_k, np.asarray([60.0], np.float32)])
    s.bond_r0 = np.concatenate([system.bond_r0, np.asarray([np.linalg.norm(d)], np.float32)])
    s.name = system.name + "+1"
    return s.normalise(), (h1, o2)


CHAIN_N = 120      # the chain length at which the handle still takes the fused pass (roles < 2.6 per slot, padding slots included)


def chain_in_water():
    return systems.small_solvated(n_chain=CHAIN_N, box=49.65)


# ---- the host mirror ------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def role_tables(system, cfg=None):
    """-> off [N + 1] u32, rec [R, 4] u32 (p0, p1, p2, meta), prm [P, 3] f32: what mdx_create uploads as role_off_o / role_rec_o /
    role_prm for a handle without PME.  (1-4 parameter values follow mdx_api.hip in f32; no test pins them, only their count.)"""
    cfg = cfg or MdConfig()
    n = system.n_atoms
    lists = [[] for _ in range(n)]
    prm, prm_index = [], {}

    def add_term(atoms, kind, p0, p1, p2):
        key = (kind, _bits(p0), _bits(p1), _bits(p2))
        pi = prm_index.get(key)
        if pi is None:
            pi = prm_index[key] = len(prm)
            prm.append((np.float32(p0), np.float32(p1), np.float32(p2)))
        for r, at in enumerate(atoms):
            p = [int(x) for k, x in enumerate(atoms) if k != r] + [0, 0, 0]
            lists[int(at)].append((p[0], p[1], p[2], kind | (r << 4) | (pi << 8)))

    for k in range(system.dihedral_idx.shape[0]):
        add_term(system.dihedral_idx[k], KIND_DIHEDRAL, system.dihedral_v[k], system.dihedral_phase[k], np.float32(system.dihedral_n[k]))
    for k in range(system.angle_idx.shape[0]):
        add_term(system.angle_idx[k], KIND_ANGLE, system.angle_k[k], system.angle_theta0[k], 0.0)
    for k in range(system.bond_idx.shape[0]):
        add_term(system.bond_idx[k], KIND_BOND, system.bond_k[k], system.bond_r0[k], 0.0)
    if system.pairs14_idx.shape[0]:
        sg, ep, q = system.lj_sigma[system.lj_type], system.lj_eps[system.lj_type], system.charge
        f = np.float32
        for a, b in system.pairs14_idx:
            sig = f(np.sqrt(sg[a] * sg[b])) if cfg.combining_rule else f(0.5) * (sg[a] + sg[b])
            add_term((a, b), KIND_PAIR14, sig, f(4.0) * f(cfg.scale14_lj) * f(np.sqrt(ep[a] * ep[b])),
                     f(cfg.scale14_coulomb) * f(cfg.coulomb_k) * q[a] * q[b])
    # the library places a term's records as it walks the terms, kind by kind: per atom that is the order of the appends above
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in lists])
    rec = np.asarray([r for x in lists for r in x], np.uint32).reshape(-1, 4)
    return off, rec, np.asarray(prm, np.float32).reshape(-1, 3)


def triad_shapes(system, tables=None, shape_cap=65536):
    """-> dict(eligible, n_shapes, codes [N], shapes [n_shapes + 1, 4] u32, tri [N, 2] u32) as mdx_triad_build gives them (not eligible:
    n_shapes 0, the arrays None).  A handle is a triad handle when this is eligible with n_shapes > 0 (mdx_refresh_triads)."""
    off, rec, _ = tables or role_tables(system)
    n = system.n_atoms
    no = dict(eligible=False, n_shapes=0, codes=None, shapes=None, tri=None)
    code_of, shapes = {}, [(0, 0, 0, 0)]
    codes, tri = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32)
    for i in range(n):
        b0, ln = int(off[i]), int(off[i + 1]) - int(off[i])
        if ln == 0:
            continue
        if ln < 2 or ln > 3:
            return no
        an = [int(x) for x in rec[b0]]
        if (an[3] & 0xF) != KIND_ANGLE or ((an[3] >> 4) & 0xF) > 2 or an[2] != 0 or an[0] >= 1 << 24 or an[1] >= 1 << 24:
            return no
        a, b = an[0], an[1]
        sh = [an[3], 0, 0, ln - 1]
        for k in range(1, ln):
            bd = [int(x) for x in rec[b0 + k]]
            if (bd[3] & 0xF) != KIND_BOND or bd[1] or bd[2] or bd[0] not in (a, b):
                return no
            sh[k] = bd[3]
            if bd[0] != a:
                sh[3] |= 1 << (7 + k)
        sh = tuple(sh)
        code = code_of.get(sh)
        if code is None:
            if len(shapes) >= shape_cap:
                return no
            code = code_of[sh] = len(shapes)
            shapes.append(sh)
        codes[i] = code
        tri[i] = (a | ((code & 0xFF) << 24), b | ((code >> 8) << 24))
    return dict(eligible=True, n_shapes=len(shapes) - 1, codes=codes, shapes=np.asarray(shapes, np.uint32), tri=tri)


def shape_combinations(tri):
    """(angle role, bonds, first selector, second selector) of every atom with roles -> set"""
    sh = tri["shapes"][tri["codes"][tri["codes"] > 0]].astype(np.int64)
    return set(zip(((sh[:, 0] >> 4) & 0xF).tolist(), (sh[:, 3] & 3).tolist(), ((sh[:, 3] >> 8) & 1).tolist(), ((sh[:, 3] >> 9) & 1).tolist()))


ALL_COMBINATIONS = {(0, 1, 0, 0), (2, 1, 1, 0), (1, 2, 1, 0), (1, 2, 0, 1), (0, 2, 0, 1), (0, 2, 1, 0), (2, 2, 0, 1), (2, 2, 1, 0)}


def mobile(system):
    f = system.flags if system.flags is not None else np.zeros(system.n_atoms, np.uint8)
    return (np.asarray(f) & (ATOM_STATIC | ATOM_GHOST)) == 0


# ---- the bound ------------------------------------------------------------------------------------------------------------------------
def bound(system, n):
    """The project's rounding rule for an f32 trajectory against the fp64 oracle (tests/test_gpu_restraints.py, _oscillators): 4 ulp of
    the largest coordinate per step."""
    return 4.0 * float(np.spacing(np.float32(max(np.abs(np.asarray(system.pos)).max(), 1.0)))) * n


def omega(system):
    """stiffest bond on the lightest mobile atom, 1/ps: a velocity error is omega times a position error"""
    m = np.asarray(system.mass, np.float64)[mobile(system)]
    return math.sqrt(2.0 * float(np.asarray(system.bond_k).max()) * 418.4 / float(m.min()))


def min_image(d, system):
    box = np.asarray(system.box_hi, np.float64) - np.asarray(system.box_lo, np.float64)
    d = np.asarray(d, np.float64)
    return d - np.rint(d / box) * box
