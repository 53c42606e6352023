"""`mdx_guest_forces` / `mdx_refine_guests`: forces, net force and torque of a library of guest ligands - described by the caller, never
entered into the handle - and their rigid-body refinement on the device.

Forces against the fp64 oracle on the COMBINED system (the environment with the guest appended as one more molecule and group:
`guest_cases.combined`, `pose_force_ref.reference`) under the bound of tests/test_gpu_pose_forces.py: per atom |dF_i| <= 1e-4 max(|F_i|, 1)
+ slack_i, net force and torque by the sums derived from it; at most 2 of 16 poses dropped for a clash, at most 2 % of the compared
rows with slack (tests/test_guest_refine_host.py holds both on the CPU).

GPU against GPU (the twin: a handle that holds the ligand as a resident, `pose_forces`): the twin bound of the rows, |dM| <= 2e-6 |M| +
1e-6 G with G the gross sum over the same pairs, carried over to a force: |dF_i| <= 2e-6 |F_i| + 1e-6 G_i, G_i = the sum over the
environment atoms within the cutoff of the magnitudes of the pair forces on ligand atom i (`gross_pair_force`, numpy fp64 - plain
Lennard-Jones and plain Coulomb magnitudes, which bound every treatment's from above).  Both handles evaluate the same fp32 pair forces
with the same pair_eval; a resident ligand changes the clusters and with them the order of the sums: eight pair forces are added in fp32
(3 roundings of 2^-24 of their gross each side), the rest in fp64, and each side rounds its sum to fp32 once (2^-24 |F_i|).  The
ligand's own pairs are walked in the same order by both and cancel bit for bit.

The refinement against the host loop of tests/pose_refine_ref.py driven by `guest_forces`, by the criteria of
tests/test_gpu_pose_refine.py: status and evaluation count equal, coordinates within 4 ulp32(max |coordinate|), xform within 1e-5."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import GuestLigand, MdConfig, _abi, systems
from molchanica_amd._abi import CGuestLigand

from tests import guest_cases as gc
from tests import pose_force_ref as pfr
from tests import pose_refine_ref as P
from tests.test_gpu_guest_screen import c_ligand, separated
from tests.test_gpu_pose_forces import compare

pytestmark = pytest.mark.gpu

t = gc.pose_batch_module()
SEED_SMALL = t.SEED_SMALL


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def row_sums(rows):
    """S of the header: the columns of the fp32 row added in column order in fp64"""
    S = np.zeros(rows.shape[0], np.float64)
    for c in range(rows.shape[1]):
        S += rows[:, c].astype(np.float64)
    return S


def small_poses(orc, n=16):
    S, R, gR, (lo, hi), lig = gc.small_case()
    pos = orc.wrap(S, S.pos)
    return t.rigid_poses(t.whole(S, pos[lo:hi]), n, SEED_SMALL)


def gross_pair_force(s, cfg, env_pos, pose, q, sigma, eps, env_q, env_sigma, env_eps):
    """G_i of the module's docstring for every atom of `pose`: sum over the environment atoms within the larger cutoff (minimum image; all
    of them without a cutoff) of |f_LJ| + |f_Coulomb|, plain forms, Lorentz-Berthelot."""
    x = np.asarray(pose, np.float64)[:, None, :] - np.asarray(env_pos, np.float64)[None]
    if s.periodic:
        box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
        x -= np.round(x / box) * box
    r = np.linalg.norm(x, axis=2)
    rc = max(cfg.lj_cutoff, cfg.coulomb_cutoff)
    near = r < rc if rc > 0 else np.ones(r.shape, bool)
    sg = 0.5 * (np.asarray(sigma, np.float64)[:, None] + np.asarray(env_sigma, np.float64)[None])
    ep = np.sqrt(np.asarray(eps, np.float64)[:, None] * np.asarray(env_eps, np.float64)[None])
    s6 = (sg / r) ** 6
    f = 24.0 * ep * np.abs(2.0 * s6 * s6 - s6) / r + cfg.coulomb_k * np.abs(np.asarray(q, np.float64)[:, None] * np.asarray(env_q, np.float64)[None]) / r ** 2
    return np.where(near, f, 0.0).sum(1)


def twin_tolerance(s, cfg, env, env_pos, lig, pose, f_ref):
    G = gross_pair_force(s, cfg, env_pos, pose, lig.charge, lig.lj_sigma, lig.lj_eps, env.charge, env.lj_sigma[env.lj_type], env.lj_eps[env.lj_type])
    return 2e-6 * np.linalg.norm(np.asarray(f_ref, np.float64), axis=1) + 1e-6 * G


def assert_twin(f, rigid, f_ref, rigid_ref, pose, tol, what):
    """Per atom within tol; net force and torque within the sums derived from it (pose_force_ref.rigid_tolerance)"""
    ratio = np.linalg.norm(f.astype(np.float64) - f_ref.astype(np.float64), axis=1) / tol
    tf, tt = pfr.rigid_tolerance(pose, tol)
    rf = np.linalg.norm(rigid[:3].astype(np.float64) - rigid_ref[:3]) / tf
    rt = np.linalg.norm(rigid[3:].astype(np.float64) - rigid_ref[3:]) / tt
    print(f"{what}: worst |dF_i| {ratio.max():.3f}x the twin bound, net force {rf:.3f}x, torque {rt:.3f}x")
    assert ratio.max() <= 1.0 and rf <= 1.0 and rt <= 1.0, what
    return float(ratio.max())


# ---- forces ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_forces(mdx, orc):
    """The guest's forces on the small complex's 16 poses, per config (forces, rows, rigid, screen rows, positions of R, poses)"""
    S, R, gR, (lo, hi), lig = gc.small_case()
    poses = small_poses(orc)
    out = []
    for cfg in t.small_configs():
        with mdx.MdState(R, cfg) as md:
            assert md.set_energy_groups(gR, 2) == 2
            pos = md.positions()
            lib_ = [lig.with_poses(poses)]
            (f,), (rows,), (rigid,) = md.guest_forces(lib_, rows=True, rigid=True)
            (screen,) = md.screen_ligands(lib_)
            out.append((f, rows, rigid, screen, pos, poses))
    return out


def test_forces_match_the_oracle_on_the_combined_system(mdx, orc, small_forces):
    S, R, gR, (lo, hi), lig = gc.small_case()
    comb, g, n, (clo, chi), env_at = gc.combined(R, gR, gc.only_molecules(S, [1]))
    for cfg, (f, rows, rigid, screen, pos, poses) in zip(t.small_configs(), small_forces):
        assert f.shape == (16, hi - lo, 3) and f.dtype == np.float32 and rigid.shape == (16, 6) and rows.shape == (16, 3)
        keep = t.usable(S, gc.s_positions(pos, lo, poses[0]), lo, hi, poses)
        pos_c = np.concatenate([pos, poses[0]])
        _, _, fmax = compare(orc, comb, cfg, pos_c, clo, chi, poses, keep, f, rigid, f"guest on the small complex, coulomb mode {cfg.coulomb_mode}")
        assert fmax > 1.0 and np.abs(f[keep]).max() > 1.0


def test_forces_agree_with_pose_forces_on_a_twin(mdx, orc, small_forces):
    S, R, gR, (lo, hi), lig = gc.small_case()
    g3 = t.three_groups(S)
    for cfg, (f, rows, rigid, screen, pos, poses) in zip(t.small_configs(), small_forces):
        with mdx.MdState(S, cfg) as twin:
            twin.set_energy_groups(g3, 3)
            assert np.array_equal(bits(np.delete(twin.positions(), np.s_[lo:hi], 0)), bits(pos)), "the twin's environment is R's"
            tf, trigid = twin.pose_forces(lo, poses, rows=False, rigid=True)
        keep = t.usable(S, gc.s_positions(pos, lo, poses[0]), lo, hi, poses)
        differ = 0
        for k in np.flatnonzero(keep):
            tol = twin_tolerance(R, cfg, R, pos, lig, poses[k], tf[k])
            assert_twin(f[k], rigid[k], tf[k], trigid[k].astype(np.float64), poses[k], tol, f"twin, mode {cfg.coulomb_mode}, pose {k}")
            differ += int((bits(f[k]) != bits(tf[k])).sum())
        print(f"coulomb mode {cfg.coulomb_mode}: {differ} force components not bit-equal to the resident ligand's")


def test_rows_are_the_bits_of_screen_ligands(mdx, small_forces):
    for cfg, (f, rows, rigid, screen, pos, poses) in zip(t.small_configs(), small_forces):
        assert rows.dtype == np.float32 and np.array_equal(bits(rows), bits(screen)), f"coulomb mode {cfg.coulomb_mode}: {rows - screen}"
        assert np.abs(rows).min() > 1e-3


def boundary_library():
    """The mixed library of tests/guest_cases.py with the 256-atom ligand first: 1 atom, 2 (collinear), an empty ligand, 7, 8, 9 (the strip
    of 8 and its neighbours), 50, 64, 65 (the wave and its neighbour) and 256 atoms.  Poses per ligand 12 24 24 0 40 40 40 48 50 24,
    cumulative 12 36 60 60 100 140 180 228 278 302: the first chunk holds the smallest and the largest ligand, the 64-atom ligand's
    poses 228 .. 277 straddle pose 256.  Reversed, the chunks hold other ligands."""
    env, groups, gs, ligs = gc.mixed_case()
    lib_ = [ligs[-1]] + list(ligs[:-1])
    assert [l.count for l in lib_] == [256, 1, 2, 7, 7, 8, 9, 50, 64, 65] and [l.n_poses for l in lib_] == [12, 24, 24, 0, 40, 40, 40, 48, 50, 24]
    edges = np.cumsum([l.n_poses for l in lib_])
    assert edges[7] < 256 < edges[8] and lib_[8].count == 64 and edges[1] <= 256
    return env, groups, lib_


def same(a, b, what):
    for x, y, name in zip(a, b, ("forces / poses", "rows", "rigid", "xform", "status", "evals")):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), f"{what}: {name} differ"


def test_mixed_library_at_the_boundaries_of_the_kernels(mdx):
    env, groups, lib_ = boundary_library()
    cfg = t.small_configs()[0]
    with mdx.MdState(env, cfg) as md:
        assert md.set_energy_groups(groups, 2) == 2
        full = md.guest_forces(lib_, rows=True, rigid=True)
        assert [f.shape for f in full[0]] == [(l.n_poses, l.count, 3) for l in lib_]
        assert [r.shape for r in full[1]] == [(l.n_poses, 3) for l in lib_] and [r.shape for r in full[2]] == [(l.n_poses, 6) for l in lib_]
        screen = md.screen_ligands(lib_)
        back = [v[::-1] for v in md.guest_forces(lib_[::-1], rows=True, rigid=True)]
        for m, lig in enumerate(lib_):
            mine = [v[m] for v in full]
            assert np.array_equal(bits(mine[1]), bits(screen[m])), f"ligand {m}: rows are not those of screen_ligands"
            same(mine, [v[m] for v in back], f"ligand {m} ({lig.count} atoms) in the reversed library")
            if lig.n_poses == 0:
                continue
            same(mine, [v[0] for v in md.guest_forces([lig], rows=True, rigid=True)], f"ligand {m} ({lig.count} atoms) by itself")
            for p in range(lig.n_poses):
                alone = md.guest_forces([lig.with_poses(lig.poses[p:p + 1])], rows=True, rigid=True)
                same([v[p:p + 1] for v in mine], [v[0] for v in alone], f"ligand {m} ({lig.count} atoms) pose {p} alone")
            assert np.isfinite(mine[0]).all() and np.abs(mine[0]).max() > 1e-3, "the guest must feel the water"
        # one atom: no pair of its own, no torque about itself; the net force is the atom's
        ion_f, _, ion_rigid = (v[1] for v in full)
        assert (ion_rigid[:, 3:] == 0.0).all() and np.array_equal(bits(ion_rigid[:, :3]), bits(ion_f[:, 0]))
        # the refinement through the same chunks: a few evaluations, the three orders of the library
        args = (4, 0.0, 0.0)
        ref = md.refine_guests(lib_, *args)
        rback = [v[::-1] for v in md.refine_guests(lib_[::-1], *args)]
        for m, lig in enumerate(lib_):
            mine = [v[m] for v in ref]
            same(mine, [v[m] for v in rback], f"refinement of ligand {m} ({lig.count} atoms) in the reversed library")
            if lig.n_poses:
                same(mine, [v[0] for v in md.refine_guests([lig], *args)], f"refinement of ligand {m} ({lig.count} atoms) by itself")
                assert (mine[5] >= 1).all() and (mine[5] <= 4).all() and np.isin(mine[4], (P.CONVERGED, P.MAX_EVALS, P.STALLED)).all()
                assert (row_sums(mine[1]) <= row_sums(full[1][m])).all(), f"ligand {m}: the row sum rose"


# ---- refinement --------------------------------------------------------------------------------------------------------------------------------
def two_sizes(orc, n_small=16, n_other=8):
    """The small complex's ligand with its 16 poses and a 23-atom guest in the same pocket: two sizes in one call"""
    S, R, gR, (lo, hi), lig = gc.small_case()
    poses = small_poses(orc, n_small)
    other = systems.lig50(seed=4, n_atoms=23)
    start = np.asarray(other.pos, np.float64) - np.asarray(other.pos, np.float64).mean(0) + poses[0].astype(np.float64).mean(0)
    return [lig.with_poses(poses), GuestLigand.from_system(other, 0, 23, poses=t.rigid_poses(start, n_other, SEED_SMALL + 1))]


def guest_evaluate(mdx, md, lig, width):
    """`evaluate` of the host loop the device loop replaces: one guest_forces call per evaluation (MDX_ENAN: all NaN)"""
    def evaluate(Y):
        try:
            _, (row,), (rigid,) = md.guest_forces([lig.with_poses(np.ascontiguousarray(Y[None]))], rows=True, rigid=True)
        except mdx.BlowUpError:
            return np.full(width, np.nan, np.float32), np.full(6, np.nan, np.float32)
        return row[0], rigid[0]
    return evaluate


def against_the_host_loop(mdx, md, lib_, what, max_evals, f_tol=0.0, tau_tol=0.0, h_start=0.0, h_max=0.0):
    dev = md.refine_guests(lib_, max_evals, f_tol, tau_tol, h_start, h_max)
    for m, lig in enumerate(lib_):
        mine = [v[m] for v in dev]
        host = P.refine_batch(lig.poses, guest_evaluate(mdx, md, lig, mine[1].shape[1]), max_evals, f_tol, tau_tol, h_start, h_max)
        assert np.array_equal(mine[4], host[4]), f"{what}, ligand {m}: status device {mine[4].tolist()} host {host[4].tolist()}"
        assert np.array_equal(mine[5], host[5]), f"{what}, ligand {m}: evaluations device {mine[5].tolist()} host {host[5].tolist()}"
        differ = int((bits(mine[0]) != bits(host[0])).sum())
        worst = float(np.abs(mine[0].astype(np.float64) - host[0].astype(np.float64)).max()) / ulp32(host[0])
        print(f"{what}, ligand {m} ({lig.count} atoms): status {mine[4].tolist()}, evaluations {mine[5].tolist()}; {differ} of {mine[0].size} "
              f"coordinates not bit-equal to the host loop's, worst difference {worst:.2f} ulp32(max |coordinate|)")
        assert worst <= 4.0, f"{what}, ligand {m}: a coordinate differs from the host loop's by {worst:.1f} ulp32"
        assert np.abs(mine[3] - host[3]).max() <= 1e-5, f"{what}, ligand {m}: xform {np.abs(mine[3] - host[3]).max()}"
    return dev


def self_consistent(md, lib_, dev, what):
    """rows_out / rigid_out are the bits screen_ligands / guest_forces return for poses_out (finite poses only: the calls refuse the others)"""
    for m, lig in enumerate(lib_):
        ok = dev[4][m] != P.NONFINITE
        if not ok.any():
            continue
        again = [lig.with_poses(np.ascontiguousarray(dev[0][m][ok]))]
        assert np.array_equal(bits(dev[1][m][ok]), bits(md.screen_ligands(again)[0])), f"{what}, ligand {m}: rows_out is not screen_ligands(poses_out)"
        _, (rows,), (rigid,) = md.guest_forces(again, rows=True, rigid=True)
        assert np.array_equal(bits(dev[1][m][ok]), bits(rows)), f"{what}, ligand {m}: rows_out is not the rows of guest_forces(poses_out)"
        assert np.array_equal(bits(dev[2][m][ok]), bits(rigid)), f"{what}, ligand {m}: rigid_out is not that of guest_forces(poses_out)"


def test_refinement_equals_the_host_loop(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    lib_ = two_sizes(orc)
    with mdx.MdState(R, t.small_configs()[0]) as md:
        md.set_energy_groups(gR, 2)
        dev = against_the_host_loop(mdx, md, lib_, "12 evaluations", 12)
        assert [y.shape for y in dev[0]] == [(16, lig.count, 3), (8, 23, 3)] and [r.shape for r in dev[1]] == [(16, 3), (8, 3)]
        assert [x.shape for x in dev[3]] == [(16, 7), (8, 7)] and dev[4][0].dtype == np.uint32 and dev[5][1].dtype == np.uint32
        assert (dev[5][0] == 12).all() and (dev[4][0] == P.MAX_EVALS).all()
        self_consistent(md, lib_, dev, "12 evaluations")


def test_refinement_equals_the_host_loop_through_rejects(mdx, orc):
    """h_start = h_max = 0.2 A overshoots soon, so the 48 evaluations hold rejects; with f_tol 2 kcal/mol/A and tau_tol 6 kcal/mol poses
    converge and stall at many different evaluation counts: live and frozen poses of two ligands share the chunk for most of the run."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    lib_ = two_sizes(orc)
    with mdx.MdState(R, t.small_configs()[0]) as md:
        md.set_energy_groups(gR, 2)
        dev = against_the_host_loop(mdx, md, lib_, "h_start = h_max = 0.2 A", 48, f_tol=2.0, tau_tol=6.0, h_start=0.2, h_max=0.2)
        evals, status = np.concatenate(dev[5]), np.concatenate(dev[4])
        assert (evals >= 1).all() and (evals <= 48).all() and len(set(evals.tolist())) > 4
        assert (status == P.CONVERGED).any() and (status == P.STALLED).any()
        self_consistent(md, lib_, dev, "h_start = h_max = 0.2 A")


def test_one_evaluation_returns_the_input(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    lib_ = two_sizes(orc)
    with mdx.MdState(R, t.small_configs()[0]) as md:
        md.set_energy_groups(gR, 2)
        y, rows, rigid, xform, status, evals = md.refine_guests(lib_, 1, 0.0, 0.0)
        f, frows, frigid = md.guest_forces(lib_, rows=True, rigid=True)
        for m, l in enumerate(lib_):
            assert np.array_equal(bits(y[m]), bits(l.poses)) and (evals[m] == 1).all() and (status[m] == P.MAX_EVALS).all()
            assert np.array_equal(bits(rows[m]), bits(frows[m])) and np.array_equal(bits(rigid[m]), bits(frigid[m]))
            assert np.array_equal(xform[m], np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), (l.n_poses, 1)))


def test_descent_and_rigidity(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    lib_ = two_sizes(orc)
    with mdx.MdState(R, t.small_configs()[0]) as md:
        md.set_energy_groups(gR, 2)
        y, rows, rigid, xform, status, evals = md.refine_guests(lib_, 48, 0.0, 0.0)
        start = md.screen_ligands(lib_)
        for m, l in enumerate(lib_):
            before, after = row_sums(start[m]), row_sums(rows[m])
            print(f"ligand {m}: decrease of the row sum, kcal/mol:", np.round(before - after, 3).tolist(), "evaluations", evals[m].tolist())
            assert (after <= before).all() and ((evals[m] > 1) & (after < before)).any()
            for k in range(l.n_poses):
                a, b = l.poses[k].astype(np.float64), y[m][k].astype(np.float64)
                d0 = np.linalg.norm(a[:, None] - a[None], axis=2)
                d1 = np.linalg.norm(b[:, None] - b[None], axis=2)
                tol = 4 * max(ulp32(a), ulp32(b))
                assert np.abs(d1 - d0).max() <= tol, f"ligand {m} pose {k}: a pair distance changed by {np.abs(d1 - d0).max():.2e} A (bound {tol:.2e})"
                assert abs(np.linalg.norm(xform[m][k, :4].astype(np.float64)) - 1.0) <= 1e-6


def test_best_pose_is_the_host_argmin_of_the_accepted_rows(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    poses = small_poses(orc)
    a, b = two_sizes(orc)
    with mdx.MdState(R, t.small_configs()[1]) as md:
        md.set_energy_groups(gR, 2)
        pos = md.positions()
        on_top = poses[5].copy()
        on_top[0] = pos[3]      # its first atom on an atom of the receptor: not finite at evaluation 0
        with pytest.raises(mdx.BlowUpError):
            md.guest_forces([lig.with_poses(on_top[None])])
        lib_ = [a,
                b.with_poses(None),                                                        # no poses
                lig.with_poses(np.concatenate([poses[7:8], poses[:8]])),                   # pose 7 first and again at index 8
                lig.with_poses(on_top[None]),                                              # its only pose is not finite
                lig.with_poses(np.stack([on_top, poses[2], on_top, poses[2]])),            # a finite pose behind a non-finite one, twice
                b,
                lig.with_poses(np.stack([poses[3]] * 5))]                                  # one pose five times
        *out, (bp, bs) = md.refine_guests(lib_, 10, 0.0, 0.0, best=True)
        rows, status = out[1], out[4]
        assert bp.dtype == np.uint32 and bs.dtype == np.float64 and bp.shape == bs.shape == (len(lib_),)
        for m, r in enumerate(rows):
            ok = status[m] != P.NONFINITE
            if not ok.any():
                assert bp[m] == 0xFFFFFFFF and bs[m] == np.inf, (m, bp[m], bs[m])
                continue
            S_ = np.where(ok, row_sums(np.where(np.isfinite(r), r, 0)), np.inf)
            assert bp[m] == int(np.argmin(S_)), (m, bp[m], S_)
            assert bs[m] == row_sums(r[bp[m]:bp[m] + 1])[0]
        assert rows[1].shape == (0, 3) and status[3].tolist() == [P.NONFINITE] and status[4].tolist() == [P.NONFINITE, P.MAX_EVALS] * 2
        assert np.array_equal(bits(rows[2][0]), bits(rows[2][8])) and bp[2] != 8, "the same pose twice refines to the same bits; the lower index wins"
        assert bp[4] == 1 and bp[6] == 0
        # picking the best changes nothing else, and without it nothing is picked
        plain = md.refine_guests(lib_, 10, 0.0, 0.0)
        for m in range(len(lib_)):
            same([v[m] for v in out], [v[m] for v in plain], f"ligand {m} with and without best")


# ---- both calls --------------------------------------------------------------------------------------------------------------------------------
def test_periodic_images(mdx, orc):
    """A pose translated by box vectors: the rows as tests/test_gpu_guest_screen.py holds them (the oracle's row of the untranslated pose,
    and the bits of screen_ligands); the forces against the twin's for the same translated coordinates, within the twin bound."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    cfg = t.small_configs()[0]
    box = np.asarray(R.box_hi, np.float32) - np.asarray(R.box_lo, np.float32)
    base = small_poses(orc)[0]
    shifts = [(1, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -2, 1), (2, -1, -2), (-2, 1, 2)]
    moved = np.stack([base] + [base + box * np.array(k, np.float32) for k in shifts]).astype(np.float32)
    with mdx.MdState(R, cfg) as md, mdx.MdState(S, cfg) as twin:
        md.set_energy_groups(gR, 2)
        twin.set_energy_groups(t.three_groups(S), 3)
        pos = md.positions()
        lib_ = [lig.with_poses(moved)]
        (f,), (rows,), (rigid,) = md.guest_forces(lib_, rows=True, rigid=True)
        assert np.array_equal(bits(rows), bits(md.screen_ligands(lib_)[0]))
        tf, trigid = twin.pose_forces(lo, moved, rows=False, rigid=True)
        ro, gr = gc.guest_oracle_row(orc, R, gR, pos, gc.only_molecules(S, [1]), base, cfg)
        for k in range(moved.shape[0]):
            t.assert_row(rows[k], ro, gr, f"image {k} of the pose")
            tol = twin_tolerance(R, cfg, R, pos, lig, moved[k], tf[k])
            assert_twin(f[k], rigid[k], tf[k], trigid[k].astype(np.float64), moved[k], tol, f"forces of image {k}")
        assert np.abs(f[0]).max() > 1.0
        y, rrows, *_ = md.refine_guests(lib_, 6, 0.0, 0.0)
        assert np.array_equal(bits(rrows[0]), bits(md.screen_ligands([lig.with_poses(y[0])])[0]))
        assert (row_sums(rrows[0]) <= row_sums(rows)).all()


def test_vacuum_without_cutoff_and_far_away(mdx, orc):
    """The `all` branch on a non-periodic grid; then a guest 500 A away under a cutoff: forces from its own pairs only."""
    s = systems.lig50()
    gsys = systems.lig50(seed=2)
    guest = GuestLigand.from_system(gsys, 0, gsys.n_atoms)
    g = np.zeros(s.n_atoms, np.uint8)
    comb, cg, n, (clo, chi), env_at = gc.combined(s, g, gsys)
    cfg = MdConfig(lj_cutoff=0, coulomb_cutoff=0)
    with mdx.MdState(s, cfg) as md:
        assert md.set_energy_groups(g, 1) == 1
        pos = md.positions()
        near = separated(pos, gsys.pos, 6.0)
        (f,), (rows,), (rigid,) = md.guest_forces([guest.with_poses(near[None])], rows=True, rigid=True)
        assert np.array_equal(bits(rows), bits(md.screen_ligands([guest.with_poses(near[None])])[0]))
        compare(orc, comb, cfg, np.concatenate([pos, near]), clo, chi, near[None], np.ones(1, bool), f, rigid, "lig50 beside lig50 in vacuum, no cutoff",
                use_cells=False)
        y, rrows, _, _, status, evals = md.refine_guests([guest.with_poses(near[None])], 8, 0.0, 0.0)
        assert row_sums(rrows[0])[0] <= row_sums(rows)[0] and evals[0][0] >= 1
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 1)
        pos = md.positions()
        far = (near + np.array([500.0, -300.0, 250.0], np.float32)).astype(np.float32)
        (f,), (rows,), (rigid,) = md.guest_forces([guest.with_poses(far[None])], rows=True, rigid=True)
        assert rows[0, 0] == 0.0 and abs(rows[0, 1]) > 1e-3
        pos_c = np.concatenate([pos, far])
        compare(orc, comb, cfg, pos_c, clo, chi, far[None], np.ones(1, bool), f, rigid, "far guest", use_cells=False)
        fo, tol, _ = pfr.reference(orc, comb, cfg, pos_c, clo, chi, far, use_cells=False)
        alone = np.linalg.norm(rigid[0, :3]) / tol.sum()
        print(f"far guest: |F_net| {np.linalg.norm(rigid[0, :3]):.2e} = {alone:.3f}x sum tol; oracle |F_net| {np.linalg.norm(fo.sum(0)):.1e}")
        assert alone <= 1.0 and np.abs(f[0]).max() > 1e-3
        dev = against_the_host_loop(mdx, md, [guest.with_poses(far[None])], "far guest", 12)
        assert (dev[1][0][:, 0] == 0.0).all()


def test_the_handle_is_untouched(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)      # the fixed-order pair kernel
    lib_ = two_sizes(orc)
    with mdx.MdState(R, cfg) as md, mdx.MdState(R, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(gR, 2)
            m.step(0.0005, None, 4)
        rebuilds = md.stats()["rebuild_count"]
        x0, f0, v0 = md.positions(), md.forces(), md.velocities()
        md.guest_forces(lib_, rows=True, rigid=True)
        md.refine_guests(lib_, 12, 0.0, 0.0, best=True)
        assert md.stats()["rebuild_count"] == rebuilds, "the guest calls must not rebuild the list of a ready handle"
        x1, f1, v1 = md.positions(), md.forces(), md.velocities()
        assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1)) and np.array_equal(bits(v0), bits(v1))
        twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        for what in ("positions", "velocities", "forces"):
            assert np.array_equal(bits(getattr(md, what)()), bits(getattr(twin, what)())), what
        assert md.stats()["rebuild_count"] == twin.stats()["rebuild_count"]
    # the resident-pose cache of a handle survives both calls on it
    g3 = t.three_groups(S)
    poses = small_poses(orc)
    with mdx.MdState(S, cfg) as md:
        md.set_energy_groups(g3, 3)
        before = md.score_poses(lo, poses)
        fbefore = md.pose_forces(lo, poses, rows=True, rigid=True)
        rbefore = md.refine_poses(lo, poses, 6, 0.0, 0.0)
        other = lib_[1].with_poses(lib_[1].poses + np.array([0, 0, 9.0], np.float32))
        md.guest_forces([other], rows=True, rigid=True)
        assert np.array_equal(bits(before), bits(md.score_poses(lo, poses)))
        md.refine_guests([other], 6, 0.0, 0.0, best=True)
        assert np.array_equal(bits(before), bits(md.score_poses(lo, poses)))
        same(fbefore, md.pose_forces(lo, poses, rows=True, rigid=True), "pose_forces after the guest calls")
        same(rbefore, md.refine_poses(lo, poses, 6, 0.0, 0.0), "refine_poses after the guest calls")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def refused(mdx, md, recs, n_groups, match, no_out=False, opts=(12, 0.0, 0.0, 0.0, 0.0), refine_only=False, no_opts=False):
    """Both entry points refuse, name the reason and leave ALL outputs as they were"""
    lib = mdx.load_library()
    fp, up, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    arr = (CGuestLigand * len(recs))(*recs)
    n = max(sum(r.n_poses for r in recs), 1)
    nx = max(sum(3 * r.count * r.n_poses for r in recs), 1)
    W = max(n_groups, 1) + 1
    new = lambda: [np.full(nx, -7.0, np.float32), np.full((n, W), -7.0, np.float32), np.full((n, 6), -7.0, np.float32), np.full((n, 7), -7.0, np.float32)]
    p = lambda a: a.ctypes.data_as(fp)
    u = lambda a: a.ctypes.data_as(up)
    if not refine_only:
        o = new()
        rc = lib.mdx_guest_forces(md._h, len(recs), arr, p(o[1]), n_groups, None if no_out else p(o[0]), p(o[2]))
        msg = lib.mdx_last_error().decode()
        assert rc == -1 and match in msg, (rc, msg)
        assert all((v == -7.0).all() for v in o), "a refused mdx_guest_forces must leave every output untouched"
    o = new()
    st, ev, bp, bs = np.full(n, 77, np.uint32), np.full(n, 77, np.uint32), np.full(len(recs), 77, np.uint32), np.full(len(recs), -7.0, np.float64)
    ro = _abi.CRefineOpts(*opts)
    rc = lib.mdx_refine_guests(md._h, len(recs), arr, None if no_opts else C.byref(ro), None if no_out else p(o[0]), p(o[1]), n_groups, p(o[2]), p(o[3]),
                               u(st), u(ev), u(bp), bs.ctypes.data_as(dp))
    msg = lib.mdx_last_error().decode()
    assert rc == -1 and match in msg, (rc, msg)
    assert all((v == -7.0).all() for v in o) and (st == 77).all() and (ev == 77).all() and (bp == 77).all() and (bs == -7.0).all(), \
        "a refused mdx_refine_guests must leave every output untouched"


def test_refusals(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    cfg = t.small_configs()[0]
    poses = small_poses(orc)[:2]
    n = lig.count
    keep = []
    good = lambda **kw: c_ligand(keep, **{**dict(charge=lig.charge, sigma=lig.lj_sigma, eps=lig.lj_eps, excl=lig.excl_pairs, p14=lig.pairs14,
                                                 poses=poses), **kw})
    with mdx.MdState(R, cfg) as md:
        refused(mdx, md, [good()], 2, "no energy groups")
        md.set_energy_groups(gR, 2)
        assert md.guest_forces([lig.with_poses(poses)])[0][0].shape == (2, n, 3)
        refused(mdx, md, [good()], 3, "n_groups")
        refused(mdx, md, [good()], 2, "null", no_out=True)
        refused(mdx, md, [good()], 2, "null", no_opts=True, refine_only=True)
        for hole in ("charge", "lj_sigma", "lj_eps", "excl_pairs", "pairs14", "poses"):
            r = good()
            setattr(r, hole, None)
            refused(mdx, md, [good(), r], 2, "ligand 1: null")
        r = good()
        r.count = 0
        refused(mdx, md, [r], 2, "ligand 0: count")
        big = np.zeros(257, np.float32)
        refused(mdx, md, [good(), good(), c_ligand(keep, big, big + 1, big, None, None, np.zeros((1, 257, 3), np.float32))], 2, "ligand 2: count")
        refused(mdx, md, [good(excl=np.array([[0, n]], np.uint32))], 2, "outside the ligand")
        refused(mdx, md, [good(p14=np.array([[n + 5, 1]], np.uint32))], 2, "outside the ligand")
        refused(mdx, md, [good(excl=np.array([[3, 3]], np.uint32))], 2, "with itself")
        both = np.asarray(lig.pairs14[:1])[:, ::-1]      # (the same pair, the other way round)
        refused(mdx, md, [good(excl=np.concatenate([lig.excl_pairs, both]))], 2, "both")
        for field, arr in (("charge", lig.charge), ("sigma", lig.lj_sigma), ("eps", lig.lj_eps)):
            bad = np.array(arr, np.float32)
            bad[n // 2] = np.nan
            refused(mdx, md, [good(**{field: bad})], 2, "non-finite")
        bad = np.array(lig.lj_eps, np.float32)
        bad[1] = -0.5
        refused(mdx, md, [good(eps=bad)], 2, "negative")
        for v in (np.nan, -np.inf):
            bad = poses.copy()
            bad[1, 7, 2] = v
            refused(mdx, md, [good(poses=bad)], 2, "non-finite pose coordinate")
        for opts, match in (((0, 0.1, 0.1, 0, 0), "max_evals"), ((_abi.REFINE_MAX_EVALS_CAP + 1, 0.1, 0.1, 0, 0), "max_evals"),
                            ((12, -0.1, 0.1, 0, 0), "negative"), ((12, 0.1, float("nan"), 0, 0), "not finite"),
                            ((12, 0.1, 0.1, 0.3, 0.25), "h_start"), ((12, 0.1, 0.1, 0.0, 0.005), "h_start")):
            refused(mdx, md, [good()], 2, match, opts=opts, refine_only=True)
        # atoms on top of each other: mdx_guest_forces fails as a whole and writes nothing
        lib = mdx.load_library()
        fp = C.POINTER(C.c_float)
        on_top = poses.copy()
        on_top[1, 0] = md.positions()[3]
        arr = (CGuestLigand * 1)(good(poses=on_top))
        o = [np.full((2, n, 3), -7.0, np.float32), np.full((2, 3), -7.0, np.float32), np.full((2, 6), -7.0, np.float32)]
        assert lib.mdx_guest_forces(md._h, 1, arr, o[1].ctypes.data_as(fp), 2, o[0].ctypes.data_as(fp), o[2].ctypes.data_as(fp)) == _abi.MDX_ENAN
        assert all((v == -7.0).all() for v in o)
        # nothing to do: no ligand, or no pose in the whole library
        out = np.full(3, -7.0, np.float32)
        assert lib.mdx_guest_forces(md._h, 0, None, None, 2, out.ctypes.data_as(fp), None) == 0
        arr = (CGuestLigand * 1)(good(poses=None))
        assert lib.mdx_guest_forces(md._h, 1, arr, None, 2, out.ctypes.data_as(fp), None) == 0
        ro = _abi.CRefineOpts(12, 0.0, 0.0, 0.0, 0.0)
        bp = np.full(1, 77, np.uint32)
        assert lib.mdx_refine_guests(md._h, 1, arr, C.byref(ro), out.ctypes.data_as(fp), None, 2, None, None, None, None,
                                     bp.ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0
        assert (out == -7.0).all() and bp[0] == 77
        f, rows, rigid = md.guest_forces([lig.with_poses(None)], rows=True, rigid=True)
        assert f[0].shape == (0, n, 3) and rows[0].shape == (0, 3) and rigid[0].shape == (0, 6)
    S3 = t.three_groups(S)
    with mdx.MdState(S, cfg) as md:
        md.set_energy_groups(S3, 3)
        md.configure_alchemical_window(1, 0.5)
        refused(mdx, md, [good()], 3, "alchemical")


def test_refused_on_a_decomposed_handle(mdx, orc):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    g = t.three_groups(s)
    _, _, _, _, lig = gc.small_case()
    poses = small_poses(orc)[:2]
    world = 2
    fabric = Fabric(world)
    errs = []
    lock = threading.Lock()
    keep = []

    def run(rank):
        try:
            with MdState(s, cfg) as md:
                md.set_energy_groups(g, 3)
                md.comm_init_fabric(fabric, rank)
                with lock:      # (mdx_last_error is per thread; the lock only keeps the output readable)
                    refused(mdx, md, [c_ligand(keep, lig.charge, lig.lj_sigma, lig.lj_eps, lig.excl_pairs, lig.pairs14, poses)], 3, "decomposed")
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [x.start() for x in th]
    [x.join() for x in th]
    if errs:
        raise errs[0]
