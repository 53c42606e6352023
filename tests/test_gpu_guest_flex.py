"""`mdx_refine_guests_flex` / `MdState.refine_guests_flex`: the flexible refinement of a library of guest ligands on the device.

Against the host loop it replaces - the numpy stepper of tests/pose_flex_ref.py driven by `MdState.guest_forces` - by the criteria of
tests/test_gpu_pose_flex.py: status and evaluation count equal for every pose, coordinates within 4 ulp32(max |coordinate|), (q, t,
theta) within 1e-5; dih_out and tgrad_out within `assert_dih` / `assert_tgrad` of the restatement at poses_out.  Against itself:
rows_out / rigid_out are the bits `screen_ligands` / `guest_forces` return for poses_out; without torsions and flags every shared
output is `refine_guests` bit for bit; a (ligand, pose) gives the same bits alone, in a library of any size and order.  No tolerance
of its own: all are imported.

The start poses on the small complex are those of tests/test_pose_flex_host.py (R plus the guest's pose is S: the same geometry);
tests/test_guest_flex_host.py holds their clash conditions on the CPU, so nothing here needs a drop allowance."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import GuestFlex, MdConfig, _abi, systems
from tests import guest_cases as gc
from tests import guest_flex_cases as fc
from tests import pose_flex_ref as F
from tests import pose_refine_ref as P
from tests.test_gpu_guest_refine import row_sums, two_sizes
from tests.test_gpu_pose_flex import assert_dih, assert_tgrad, bits, ulp32

pytestmark = pytest.mark.gpu

t = gc.pose_batch_module()
NAMES = ("poses", "rows", "rigid", "xform", "dih", "tgrad", "status", "evals")
RIGID_OF_FLEX = (0, 1, 2, 3, 6, 7)      # the outputs refine_guests has too


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def same(a, b, what, names=NAMES):
    for x, y, name in zip(a, b, names):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), f"{what}: {name} differ"


def guest_evaluate(mdx, md, lig):
    """`evaluate` of the host loop: one guest_forces call per evaluation -> (row, rigid, forces) (MDX_ENAN: all NaN)"""
    def evaluate(Y):
        try:
            (f,), (row,), (rigid,) = md.guest_forces([lig.with_poses(np.ascontiguousarray(Y[None]))], rows=True, rigid=True)
        except mdx.BlowUpError:
            W = int(mdx.load_library().mdx_energy_group_count(md._h)) + 1
            return np.full(W, np.nan, np.float32), np.full(6, np.nan, np.float32), np.full(Y.shape, np.nan, np.float32)
        return row[0], rigid[0], f[0]
    return evaluate


def host_loop(mdx, md, lig, flex, poses, box, max_evals, f_tol=0.0, tau_tol=0.0, tors_tol=0.0, h_start=0.0, h_max=0.0, dihedrals=True):
    tors = fc.sides_of(flex, lig.count)
    terms = fc.terms_of(flex) if dihedrals else F.NO_TERMS
    return F.refine_batch(poses, guest_evaluate(mdx, md, lig), tors, terms, max_evals, f_tol, tau_tol, tors_tol, h_start, h_max, box)


def held_against(mine, host, what):
    """The criteria of tests/test_gpu_pose_flex.py"""
    assert np.array_equal(mine[6], host[6]), f"{what}: status device {mine[6].tolist()} host {host[6].tolist()}"
    assert np.array_equal(mine[7], host[7]), f"{what}: evaluations device {mine[7].tolist()} host {host[7].tolist()}"
    differ = int((bits(mine[0]) != bits(host[0])).sum())
    worst = float(np.abs(mine[0].astype(np.float64) - host[0].astype(np.float64)).max()) / ulp32(host[0])
    dx = float(np.abs(mine[3] - host[3]).max())
    print(f"{what}: status {mine[6].tolist()}, evaluations {mine[7].tolist()}; {differ} of {mine[0].size} coordinates not bit-equal to the "
          f"host loop's, worst difference {worst:.2f} ulp32(max |coordinate|); (q, t, theta) within {dx:.1e}")
    assert worst <= 4.0, f"{what}: a coordinate differs from the host loop's by {worst:.1f} ulp32"
    assert dx <= 1e-5, f"{what}: xform {dx}"


def self_consistent(mdx, md, lig, flex, mine, box, dihedrals, what):
    """rows_out / rigid_out are the bits screen_ligands / guest_forces return for poses_out; dih_out and tgrad_out are the restatement's"""
    ok = mine[6] != P.NONFINITE
    y = np.ascontiguousarray(mine[0][ok])
    again = [lig.with_poses(y)]
    assert np.array_equal(bits(mine[1][ok]), bits(md.screen_ligands(again)[0])), f"{what}: rows_out is not screen_ligands(poses_out)"
    (f,), (rows,), (rigid,) = md.guest_forces(again, rows=True, rigid=True)
    assert np.array_equal(bits(mine[2][ok]), bits(rigid)), f"{what}: rigid_out is not that of guest_forces(poses_out)"
    tors = fc.sides_of(flex, lig.count)
    terms = fc.terms_of(flex) if dihedrals else F.NO_TERMS
    E, G, floor = [], [], []
    for k in range(len(y)):
        e, ft, g, J, A, U = F.state_of(y[k], f[k], rigid[k], tors, terms, box)
        x = y[k].astype(np.float64)
        v = rigid[k, :3].astype(np.float64) / len(x)
        floor.append([1e-10 * float((np.linalg.norm(np.cross(U[j], x[m] - x[b]), axis=1) * np.linalg.norm(ft[m] - v, axis=1)).sum())
                      for j, (a, b, m) in enumerate(tors)])
        E.append(e), G.append(g)
    assert_dih(mine[4][ok], np.array(E, np.float32), terms, what)
    assert_tgrad(mine[5][ok], np.array(G).reshape(len(y), len(tors)), np.array(floor).reshape(len(y), len(tors)), what)


# ---- 1, 2: the small complex against the host loop, and against itself ---------------------------------------------------------------------
@pytest.mark.parametrize("dihedrals", [True, False])
@pytest.mark.parametrize("n_tors", [0, 8, 31])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_equals_the_host_loop(mdx, mode, n_tors, dihedrals):
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    flex = fc.small_flex(n_tors)
    cfg = t.small_configs()[mode]
    what = f"coulomb mode {cfg.coulomb_mode}, {n_tors} torsions, dihedral terms {'on' if dihedrals else 'off'}"
    with mdx.MdState(R, cfg) as md:
        md.set_energy_groups(gR, 2)
        dev = md.refine_guests_flex([lig], [flex], 12, 0.0, 0.0, 0.0, dihedrals=dihedrals)
        mine = [v[0] for v in dev]
        assert mine[0].shape == lig.poses.shape and mine[1].shape == (16, 3) and mine[2].shape == (16, 6)
        assert mine[3].shape == (16, 7 + n_tors) and mine[4].shape == (16,) and mine[5].shape == (16, n_tors)
        held_against(mine, host_loop(mdx, md, lig, flex, lig.poses, fc.box_of(R), 12, dihedrals=dihedrals), what)
        assert (mine[7] == 12).all() and (mine[6] == P.MAX_EVALS).all()
        assert (mine[4] > 0).all() if dihedrals else (mine[4] == 0).all()
        assert n_tors == 0 or np.abs(mine[3][:, 7:]).max() > 1e-3
        self_consistent(mdx, md, lig, flex, mine, fc.box_of(R), dihedrals, what)


@pytest.mark.parametrize("n_tors,dihedrals", [(31, True), (8, False), (0, True)])
def test_equals_the_host_loop_through_rejects(mdx, n_tors, dihedrals):
    """h_start = h_max = 0.2 A and the tolerances of tests/test_gpu_pose_flex.py: 48 evaluations with rejects, poses that converge at
    different evaluation counts share the chunk with live ones."""
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    flex = fc.small_flex(n_tors)
    what = f"h_start = h_max = 0.2 A, {n_tors} torsions, dihedral terms {'on' if dihedrals else 'off'}"
    args = dict(f_tol=20.0, tau_tol=60.0, tors_tol=80.0, h_start=0.2, h_max=0.2, dihedrals=dihedrals)
    with mdx.MdState(R, t.small_configs()[0]) as md:
        md.set_energy_groups(gR, 2)
        dev = md.refine_guests_flex([lig], [flex], 48, 20.0, 60.0, 80.0, 0.2, 0.2, dihedrals=dihedrals)
        mine = [v[0] for v in dev]
        held_against(mine, host_loop(mdx, md, lig, flex, lig.poses, fc.box_of(R), 48, **args), what)
        assert (mine[7] >= 1).all() and (mine[7] <= 48).all() and len(set(mine[7].tolist())) > 1
        self_consistent(mdx, md, lig, flex, mine, fc.box_of(R), dihedrals, what)


# ---- 3: no torsion, no flag ------------------------------------------------------------------------------------------------------------------
def test_no_torsion_and_no_flag_is_refine_guests_bit_for_bit(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    lib_ = two_sizes(orc)
    empty = [GuestFlex(), GuestFlex()]
    graph = [GuestFlex.from_system(S, lo, hi, 0, np.zeros((0, 2), np.uint32)), GuestFlex()]      # bonds and terms listed, none used
    for cfg in t.small_configs():
        with mdx.MdState(R, cfg) as md:
            md.set_energy_groups(gR, 2)
            for args in ((12, 0.0, 0.0, 0.0, 0.0), (48, 2.0, 6.0, 0.2, 0.2)):
                *rigid, (bp, bs) = md.refine_guests(lib_, *args, best=True)
                for flex in (empty, graph):
                    *dev, (fbp, fbs) = md.refine_guests_flex(lib_, flex, args[0], args[1], args[2], 0.0, args[3], args[4], dihedrals=False, best=True)
                    for m in range(2):
                        same([v[m] for v in rigid], [dev[k][m] for k in RIGID_OF_FLEX], f"coulomb mode {cfg.coulomb_mode}, {args[0]} evaluations, ligand {m}",
                             ("poses", "rows", "rigid", "xform", "status", "evals"))
                        assert dev[3][m].shape[1] == 7 and dev[5][m].shape == (lib_[m].n_poses, 0) and (dev[4][m] == 0).all()
                    assert np.array_equal(bp, fbp) and np.array_equal(bs.view(np.uint64), fbs.view(np.uint64))
            assert len(set(np.concatenate(rigid[5]).tolist())) > 1, "the 48-evaluation run should hold poses that end differently"


# ---- 4: one evaluation -----------------------------------------------------------------------------------------------------------------------
def test_one_evaluation_returns_the_input_and_the_dihedral_energy_of_the_resident_twin(mdx):
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    flex = fc.small_flex(31)
    cfg = t.small_configs()[0]
    with mdx.MdState(R, cfg) as md, mdx.MdState(S, cfg) as twin:
        md.set_energy_groups(gR, 2)
        twin.set_energy_groups(t.three_groups(S), 3)
        y, rows, rigid, xform, dih, tgrad, status, evals = (v[0] for v in md.refine_guests_flex([lig], [flex], 1, 0.0, 0.0, 0.0))
        assert np.array_equal(bits(y), bits(lig.poses)) and (evals == 1).all() and (status == P.MAX_EVALS).all()
        assert np.array_equal(xform, np.tile(np.array([1, 0, 0, 0, 0, 0, 0] + [0] * 31, np.float32), (16, 1)))
        f, (frows,), (frigid,) = md.guest_forces([lig], rows=True, rigid=True)
        assert np.array_equal(bits(rows), bits(frows)) and np.array_equal(bits(rigid), bits(frigid))
        # E_dih depends on the pose and the terms alone: the one quantity a handle that holds the ligand as a resident reproduces exactly
        tdih = twin.refine_poses_flex(lo, lig.poses, 0, tb, 1, 0.0, 0.0, 0.0)[4]
        assert np.array_equal(bits(dih), bits(tdih)) and (dih > 0).all(), (dih, tdih)
        assert np.abs(tgrad).max() > 1.0


# ---- 5: the mixed library ----------------------------------------------------------------------------------------------------------------------
def test_mixed_library_at_the_boundaries_of_the_kernels(mdx):
    env, groups, lib_, flex = fc.mixed_flex_case()
    assert [l.count for l in lib_] == [1, 2, 7, 7, 8, 9, 50, 64, 65, 256, 4]
    assert [f.n_torsions for f in flex] == [0, 0, 2, 2, 3, 3, 28, 32, 32, 32, 1]
    assert len(flex[9].dihedral_idx) > 256 and len(flex[0].dihedral_idx) == 0 and len(flex[10].dihedral_idx) == 1
    edges = np.concatenate([[0], np.cumsum([l.n_poses for l in lib_])])
    assert lib_[2].n_poses == 0 and edges[7] < 256 < edges[8] and lib_[7].count == 64
    cfg = t.small_configs()[0]
    args = (6, 0.0, 0.0, 0.0)
    with mdx.MdState(env, cfg) as md:
        assert md.set_energy_groups(groups, 2) == 2
        full = md.refine_guests_flex(lib_, flex, *args)
        assert [x.shape for x in full[3]] == [(l.n_poses, 7 + f.n_torsions) for l, f in zip(lib_, flex)]
        assert [g.shape for g in full[5]] == [(l.n_poses, f.n_torsions) for l, f in zip(lib_, flex)]
        back = [v[::-1] for v in md.refine_guests_flex(lib_[::-1], flex[::-1], *args)]
        start = md.screen_ligands(lib_)
        for m, (lig, fx) in enumerate(zip(lib_, flex)):
            mine = [v[m] for v in full]
            same(mine, [v[m] for v in back], f"ligand {m} ({lig.count} atoms) in the reversed library")
            if lig.n_poses == 0:
                continue
            same(mine, [v[0] for v in md.refine_guests_flex([lig], [fx], *args)], f"ligand {m} ({lig.count} atoms) by itself")
            assert (mine[7] >= 1).all() and (mine[7] <= 6).all() and np.isin(mine[6], (P.CONVERGED, P.MAX_EVALS, P.STALLED)).all()
            E0 = np.array([np.float32(F.dihedral(p, fc.terms_of(fx), fc.box_of(env))[0]) for p in lig.poses], np.float64)
            assert (row_sums(mine[1]) + mine[4].astype(np.float64) <= row_sums(start[m]) + E0).all(), f"ligand {m}: the objective rose"
            # the host loop on the ligand's first and last pose and on the library's poses 255 and 256: bitwise independence of the
            # library makes the subset sufficient
            pick = sorted({0, lig.n_poses - 1} | {p - int(edges[m]) for p in (255, 256) if edges[m] <= p < edges[m + 1]})
            sub = np.ascontiguousarray(lig.poses[pick])
            host = host_loop(mdx, md, lig, fx, sub, fc.box_of(env), 6)
            held_against([v[pick] for v in mine], host, f"ligand {m} ({lig.count} atoms, {fx.n_torsions} torsions), poses {pick}")
            self_consistent(mdx, md, lig, fx, [v[pick] for v in mine], fc.box_of(env), True, f"ligand {m}")
        assert np.abs(full[3][10][:, 7:]).max() > 0 and np.abs(full[3][9][:, 7:]).max() > 0, "the chain's and the largest ligand's torsions turn"
        assert (full[4][0] == 0).all() and (full[4][9] > 0).all()


# ---- 6: the best pose ------------------------------------------------------------------------------------------------------------------------
def test_best_pose_is_the_host_argmin_of_rows_plus_dihedral_energy(mdx):
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    poses = lig.poses
    fx = fc.small_flex(31)
    other = systems.lig50(seed=4, n_atoms=23)
    from molchanica_amd import GuestLigand
    start = np.asarray(other.pos, np.float64) - np.asarray(other.pos, np.float64).mean(0) + poses[0].astype(np.float64).mean(0)
    b, fb = GuestLigand.from_system(other, 0, 23, poses=t.rigid_poses(start, 8, t.SEED_SMALL + 1)), GuestFlex.from_system(other, 0, 23)
    with mdx.MdState(R, t.small_configs()[1]) as md:
        md.set_energy_groups(gR, 2)
        on_top = poses[5].copy()
        on_top[0] = md.positions()[3]      # its first atom on an atom of the receptor: not finite at evaluation 0
        lib_ = [lig, b.with_poses(None), lig.with_poses(np.concatenate([poses[7:8], poses[:8]])), lig.with_poses(on_top[None]),
                lig.with_poses(np.stack([on_top, poses[2], on_top, poses[2]])), b, lig.with_poses(np.stack([poses[3]] * 5))]
        flex = [fx, fb, fx, fx, fx, fb, fx]
        *out, (bp, bs) = md.refine_guests_flex(lib_, flex, 10, 0.0, 0.0, 0.0, best=True)
        rows, dih, status = out[1], out[4], out[6]
        assert bp.dtype == np.uint32 and bs.dtype == np.float64 and bp.shape == bs.shape == (len(lib_),)
        for m, r in enumerate(rows):
            ok = status[m] != P.NONFINITE
            if not ok.any():
                assert bp[m] == 0xFFFFFFFF and bs[m] == np.inf, (m, bp[m], bs[m])
                continue
            S_ = np.where(ok, row_sums(np.where(np.isfinite(r), r, 0)) + np.where(ok, dih[m], 0).astype(np.float64), np.inf)
            assert bp[m] == int(np.argmin(S_)), (m, bp[m], S_)
            assert bs[m] == S_[bp[m]] and (dih[m][ok] > 0).all()
        assert status[3].tolist() == [P.NONFINITE] and status[4].tolist() == [P.NONFINITE, P.MAX_EVALS] * 2
        assert np.array_equal(bits(rows[2][0]), bits(rows[2][8])) and bp[2] != 8, "the same pose twice refines to the same bits; the lower index wins"
        assert bp[4] == 1 and bp[6] == 0
        plain = md.refine_guests_flex(lib_, flex, 10, 0.0, 0.0, 0.0)
        for m in range(len(lib_)):
            same([v[m] for v in out], [v[m] for v in plain], f"ligand {m} with and without best")


# ---- 7: the handle, and the refusals that need a device ----------------------------------------------------------------------------------------
def test_the_handle_is_untouched(mdx):
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    fx = fc.small_flex(31)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)      # the fixed-order pair kernel
    with mdx.MdState(R, cfg) as md, mdx.MdState(R, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(gR, 2)
            m.step(0.0005, None, 4)
        rebuilds = md.stats()["rebuild_count"]
        x0, f0, v0 = md.positions(), md.forces(), md.velocities()
        md.refine_guests_flex([lig], [fx], 12, 0.0, 0.0, 0.0, best=True)
        assert md.stats()["rebuild_count"] == rebuilds, "the guest call must not rebuild the list of a ready handle"
        x1, f1, v1 = md.positions(), md.forces(), md.velocities()
        assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1)) and np.array_equal(bits(v0), bits(v1))
        twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        for what in ("positions", "velocities", "forces"):
            assert np.array_equal(bits(getattr(md, what)()), bits(getattr(twin, what)())), what
    # the resident-pose caches of a handle (the range's table, the torsion table) survive the call
    with mdx.MdState(S, cfg) as md:
        md.set_energy_groups(t.three_groups(S), 3)
        before = md.score_poses(lo, lig.poses)
        fbefore = md.refine_poses_flex(lo, lig.poses, 0, tb, 6, 0.0, 0.0, 0.0)
        other = lig.with_poses(lig.poses + np.array([0, 0, 9.0], np.float32))
        md.refine_guests_flex([other], [fc.small_flex(8)], 6, 0.0, 0.0, 0.0, best=True)
        assert np.array_equal(bits(before), bits(md.score_poses(lo, lig.poses)))
        same(fbefore, md.refine_poses_flex(lo, lig.poses, 0, tb, 6, 0.0, 0.0, 0.0), "refine_poses_flex after the guest call")


def raw_call(mdx, md, ligs, flex, n_groups, opts=(12, 0.0, 0.0, 0.0, 0.0, 0.0, 0), patch=None):
    """mdx_refine_guests_flex through ctypes with every output preset -> (return code, message, whether all outputs are as they were);
    patch(records): changes the mdx_guest_flex records behind the wrapper's own checks"""
    lib = mdx.load_library()
    fp, up, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    M, recs, counts, (sizes, _keep) = md._guest_records("test", ligs)
    frecs, T, _fkeep = md._guest_flex_records("test", flex, sizes)
    if patch:
        patch(frecs)
    n = max(sum(counts), 1)
    nx = max(sum(3 * a * p for a, p in zip(sizes, counts)), 1)
    W = max(n_groups, 1) + 1
    o = [np.full(nx, -7.0, np.float32), np.full((n, W), -7.0, np.float32), np.full((n, 6), -7.0, np.float32), np.full((n, 7 + 32), -7.0, np.float32),
         np.full(n, -7.0, np.float32), np.full((n, 32), -7.0, np.float32)]
    st, ev, bp, bs = np.full(n, 77, np.uint32), np.full(n, 77, np.uint32), np.full(M, 77, np.uint32), np.full(M, -7.0, np.float64)
    p = lambda a: a.ctypes.data_as(fp)
    u = lambda a: a.ctypes.data_as(up)
    fo = _abi.CFlexOpts(*opts)
    rc = lib.mdx_refine_guests_flex(md._h, M, recs, frecs, C.byref(fo), p(o[0]), p(o[1]), n_groups, p(o[2]), p(o[3]), p(o[4]), p(o[5]), u(st), u(ev),
                                    u(bp), bs.ctypes.data_as(dp))
    clean = all((v == -7.0).all() for v in o) and (st == 77).all() and (ev == 77).all() and (bp == 77).all() and (bs == -7.0).all()
    return rc, lib.mdx_last_error().decode(), clean


def test_refusals_that_need_a_device_write_nothing(mdx):
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    fx = fc.small_flex(8)
    two = lig.with_poses(lig.poses[:2])
    cfg = t.small_configs()[0]

    def refused(md, ligs, flex, n_groups, match, **kw):
        rc, msg, clean = raw_call(mdx, md, ligs, flex, n_groups, **kw)
        assert rc == _abi.MDX_EPARAM and match in msg, (rc, msg)
        assert clean, f"a refused mdx_refine_guests_flex must leave every output untouched ({match})"

    with mdx.MdState(R, cfg) as md:
        refused(md, [two], [fx], 2, "no energy groups")
        md.set_energy_groups(gR, 2)
        refused(md, [two], [fx], 3, "n_groups")
        ring = GuestFlex(bonds=np.array([[0, 1], [1, 2], [2, 3], [3, 0], [3, 4], [4, 5]] + [[k, k + 1] for k in range(5, lig.count - 1)], np.uint32),
                         torsion_bonds=np.array([[3, 4], [1, 2]], np.uint32))
        refused(md, [two, two], [fx, ring], 2, "ligand 1: torsion 1")
        # the caller's graph, torsions and terms: every rule, on a plain chain of the ligand's size
        n = lig.count
        chain = np.array([[k, k + 1] for k in range(n - 1)], np.uint32)
        term = dict(dihedral_idx=np.array([[0, 1, 2, 3]], np.uint32), dihedral_v=np.ones(1, np.float32), dihedral_phase=np.zeros(1, np.float32),
                    dihedral_n=np.ones(1, np.int32))
        tbs = lambda *pairs: np.array(pairs, np.uint32).reshape(-1, 2)
        assert raw_call(mdx, md, [two], [GuestFlex(bonds=chain, torsion_bonds=tbs((5, 6), (20, 19)), **term)], 2)[0] == 0
        for bad, match in ((GuestFlex(bonds=tbs((0, n))), "bond 0 names an atom index"),
                           (GuestFlex(bonds=np.concatenate([chain, tbs((3, 3))])), f"bond {n - 1} names the same atom twice"),
                           (GuestFlex(bonds=chain, torsion_bonds=tbs((5, 6), (0, 5))), "torsion 1: the two atoms are not bonded"),
                           (GuestFlex(bonds=chain, torsion_bonds=tbs((5, 6), (6, 5))), "torsion 1: the bond is listed twice"),
                           (GuestFlex(bonds=chain, torsion_bonds=tbs((0, 1))), "torsion 0: one side of the bond is a single atom"),
                           (GuestFlex(bonds=chain, torsion_bonds=tbs((7, 7))), "torsion 0 names the same atom twice"),
                           (GuestFlex(bonds=chain[:-1], torsion_bonds=tbs((5, 6))), "the bond graph of the range is not connected"),
                           (GuestFlex(bonds=chain, **{**term, "dihedral_idx": np.array([[0, 1, 2, n]], np.uint32)}), "dihedral term 0 names an atom index"),
                           (GuestFlex(bonds=chain, **{**term, "dihedral_v": np.array([np.nan], np.float32)}), "dihedral term 0: v or phase is not finite"),
                           (GuestFlex(bonds=chain, **{**term, "dihedral_phase": np.array([np.inf], np.float32)}), "dihedral term 0: v or phase is not finite")):
            refused(md, [two, two], [fx, bad], 2, "ligand 1: " + match)
        ok = GuestFlex(bonds=chain, torsion_bonds=tbs((5, 6)), **term)

        def setter(**kw):
            def patch(recs):
                for k, v in kw.items():
                    setattr(recs[0], k, v)
            return patch
        for kw, match in ((dict(n_torsions=33), "n_torsions exceeds MDX_POSE_MAX_TORSIONS"), (dict(torsion_bonds=None), "null"), (dict(bonds=None), "null"),
                          (dict(dihedral_v=None), "null"), (dict(dihedral_n=None), "null"), (dict(root=n), "root")):
            refused(md, [two], [ok], 2, "ligand 0: " + match, patch=setter(**kw))
        with pytest.raises(mdx.ParamError, match="names an atom index"):
            md.refine_guests_flex([two], [GuestFlex(bonds=chain, torsion_bonds=tbs((5, n)))], 12, 0.0, 0.0, 0.0)
        refused(md, [two], [fx], 2, "unknown flag", opts=(12, 0.0, 0.0, 0.0, 0.0, 0.0, 2))
        refused(md, [two], [fx], 2, "negative", opts=(12, 0.0, 0.0, -1.0, 0.0, 0.0, 1))
        rc, msg, clean = raw_call(mdx, md, [two.with_poses(None)], [fx], 2)
        assert rc == 0 and clean, "a library without a pose succeeds and writes nothing"
        rc, msg, clean = raw_call(mdx, md, [two], [fx], 2)
        assert rc == 0 and not clean
    with mdx.MdState(S, cfg) as md:
        md.set_energy_groups(t.three_groups(S), 3)
        md.configure_alchemical_window(1, 0.5)
        refused(md, [two], [fx], 3, "alchemical")


def test_refused_on_a_decomposed_handle(mdx):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    g = t.three_groups(s)
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    two, fx = lig.with_poses(lig.poses[:2]), fc.small_flex(8)
    world = 2
    fabric = Fabric(world)
    errs = []
    lock = threading.Lock()

    def run(rank):
        try:
            with MdState(s, cfg) as md:
                md.set_energy_groups(g, 3)
                md.comm_init_fabric(fabric, rank)
                with lock:      # (mdx_last_error is per thread; the lock only keeps the output readable)
                    rc, msg, clean = raw_call(mdx, md, [two], [fx], 3)
                    assert rc == _abi.MDX_EPARAM and "decomposed" in msg and clean, (rc, msg, clean)
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [x.start() for x in th]
    [x.join() for x in th]
    if errs:
        raise errs[0]
