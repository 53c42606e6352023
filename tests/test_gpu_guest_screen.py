"""`mdx_screen_ligands` / `MdState.screen_ligands`: a library of guest ligands - described by the caller, never entered into the handle -
scored against the resident atoms, against the fp64 oracle (`orc.between_mols` on the COMBINED system: the environment with the guest
appended as one more molecule and one more group).

Tolerance per row element - `assert_row` of tests/test_gpu_pose_batch.py: |dM| <= 2e-6 |M| + 1e-6 G + 1e-3 + |M| 2^-23, G = the oracle's
gross sum of |e_pair| over the same pairs.  GPU against GPU (the twin): |d| <= 2e-6 |M| + 1e-6 G, as the existing twin test.

The small-complex cases use the environment, poses and seed of the resident-pose tests (at most 2 of 16 poses dropped for a clash
below 1.0 A); the mixed library's environment is carved so that nothing has to be dropped (tests/test_guest_screen_host.py checks both
on the CPU)."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import GuestLigand, MdConfig, systems
from molchanica_amd._abi import CGuestLigand

from tests import guest_cases as gc

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


def small_poses(orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    pos = orc.wrap(S, S.pos)
    return t.rigid_poses(t.whole(S, pos[lo:hi]), 16, SEED_SMALL)


@pytest.fixture(scope="module")
def small_rows(mdx, orc):
    """Test 1's screening, kept for the twin: per config (rows, positions of R, poses)."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    poses = small_poses(orc)
    out = []
    for cfg in t.small_configs():
        with mdx.MdState(R, cfg) as md:
            assert md.set_energy_groups(gR, 2) == 2
            pos = md.positions()
            (rows,) = md.screen_ligands([lig.with_poses(poses)])
            out.append((rows, pos, poses))
    return out


def test_rows_match_the_oracle_on_the_small_complex(mdx, orc, small_rows):
    S, R, gR, (lo, hi), lig = gc.small_case()
    g3 = t.three_groups(S)
    for cfg, (rows, pos_r, poses) in zip(t.small_configs(), small_rows):
        assert rows.shape == (16, 3) and rows.dtype == np.float32
        x = gc.s_positions(pos_r, lo, poses[0])
        keep = t.usable(S, x, lo, hi, poses)
        for k in np.flatnonzero(keep):
            ro, gr = t.oracle_row(orc, S, cfg, g3, 3, x, lo, hi, poses[k], 1)
            t.assert_row(rows[k], ro[[0, 2, 1]], gr[[0, 2, 1]], f"guest on the small complex, coulomb mode {cfg.coulomb_mode}, pose {k}")
        assert abs(rows[0, 0]) > 1e-3 and abs(rows[0, 1]) > 1e-3 and abs(rows[0, 2]) > 1e-3


def test_rows_agree_with_score_poses_on_a_twin(mdx, orc, small_rows):
    """GPU against GPU: the guest's rows against md.score_poses on a handle that holds the ligand as a resident."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    g3 = t.three_groups(S)
    for cfg, (rows, pos_r, poses) in zip(t.small_configs(), small_rows):
        with mdx.MdState(S, cfg) as twin:
            twin.set_energy_groups(g3, 3)
            assert np.array_equal(bits(np.delete(twin.positions(), np.s_[lo:hi], 0)), bits(pos_r)), "the twin's environment is R's"
            res = twin.score_poses(lo, poses).astype(np.float64)
        x = gc.s_positions(pos_r, lo, poses[0])
        keep = t.usable(S, x, lo, hi, poses)
        for k in np.flatnonzero(keep):
            _, gr = t.oracle_row(orc, S, cfg, g3, 3, x, lo, hi, poses[k], 1)
            m = res[k][[0, 2, 1]]
            tol = 2e-6 * np.abs(m) + 1e-6 * gr[[0, 2, 1]]
            print(f"twin, mode {cfg.coulomb_mode}, pose {k}: guest {rows[k]} resident {m} tol {tol}")
            assert np.all(np.abs(rows[k].astype(np.float64) - m) <= tol), (k, rows[k], m, tol)


def test_mixed_library_at_the_boundaries_of_the_kernel(mdx, orc):
    """One atom, the strip of 8 and its neighbours, the wave of 64 and its neighbour, the cap of 256, an empty ligand, 302 poses (the
    64-atom ligand's straddle pose 256), two alternating water groups."""
    env, groups, gs, ligs = gc.mixed_case()
    cfg = t.small_configs()[0]
    with mdx.MdState(env, cfg) as md:
        assert md.set_energy_groups(groups, 2) == 2
        pos = md.positions()
        rows = md.screen_ligands(ligs)
        assert [r.shape for r in rows] == [(n, 3) for n in gc.MIXED_POSES]
        # (a) bit for bit: the reversed library, and every (ligand, pose) alone
        back = md.screen_ligands(ligs[::-1])[::-1]
        for m, (a, b) in enumerate(zip(rows, back)):
            assert np.array_equal(bits(a), bits(b)), f"ligand {m} in the reversed library"
        for m, lig in enumerate(ligs):
            for p in range(lig.n_poses):
                (alone,) = md.screen_ligands([lig.with_poses(lig.poses[p:p + 1])])
                assert np.array_equal(bits(alone), bits(rows[m][p:p + 1])), f"ligand {m} pose {p} alone"
        # (b) one sampled pose per ligand against the oracle on the combined system
        for m, (g, lig) in enumerate(zip(gs, ligs)):
            if lig.n_poses == 0:
                continue
            p = (5 * m + 3) % lig.n_poses
            ro, gr = gc.guest_oracle_row(orc, env, groups, pos, g, lig.poses[p], cfg)
            t.assert_row(rows[m][p], ro, gr, f"mixed library, ligand {m} ({lig.count} atoms), pose {p}")
            assert np.abs(rows[m][p][:2]).max() > 1e-3, "the guest must see the water"
        # (c) a single atom has no pair of its own
        assert ligs[0].count == 1 and np.all(rows[0][:, 2] == 0.0)
        assert np.abs(rows[-1][:, 2]).min() > 1e-3


def test_periodic_images(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    cfg = t.small_configs()[0]
    box = np.asarray(R.box_hi, np.float32) - np.asarray(R.box_lo, np.float32)
    base = small_poses(orc)[0]
    shifts = [(1, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -2, 1), (2, -1, -2), (-2, 1, 2)]
    moved = [base + box * np.array(k, np.float32) for k in shifts]
    wrapped = base - np.floor((base - np.asarray(R.box_lo, np.float32)) / box) * box
    with mdx.MdState(R, cfg) as md:
        md.set_energy_groups(gR, 2)
        pos = md.positions()
        (rows,) = md.screen_ligands([lig.with_poses(np.stack([base] + moved + [wrapped]).astype(np.float32))])
        ro, gr = gc.guest_oracle_row(orc, R, gR, pos, gc.only_molecules(S, [1]), base, cfg)
        for k in range(rows.shape[0]):
            t.assert_row(rows[k], ro, gr, f"image {k} of the pose")
        assert abs(rows[0, 0]) > 1e-3 and abs(rows[0, 1]) > 1e-3


def separated(env_pos, guest_pos, gap):
    """guest_pos translated along x so that its closest atom is `gap` from the environment's."""
    g = np.asarray(guest_pos, np.float64) - np.asarray(guest_pos, np.float64).mean(0) + np.asarray(env_pos, np.float64).mean(0)
    lo_, hi_ = 0.0, 1000.0
    for _ in range(60):
        mid = 0.5 * (lo_ + hi_)
        d = np.linalg.norm((g + [mid, 0, 0])[:, None, :] - np.asarray(env_pos, np.float64)[None], axis=2).min()
        lo_, hi_ = (mid, hi_) if d < gap else (lo_, mid)
    return (g + [hi_, 0, 0]).astype(np.float32)


def test_vacuum_without_cutoff_and_far_away(mdx, orc):
    """The `all` branch on a non-periodic grid; then a guest 500 A away under a cutoff: nothing of the environment, its own energy."""
    s = systems.lig50()
    gsys = systems.lig50(seed=2)
    guest = GuestLigand.from_system(gsys, 0, gsys.n_atoms)
    g = np.zeros(s.n_atoms, np.uint8)
    cfg = MdConfig(lj_cutoff=0, coulomb_cutoff=0)
    with mdx.MdState(s, cfg) as md:
        assert md.set_energy_groups(g, 1) == 1
        pos = md.positions()
        near = separated(pos, gsys.pos, 6.0)
        (rows,) = md.screen_ligands([guest.with_poses(near[None])])
        ro, gr = gc.guest_oracle_row(orc, s, g, pos, gsys, near, cfg, use_cells=False)
        t.assert_row(rows[0], ro, gr, "lig50 beside lig50 in vacuum, no cutoff")
        assert abs(rows[0, 0]) > 1e-3 and abs(rows[0, 1]) > 1e-3
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 1)
        pos = md.positions()
        far = (near + np.array([500.0, -300.0, 250.0], np.float32)).astype(np.float32)
        (rows,) = md.screen_ligands([guest.with_poses(far[None])])
        ro, gr = gc.guest_oracle_row(orc, s, g, pos, gsys, far, cfg, use_cells=False)
        assert rows[0, 0] == 0.0 and ro[0] == 0.0
        t.assert_row(rows[0], ro, gr, "far guest")
        assert abs(rows[0, 1]) > 1e-3


def test_stale_structure_after_a_burst_of_steps(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    g3 = t.three_groups(S)
    cfg = t.small_configs()[0]
    poses = small_poses(orc)
    with mdx.MdState(R, cfg) as md:
        md.set_energy_groups(gR, 2)
        md.step(0.001, None, 30)      # the cluster boxes are 30 steps old
        pos = md.positions()
        x = gc.s_positions(pos, lo, poses[0])
        keep = t.usable(S, x, lo, hi, poses)
        (rows,) = md.screen_ligands([lig.with_poses(poses)])
        for k in np.flatnonzero(keep):
            ro, gr = t.oracle_row(orc, S, cfg, g3, 3, x, lo, hi, poses[k], 1)
            t.assert_row(rows[k], ro[[0, 2, 1]], gr[[0, 2, 1]], f"after 30 steps, pose {k}")


def test_the_handle_is_untouched(mdx, orc):
    S, R, gR, (lo, hi), lig = gc.small_case()
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)      # the deterministic pair kernel
    poses = small_poses(orc)
    with mdx.MdState(R, cfg) as md, mdx.MdState(R, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(gR, 2)
            m.step(0.0005, None, 4)
        rebuilds = md.stats()["rebuild_count"]
        x0, f0, v0 = md.positions(), md.forces(), md.velocities()
        md.screen_ligands([lig.with_poses(poses)], best=True)
        assert md.stats()["rebuild_count"] == rebuilds, "screening must not rebuild the list of a ready handle"
        x1, f1, v1 = md.positions(), md.forces(), md.velocities()
        assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1)) and np.array_equal(bits(v0), bits(v1))
        twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        for what in ("positions", "velocities", "forces"):
            assert np.array_equal(bits(getattr(md, what)()), bits(getattr(twin, what)())), what
        assert md.stats()["rebuild_count"] == twin.stats()["rebuild_count"]
    # the resident-pose table of a handle survives a screening on it
    g3 = t.three_groups(S)
    with mdx.MdState(S, cfg) as md:
        md.set_energy_groups(g3, 3)
        before = md.score_poses(lo, poses)
        other = systems.lig50(seed=4, n_atoms=23)
        og = GuestLigand.from_system(other, 0, 23, poses=(other.pos - other.pos.mean(0) + np.asarray(S.pos[lo:hi]).mean(0) + [0, 0, 9.0])[None])
        md.screen_ligands([og], best=True)
        after = md.score_poses(lo, poses)
        assert np.array_equal(bits(before), bits(after))


def test_best_pose_is_the_host_argmin_of_the_returned_rows(mdx, orc):
    env, groups, gs, ligs = gc.mixed_case()
    cfg = t.small_configs()[1]
    twice = ligs[4].with_poses(np.concatenate([ligs[4].poses[7:8], ligs[4].poses[:8]]))      # pose 0 again at index 8
    lib_ = list(ligs) + [twice]
    with mdx.MdState(env, cfg) as md:
        md.set_energy_groups(groups, 2)
        rows, (bp, bs) = md.screen_ligands(lib_, best=True)
        assert bp.dtype == np.uint32 and bs.dtype == np.float64 and bp.shape == bs.shape == (len(lib_),)
        for m, r in enumerate(rows):
            if r.shape[0] == 0:
                assert bp[m] == 0xFFFFFFFF and bs[m] == np.inf
                continue
            S_ = np.zeros(r.shape[0], np.float64)
            for c in range(r.shape[1]):
                S_ += r[:, c].astype(np.float64)
            assert bp[m] == int(np.argmin(S_)), (m, bp[m], S_)
            assert bs[m] == S_[bp[m]]
        assert np.array_equal(bits(rows[-1][0]), bits(rows[-1][8])), "the same pose twice gives the same bits"
        # a ligand that is nothing but one pose repeated: the tie goes to the lowest index
        same = ligs[5].with_poses(np.stack([ligs[5].poses[3]] * 5))
        _, (bp1, _) = md.screen_ligands([same], best=True)
        assert bp1[0] == 0
        assert gc.MIXED_POSES[2] == 0 and bp[2] == 0xFFFFFFFF


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def c_ligand(keep, charge, sigma, eps, excl, p14, poses):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    r = CGuestLigand()

    def hold(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a

    q, sg, ep = hold(charge, np.float32), hold(sigma, np.float32), hold(eps, np.float32)
    ex, pp, ps = hold(excl, np.uint32), hold(p14, np.uint32), hold(poses, np.float32)
    r.count = 0 if q is None else q.shape[0]
    r.charge = None if q is None else q.ctypes.data_as(fp)
    r.lj_sigma = None if sg is None else sg.ctypes.data_as(fp)
    r.lj_eps = None if ep is None else ep.ctypes.data_as(fp)
    r.n_excl, r.excl_pairs = (0, None) if ex is None else (ex.reshape(-1, 2).shape[0], ex.ctypes.data_as(up))
    r.n_pairs14, r.pairs14 = (0, None) if pp is None else (pp.reshape(-1, 2).shape[0], pp.ctypes.data_as(up))
    r.n_poses, r.poses = (0, None) if ps is None else (ps.shape[0], ps.ctypes.data_as(fp))
    return r


def refused(mdx, md, recs, n_groups, match, rows_null=False):
    lib = mdx.load_library()
    fp = C.POINTER(C.c_float)
    arr = (CGuestLigand * len(recs))(*recs)
    n = sum(r.n_poses for r in recs)
    out = np.full((max(n, 1), max(n_groups, 1) + 1), -7.0, np.float32)
    bp = np.full(len(recs), 77, np.uint32)
    bs = np.full(len(recs), -7.0, np.float64)
    rc = lib.mdx_screen_ligands(md._h, len(recs), arr, None if rows_null else out.ctypes.data_as(fp), n_groups,
                                bp.ctypes.data_as(C.POINTER(C.c_uint32)), bs.ctypes.data_as(C.POINTER(C.c_double)))
    msg = lib.mdx_last_error().decode()
    assert rc == -1, (rc, msg)
    assert (out == -7.0).all() and (bp == 77).all() and (bs == -7.0).all(), "a refused call must leave every output untouched"
    assert match in msg, msg


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
        assert md.screen_ligands([lig.with_poses(poses)])[0].shape == (2, 3)
        refused(mdx, md, [good()], 3, "n_groups")
        refused(mdx, md, [good()], 2, "null", rows_null=True)
        for hole in ("charge", "sigma", "eps", "excl", "p14", "poses"):
            r = good()
            setattr(r, dict(charge="charge", sigma="lj_sigma", eps="lj_eps", excl="excl_pairs", p14="pairs14", poses="poses")[hole], None)
            refused(mdx, md, [good(), r], 2, "ligand 1: null")
        r = good()
        r.count = 0
        refused(mdx, md, [r], 2, "ligand 0: count")
        big = np.zeros(257, np.float32)
        refused(mdx, md, [good(), good(), c_ligand(keep, big, big + 1, big, None, None, np.zeros((1, 257, 3), np.float32))], 2, "ligand 2: count")
        refused(mdx, md, [good(excl=np.array([[0, n]], np.uint32))], 2, "outside the ligand")
        refused(mdx, md, [good(p14=np.array([[n + 5, 1]], np.uint32))], 2, "outside the ligand")
        refused(mdx, md, [good(excl=np.array([[3, 3]], np.uint32))], 2, "with itself")
        refused(mdx, md, [good(p14=np.array([[4, 4]], np.uint32))], 2, "with itself")
        both = np.asarray(lig.pairs14[:1])[:, ::-1]      # (the same pair, the other way round)
        refused(mdx, md, [good(excl=np.concatenate([lig.excl_pairs, both]))], 2, "both")
        for field, arr in (("charge", lig.charge), ("sigma", lig.lj_sigma), ("eps", lig.lj_eps)):
            for v in (np.nan, np.inf):
                bad = np.array(arr, np.float32)
                bad[n // 2] = v
                refused(mdx, md, [good(**{field: bad})], 2, "non-finite")
        for field, arr in (("sigma", lig.lj_sigma), ("eps", lig.lj_eps)):
            bad = np.array(arr, np.float32)
            bad[1] = -0.5
            refused(mdx, md, [good(**{field: bad})], 2, "negative")
        for v in (np.nan, -np.inf):
            bad = poses.copy()
            bad[1, 7, 2] = v
            refused(mdx, md, [good(poses=bad)], 2, "non-finite pose coordinate")
        # nothing to do: no ligand, or no pose in the whole library
        lib = mdx.load_library()
        out = np.full(3, -7.0, np.float32)
        bp = np.full(1, 77, np.uint32)
        fp = C.POINTER(C.c_float)
        assert lib.mdx_screen_ligands(md._h, 0, None, out.ctypes.data_as(fp), 2, None, None) == 0
        arr = (CGuestLigand * 1)(good(poses=None))
        assert lib.mdx_screen_ligands(md._h, 1, arr, out.ctypes.data_as(fp), 2, bp.ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0
        assert (out == -7.0).all() and bp[0] == 77
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
