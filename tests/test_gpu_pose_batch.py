"""`mdx_score_poses` / `MdState.score_poses`: the ligand row of `energy_potential_between_mols` for a batch of alternative placements
of the ligand, against the fp64 oracle (`orc.between_mols` at each pose's full coordinate set).

Tolerance per row element - the one tests/test_gpu_between_mols.py::assert_matrix applies to the matrix:
|dM| <= 2e-6 |M| + 1e-6 G + 1e-3 + |M| 2^-23, G = the oracle's gross sum of |e_pair| over the same pairs.

Poses: rigid moves of the ligand about its centroid (rotation by 0.3 u^3 rad about a random axis, translation by 3 u^3 A in a random
direction, u uniform in [0, 1): bounded by 0.3 rad / 3 A, most of them small as the moves of a local pose search are - the ligand sits
in water at liquid density, where a uniform draw up to 3 A clashes nearly every time), pose 0 = the start.  A pose that puts a ligand atom closer than 1.0 A to an atom of the
environment leaves the tolerance meaningless (r^-12 of a clash) and is dropped; at most 2 of 16 may be dropped, and the seeds below
were chosen on the CPU (tests/test_pose_batch_host.py re-checks them without a GPU)."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, systems

pytestmark = pytest.mark.gpu

SEED_SMALL, SEED_FLEX, SEED_50K = 8, 11, 2
MAX_DROPPED = 2
SAMPLED_50K = (0, 41, 97, 150, 203, 255)


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def three_groups(s):
    """receptor (molecule 0) / ligand (molecule 1) / solvent (the rest)"""
    ms = np.asarray(s.mol_start, dtype=np.int64)
    g = np.full(s.n_atoms, 2, np.uint8)
    g[:ms[1]] = 0
    g[ms[1]:ms[2]] = 1
    return g


def ligand_range(s):
    return int(s.mol_start[1]), int(s.mol_start[2])


def rigid_poses(lig, n, seed, max_rot=0.3, max_tr=3.0, jitter=0.0, power=3):
    """n placements of `lig` [count, 3]: pose 0 is the start; jitter: per-atom Gaussian noise (A rms per coordinate) on top."""
    rng = np.random.default_rng(seed)
    lig = np.asarray(lig, np.float64)
    c = lig.mean(0)
    out = np.empty((n,) + lig.shape, np.float64)
    for k in range(n):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = max_rot * rng.random() ** power
        kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        rot = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        out[k] = (lig - c) @ rot.T + c + d * max_tr * rng.random() ** power
        if jitter:
            out[k] += rng.normal(0, jitter, lig.shape)
    if not jitter:
        out[0] = lig
    return out.astype(np.float32)


def whole(s, lig):
    """The ligand as one piece: the handle wraps atom by atom, which may leave it on both sides of a box face."""
    lig = np.asarray(lig, np.float64)
    if not s.periodic:
        return lig
    box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    return lig - np.round((lig - lig[0]) / box) * box


def min_env_distance(s, pos, lo, hi, poses):
    """Closest ligand - environment distance of every pose (minimum image), fp64 on the CPU."""
    pos = np.asarray(pos, np.float64)
    env = np.concatenate([pos[:lo], pos[hi:]])
    if env.shape[0] == 0:
        return np.full(len(poses), np.inf)
    box = (np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)) if s.periodic else None
    out = []
    for p in np.asarray(poses, np.float64):
        m = np.inf
        for a in p:
            d = env - a
            if box is not None:
                d -= np.round(d / box) * box
            m = min(m, float((d * d).sum(1).min()))
        out.append(np.sqrt(m))
    return np.asarray(out)


def usable(s, pos, lo, hi, poses, cap=MAX_DROPPED):
    keep = min_env_distance(s, pos, lo, hi, poses) >= 1.0
    assert (~keep).sum() <= cap, f"{(~keep).sum()} poses clash with the environment (< 1.0 A): choose another seed"
    return keep


def oracle_row(orc, s, cfg, g, n, pos, lo, hi, pose, lig_group, use_cells=True):
    x = np.asarray(pos, np.float64).copy()
    x[lo:hi] = np.asarray(pose, np.float64)
    mo, gr = orc.between_mols(s, cfg, g, n, pos=x, use_cells=use_cells)
    return mo[lig_group], gr[lig_group]


def assert_row(row, ro, gross, what):
    row = np.asarray(row, np.float64)
    tol = 2e-6 * np.abs(ro) + 1e-6 * gross + 1e-3 + np.abs(ro) * 2.0 ** -23
    ratio = np.abs(row - ro) / tol
    k = int(np.argmax(ratio))
    print(f"{what}: gpu {row} oracle {ro} worst {ratio[k]:.3f}x tolerance")
    assert ratio[k] <= 1.0, f"{what}: element {k} gpu {row[k]!r} oracle {ro[k]!r}: {ratio[k]:.2f}x its tolerance {tol[k]:.2e}"


def small_configs():
    cfgs = (MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5),
            MdConfig(lj_cutoff=9.0, coulomb_cutoff=8.0, skin=1.5, coulomb_mode=1),                       # reaction field, two cutoffs
            MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=2, ewald_alpha=0.35))     # erfc real space (+ SPME)
    cfgs[2].overrides = 0
    return cfgs


def test_rows_match_the_oracle_on_the_small_complex(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    for cfg in small_configs():
        with mdx.MdState(s, cfg) as md:
            assert md.set_energy_groups(g, 3) == 3
            pos = md.positions()
            poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
            keep = usable(s, pos, lo, hi, poses)
            rows = md.score_poses(lo, poses)
            assert rows.shape == (16, 3) and rows.dtype == np.float32
            for k in np.flatnonzero(keep):
                ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[k], 1)
                assert_row(rows[k], ro, gr, f"small complex, coulomb mode {cfg.coulomb_mode}, pose {k}")
            assert abs(rows[0, 0]) > 1e-3 and abs(rows[0, 2]) > 1e-3      # the ligand sees receptor and water at the start
            # pose 0 is the resident placement: the row of the matrix itself
            m = md.energy_between_mols().astype(np.float64)
            ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[0], 1)
            assert np.all(np.abs(rows[0] - m[1]) <= 2e-6 * np.abs(m[1]) + 1e-6 * gr)


def test_flexible_poses_change_the_diagonal(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_FLEX, jitter=0.05)
        keep = usable(s, pos, lo, hi, poses)
        rows = md.score_poses(lo, poses)
        diag = []
        for k in np.flatnonzero(keep):
            ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[k], 1)
            assert_row(rows[k], ro, gr, f"flexible pose {k}")
            diag.append(ro[1])
        assert np.ptp(diag) > 1e-2 and len(set(rows[keep, 1].tolist())) > 1, "the intra-ligand element must move with the conformer"


def test_batch_agrees_with_upload_and_matrix_on_a_twin(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[1]
    with mdx.MdState(s, cfg) as md, mdx.MdState(s, cfg) as twin:
        md.set_energy_groups(g, 3)
        twin.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        keep = np.flatnonzero(usable(s, pos, lo, hi, poses))[:8]
        rows = md.score_poses(lo, poses).astype(np.float64)
        for k in keep:
            twin.set_positions_range(lo, poses[k])
            m = twin.energy_between_mols().astype(np.float64)
            _, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[k], 1)
            tol = 2e-6 * np.abs(m[1]) + 1e-6 * gr
            print(f"twin pose {k}: batch {rows[k]} loop {m[1]} tol {tol}")
            assert np.all(np.abs(rows[k] - m[1]) <= tol), (k, rows[k], m[1], tol)


def test_stale_structure_after_a_burst_of_steps(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        md.step(0.0005, None, 12)      # the inner list is in use; the cluster boxes are 12 steps old
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        keep = usable(s, pos, lo, hi, poses)
        rows = md.score_poses(lo, poses)
        for k in np.flatnonzero(keep):
            ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[k], 1)
            assert_row(rows[k], ro, gr, f"after 12 steps, pose {k}")


def test_periodic_images(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    box = np.asarray(s.box_hi, np.float32) - np.asarray(s.box_lo, np.float32)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        base = whole(s, pos[lo:hi]).astype(np.float32)
        ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, base, 1)
        shifted = np.stack([base, base + box * np.array([1, 0, 0], np.float32), base - box * np.array([0, 2, 1], np.float32)])
        rows = md.score_poses(lo, shifted.astype(np.float32))
        for k in range(3):
            assert_row(rows[k], ro, gr, f"pose translated by a box vector ({k})")
    # poses straddling a box face: the whole system is shifted so that the ligand's centroid lies on the face x = box_hi; the handle
    # wraps atom by atom, the poses are placements of the UNWRAPPED ligand (atoms on both sides of the face)
    s2 = systems.small_complex()
    p2 = np.asarray(s2.pos, np.float32).copy()
    p2[:, 0] += np.float32(s2.box_hi[0]) - p2[lo:hi, 0].mean()
    s2.pos = p2
    with mdx.MdState(s2, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(p2[lo:hi], 16, SEED_SMALL)
        assert (poses[0][:, 0] > s2.box_hi[0]).any() and (poses[0][:, 0] < s2.box_hi[0]).any()
        keep = usable(s2, pos, lo, hi, poses)
        rows = md.score_poses(lo, poses)
        for k in np.flatnonzero(keep):
            ro_f, gr_f = oracle_row(orc, s2, cfg, g, 3, pos, lo, hi, poses[k], 1)
            assert_row(rows[k], ro_f, gr_f, f"pose {k} straddling the face x = box_hi")
        assert abs(rows[0, 0]) > 1e-3 and abs(rows[0, 2]) > 1e-3


def test_a_pose_far_from_everything(mdx, orc):
    """Non-periodic: the ligand 500 A away sees nothing; the diagonal is its own energy."""
    s = systems.small_complex()
    s.periodic = False
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        far = (pos[lo:hi] + np.array([500.0, -300.0, 250.0], np.float32)).astype(np.float32)
        rows = md.score_poses(lo, np.stack([pos[lo:hi], far]))
        ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, far, 1, use_cells=False)
        assert rows[1, 0] == 0.0 and rows[1, 2] == 0.0 and ro[0] == 0.0 and ro[2] == 0.0
        assert_row(rows[1], ro, gr, "far pose")
        ro0, gr0 = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, pos[lo:hi], 1, use_cells=False)
        assert_row(rows[0], ro0, gr0, "non-periodic start pose")
        assert abs(rows[1, 1]) > 1e-3


def test_vacuum_ligand_is_one_group(mdx, orc):
    s = systems.lig50()
    cfg = MdConfig(lj_cutoff=0, coulomb_cutoff=0)
    g = np.zeros(s.n_atoms, np.uint8)
    with mdx.MdState(s, cfg) as md:
        assert md.set_energy_groups(g, 1) == 1
        pos = md.positions()
        poses = rigid_poses(pos, 16, SEED_FLEX, jitter=0.05)
        rows = md.score_poses(0, poses)
        assert rows.shape == (16, 1)
        for k in range(16):
            mo, gr = orc.between_mols(s, cfg, g, 1, pos=poses[k].astype(np.float64))
            assert_row(rows[k], mo[0], gr[0], f"lig50 in vacuum, pose {k}")
        assert len(set(rows[:, 0].tolist())) > 1


def test_config3_at_size_and_bitwise_reproducibility(mdx, orc):
    s = systems.complex50k()
    cfg = MdConfig()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 256, SEED_50K)
        sample = np.asarray(SAMPLED_50K)
        keep = usable(s, pos, lo, hi, poses[sample], cap=2)
        rows = md.score_poses(lo, poses)
        for k in sample[keep]:
            ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[k], 1)
            assert_row(rows[k], ro, gr, f"complex50k pose {k}")
        assert abs(rows[0, 0]) > 0.1 and abs(rows[0, 2]) > 0.1
        again = md.score_poses(lo, poses)
        assert np.array_equal(rows.view(np.uint32), again.view(np.uint32)), "the same call twice"
        perm = np.random.default_rng(5).permutation(256)
        shuffled = md.score_poses(lo, np.ascontiguousarray(poses[perm]))
        assert np.array_equal(shuffled.view(np.uint32), rows[perm].view(np.uint32)), "permuting the batch permutes the rows"
        for k in (0, 77, 255):
            alone = md.score_poses(lo, np.ascontiguousarray(poses[k:k + 1]))
            assert np.array_equal(alone.view(np.uint32), rows[k:k + 1].view(np.uint32)), f"pose {k} alone"


def test_the_handle_is_untouched(mdx):
    """nb_variant 2, the deterministic pair kernel: every energy the pair, bonded and 1-4 passes produce, the positions and the forces
    are bit-identical before and after a score_poses call, and 10 further steps land on the bits of a twin that never scored.
    `kinetic`, `temperature` and `pressure` (which holds the kinetic energy) are the entries of energy() that are NOT a function of the state alone on this engine:
    kinetic_kernel adds its per-block fp64 sums with atomics, so two energy() calls on an untouched handle already differ in the last
    bit (measured on an MI355X: 7234.968642024269 against 7234.968642024268 kcal/mol, temperature 912.8188129786108 against ...107).
    For those the test demands what they are made of - the velocities - bit for bit, and the sums to 1e-13 relative."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)      # the deterministic pair kernel
    with mdx.MdState(s, cfg) as md, mdx.MdState(s, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(g, 3)
            m.step(0.0005, None, 4)
        e0, x0, f0, v0 = md.energy(), md.positions(), md.forces(), md.velocities()
        rebuilds = md.stats()["rebuild_count"]
        poses = rigid_poses(whole(s, x0[lo:hi]), 16, SEED_SMALL)
        md.score_poses(lo, poses)
        assert md.stats()["rebuild_count"] == rebuilds, "scoring must not rebuild the list of a ready handle"
        e1, x1, f1, v1 = md.energy(), md.positions(), md.forces(), md.velocities()
        atomic_sums = ("kinetic", "temperature", "pressure")      # (the pressure holds the kinetic energy)
        print("energy() before", e0, "after", e1)
        for k in e0:
            if k in atomic_sums:
                assert e1[k] == pytest.approx(e0[k], rel=1e-13), k
            else:
                assert e0[k] == e1[k], (k, e0[k], e1[k])
        assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
        assert np.array_equal(x0.view(np.uint32), x1.view(np.uint32)) and np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
        twin.energy(), twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        assert np.array_equal(md.positions().view(np.uint32), twin.positions().view(np.uint32))
        assert np.array_equal(md.velocities().view(np.uint32), twin.velocities().view(np.uint32))
        assert md.stats()["rebuild_count"] == twin.stats()["rebuild_count"]


def _refused(mdx, md, first, count, poses, n_groups, match):
    lib = mdx.load_library()
    fp = C.POINTER(C.c_float)
    p = np.ascontiguousarray(poses, np.float32)
    out = np.full((p.shape[0], max(n_groups, 1)), -7.0, np.float32)
    rc = lib.mdx_score_poses(md._h, first, count, p.shape[0], p.ctypes.data_as(fp), out.ctypes.data_as(fp), n_groups)
    msg = lib.mdx_last_error().decode()
    assert rc == -1, (rc, msg)
    assert (out == -7.0).all(), "a refused call must leave out untouched"
    assert match in msg, msg


def test_refusals(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    n = hi - lo
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        pos = md.positions()
        poses = np.stack([pos[lo:hi]] * 2)
        _refused(mdx, md, lo, n, poses, 3, "no energy groups")
        md.set_energy_groups(g, 3)
        assert md.score_poses(lo, poses).shape == (2, 3)
        _refused(mdx, md, lo, n, poses, 2, "n_groups")
        _refused(mdx, md, lo - 1, n + 1, np.stack([pos[lo - 1:hi]] * 2), 3, "exactly one energy group")      # a receptor atom in the range
        _refused(mdx, md, lo, 0, np.zeros((2, 1, 3), np.float32), 3, "count")
        _refused(mdx, md, 0, 257, np.zeros((1, 257, 3), np.float32), 3, "count")
        _refused(mdx, md, s.n_atoms - 10, n, poses, 3, "out of bounds")
        bad = poses.copy()
        bad[1, 7, 2] = np.nan
        _refused(mdx, md, lo, n, bad, 3, "non-finite")
        bad[1, 7, 2] = np.inf
        _refused(mdx, md, lo, n, bad, 3, "non-finite")
        # half of the ligand as a group of its own: bonds, exclusions and 1-4 pairs cross the range
        g4 = g.copy()
        g4[lo + n // 2:hi] = 3
        md.set_energy_groups(g4, 4)
        _refused(mdx, md, lo, n // 2, poses[:, :n // 2], 4, "links the range")
        md.set_energy_groups(g, 3)
        # n_poses == 0 succeeds and does nothing
        out = np.full(3, -7.0, np.float32)
        fp = C.POINTER(C.c_float)
        assert mdx.load_library().mdx_score_poses(md._h, lo, n, 0, None, out.ctypes.data_as(fp), 3) == 0 and (out == -7.0).all()
        # an alchemical window
        md.configure_alchemical_window(1, 0.5)      # the ligand is molecule 1
        _refused(mdx, md, lo, n, poses, 3, "alchemical")


def test_refused_on_a_decomposed_handle(mdx):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    g = three_groups(s)
    lo, hi = ligand_range(s)
    poses = np.stack([np.asarray(s.pos, np.float32)[lo:hi]] * 2)
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
                    _refused(mdx, md, lo, hi - lo, poses, 3, "decomposed")
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]
