"""`mdx_pose_forces` / `MdState.pose_forces`: per-atom forces, net force and torque of a batch of ligand placements against the fp64
oracle (tests/pose_force_ref.py: the oracle's non-bonded forces at each pose's full coordinate set, pinned on the CPU by
tests/test_pose_forces_host.py as minus the gradient of the sum of the oracle's ligand row - never the library's own energies).

Per atom |dF_i| <= 1e-4 max(|F_i|, 1) + slack_i; net force |dF_net| <= sum_i tol_i; torque |d tau| <= sum_i |x_i - c| tol_i.
Poses with a ligand atom within 1.0 A of the environment are dropped (at most 2 of 16); at most 2 % of the compared rows may carry
slack.  Every comparison prints its worst fraction of the tolerance.

Measured on an MI355X: see DESIGN.md section 7d for the worst fractions."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, systems
from tests import pose_force_ref as R
from tests.test_gpu_pose_batch import SEED_FLEX, SEED_SMALL, ligand_range, rigid_poses, small_configs, three_groups, usable, whole

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare(orc, s, cfg, pos, lo, hi, poses, keep, forces, rigid, what, use_cells=True, ref_poses=None):
    """Forces and rigid of the kept poses against the oracle (at ref_poses[k] where given: a pose that is an image of it).
    -> (worst per-atom ratio, worst rigid ratio, largest oracle force); asserts the bounds and the slack cap."""
    worst = worst_rigid = fmax = 0.0
    rows = slacked = 0
    for k in np.flatnonzero(keep):
        ref = poses[k] if ref_poses is None else ref_poses[k]
        fo, tol, slack = R.reference(orc, s, cfg, pos, lo, hi, ref, use_cells=use_cells)
        rows += slack.size
        slacked += int((slack > 0).sum())
        ratio = np.linalg.norm(forces[k].astype(np.float64) - fo, axis=1) / tol
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1.0, (f"{what}, pose {k}, atom {i}: gpu {forces[k][i]!r} oracle {fo[i]!r}: {ratio[i]:.2f}x its tolerance "
                                 f"{tol[i]:.2e} (slack {slack[i]:.1e})")
        worst = max(worst, float(ratio[i]))
        fmax = max(fmax, float(np.abs(fo).max()))
        if rigid is not None:
            ro = R.rigid_of(ref, fo)
            tf, tt = R.rigid_tolerance(ref, tol)
            rf = np.linalg.norm(rigid[k, :3] - ro[:3]) / tf
            rt = np.linalg.norm(rigid[k, 3:] - ro[3:]) / tt
            assert rf <= 1.0 and rt <= 1.0, f"{what}, pose {k}: net force {rigid[k, :3]} oracle {ro[:3]} ({rf:.2f}x), torque {rigid[k, 3:]} oracle {ro[3:]} ({rt:.2f}x)"
            worst_rigid = max(worst_rigid, float(rf), float(rt))
    print(f"{what}: {int(np.count_nonzero(keep))} poses, worst |dF_i| {worst:.3f}x tolerance, worst rigid {worst_rigid:.3f}x, "
          f"{slacked} of {rows} rows with slack, largest |F| component {fmax:.1f}")
    assert slacked <= R.MAX_SLACK_ROWS * rows, f"{what}: {slacked} of {rows} compared rows carry slack"
    return worst, worst_rigid, fmax


def test_forces_match_the_oracle_on_the_small_complex(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    for cfg in small_configs():
        with mdx.MdState(s, cfg) as md:
            md.set_energy_groups(g, 3)
            pos = md.positions()
            poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)      # pose 0 is the resident placement
            keep = usable(s, pos, lo, hi, poses)
            f, rigid = md.pose_forces(lo, poses, rows=False, rigid=True)
            assert f.shape == (16, hi - lo, 3) and f.dtype == np.float32 and rigid.shape == (16, 6) and rigid.dtype == np.float32
            _, _, fmax = compare(orc, s, cfg, pos, lo, hi, poses, keep, f, rigid, f"small complex, coulomb mode {cfg.coulomb_mode}")
            assert fmax > 1.0 and np.abs(f[keep]).max() > 1.0


def test_softened_coulomb(mdx, orc):
    """softening_sq != 0 selects the softened-Coulomb instantiation.  Its force is the engine's (and the oracle's) softened one while the
    row's energy is not softened (mdx.h says so); at the reference's 1e-6 A^2 the two differ by 1e-6 / r^2 relative, far inside the
    bound.  Cutoffs, poses and so the two caps are those of small_configs()[0]."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, softening_sq=1e-6)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        keep = usable(s, pos, lo, hi, poses)
        f, rows, rigid = md.pose_forces(lo, poses, rows=True, rigid=True)
        _, _, fmax = compare(orc, s, cfg, pos, lo, hi, poses, keep, f, rigid, "softened coulomb")
        assert fmax > 1.0
        assert np.array_equal(bits(rows), bits(md.score_poses(lo, poses)))


def test_flexible_poses(mdx, orc):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_FLEX, jitter=0.05)
        keep = usable(s, pos, lo, hi, poses)
        f, rigid = md.pose_forces(lo, poses, rows=False, rigid=True)
        compare(orc, s, cfg, pos, lo, hi, poses, keep, f, rigid, "flexible poses")


def test_rows_are_the_bits_of_score_poses(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    for cfg in small_configs():
        with mdx.MdState(s, cfg) as md:
            md.set_energy_groups(g, 3)
            pos = md.positions()
            poses = np.concatenate([rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL),
                                    rigid_poses(whole(s, pos[lo:hi]), 16, SEED_FLEX, jitter=0.05)])
            rows = md.score_poses(lo, poses)
            _, frows = md.pose_forces(lo, poses)
            assert frows.shape == rows.shape and frows.dtype == np.float32
            assert np.array_equal(bits(frows), bits(rows)), f"coulomb mode {cfg.coulomb_mode}: {frows - rows}"
            assert np.array_equal(bits(md.score_poses(lo, poses)), bits(rows))


def test_aged_structure_after_a_burst_of_steps(mdx, orc):
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
        f, rigid = md.pose_forces(lo, poses, rows=False, rigid=True)
        compare(orc, s, cfg, pos, lo, hi, poses, keep, f, rigid, "after 12 steps")


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
        shifted = np.stack([base, base + box * np.array([1, 0, 0], np.float32), base - box * np.array([0, 2, 1], np.float32)])
        f, rigid = md.pose_forces(lo, shifted, rows=False, rigid=True)
        compare(orc, s, cfg, pos, lo, hi, shifted, np.ones(3, bool), f, rigid, "pose translated by box vectors",
                ref_poses=np.stack([base] * 3))
    # poses straddling a box face: the system is shifted so that the ligand's centroid lies on the face x = box_hi; the handle wraps atom
    # by atom, the poses are placements of the UNWRAPPED ligand
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
        f, rigid = md.pose_forces(lo, poses, rows=False, rigid=True)
        _, _, fmax = compare(orc, s2, cfg, pos, lo, hi, poses, keep, f, rigid, "poses straddling the face x = box_hi")
        assert fmax > 1.0


def test_a_pose_far_from_everything(mdx, orc):
    """Non-periodic: the ligand 500 A away feels its own atoms only - the net force is Newton's third law inside the ligand unit."""
    s = systems.small_complex()
    s.periodic = False
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        far = (pos[lo:hi] + np.array([500.0, -300.0, 250.0], np.float32)).astype(np.float32)
        poses = np.stack([pos[lo:hi], far])
        f, rigid = md.pose_forces(lo, poses, rows=False, rigid=True)
        compare(orc, s, cfg, pos, lo, hi, poses, np.ones(2, bool), f, rigid, "non-periodic: start and far pose", use_cells=False)
        fo, tol, _ = R.reference(orc, s, cfg, pos, lo, hi, far, use_cells=False)
        s_alone = np.linalg.norm(rigid[1, :3]) / tol.sum()
        print(f"far pose: |F_net| {np.linalg.norm(rigid[1, :3]):.2e} = {s_alone:.3f}x sum tol; oracle |F_net| {np.linalg.norm(fo.sum(0)):.1e}")
        assert s_alone <= 1.0 and np.abs(f[1]).max() > 1e-3


def test_vacuum_ligand_is_one_group(mdx, orc):
    s = systems.lig50()
    cfg = MdConfig(lj_cutoff=0, coulomb_cutoff=0)
    g = np.zeros(s.n_atoms, np.uint8)
    with mdx.MdState(s, cfg) as md:
        assert md.set_energy_groups(g, 1) == 1
        pos = md.positions()
        poses = rigid_poses(pos, 16, SEED_FLEX, jitter=0.05)
        f, rows, rigid = md.pose_forces(0, poses, rigid=True)
        assert rows.shape == (16, 1)
        compare(orc, s, cfg, pos, 0, s.n_atoms, poses, np.ones(16, bool), f, rigid, "lig50 in vacuum", use_cells=False)
        for k in range(16):
            _, tol, _ = R.reference(orc, s, cfg, pos, 0, s.n_atoms, poses[k], use_cells=False)
            tf, tt = R.rigid_tolerance(poses[k], tol)
            assert np.linalg.norm(rigid[k, :3]) <= tf and np.linalg.norm(rigid[k, 3:]) <= tt, (k, rigid[k], tf, tt)
        assert np.abs(f).max() > 1.0


def test_ranges_beyond_one_wave_and_below_one_strip(mdx, orc):
    """The chain (120 atoms: 15 strips, two staging waves) and one water (3 atoms, a group of its own) as the range."""
    s = systems.small_complex()
    cfg = small_configs()[0]
    ms = s.mol_start
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(three_groups(s), 3)
        pos = md.positions()
        lo, hi = 0, int(ms[1])
        poses = R.chain_poses(whole(s, pos[lo:hi]))
        keep = usable(s, pos, lo, hi, poses)
        f, rows, rigid = md.pose_forces(lo, poses, rigid=True)
        assert np.array_equal(bits(rows), bits(md.score_poses(lo, poses)))
        _, _, fmax = compare(orc, s, cfg, pos, lo, hi, poses, keep, f, rigid, "the chain as the range")
        assert fmax > 1.0
        md.set_energy_groups(R.four_groups(s), 4)
        lo, hi = int(ms[2]), int(ms[3])
        assert hi - lo == 3
        poses = R.water_poses(whole(s, pos[lo:hi]))
        keep = usable(s, pos, lo, hi, poses)
        f, rows, rigid = md.pose_forces(lo, poses, rigid=True)
        assert np.array_equal(bits(rows), bits(md.score_poses(lo, poses)))
        _, _, fmax = compare(orc, s, cfg, pos, lo, hi, poses, keep, f, rigid, "one water as the range")
        assert fmax > 1.0


def test_bitwise_behaviour(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 64, SEED_SMALL)
        f, rows, rigid = md.pose_forces(lo, poses, rigid=True)
        assert np.abs(f).max() > 1.0
        again = md.pose_forces(lo, poses, rigid=True)
        for a, b, what in zip((f, rows, rigid), again, ("forces", "rows", "rigid")):
            assert np.array_equal(bits(a), bits(b)), f"the same call twice: {what}"
        perm = np.random.default_rng(5).permutation(64)
        shuffled = md.pose_forces(lo, np.ascontiguousarray(poses[perm]), rigid=True)
        for a, b, what in zip((f, rows, rigid), shuffled, ("forces", "rows", "rigid")):
            assert np.array_equal(bits(a[perm]), bits(b)), f"permuting the batch permutes the {what}"
        for k in (0, 31, 63):
            alone = md.pose_forces(lo, np.ascontiguousarray(poses[k:k + 1]), rigid=True)
            for a, b, what in zip((f, rows, rigid), alone, ("forces", "rows", "rigid")):
                assert np.array_equal(bits(a[k:k + 1]), bits(b)), f"pose {k} alone: {what}"
        assert np.array_equal(bits(md.pose_forces(lo, poses, rows=True, rigid=None)[0]), bits(f)), "rigid=None changes forces"
        assert np.array_equal(bits(md.pose_forces(lo, poses, rows=None, rigid=True)[0]), bits(f)), "rows=None changes forces"
        only = md.pose_forces(lo, poses, rows=None, rigid=None)
        assert len(only) == 1 and np.array_equal(bits(only[0]), bits(f))


def test_the_handle_is_untouched(mdx):
    """The twin test of tests/test_gpu_pose_batch.py::test_the_handle_is_untouched with pose_forces in place of score_poses: nb_variant 2,
    the deterministic pair kernel; `kinetic`, `temperature` and `pressure` are sums taken with atomics and get 1e-13 relative, their
    ingredients - the velocities - bit for bit (see there)."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)
    with mdx.MdState(s, cfg) as md, mdx.MdState(s, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(g, 3)
            m.step(0.0005, None, 4)
        e0, x0, f0, v0 = md.energy(), md.positions(), md.forces(), md.velocities()
        rebuilds = md.stats()["rebuild_count"]
        poses = rigid_poses(whole(s, x0[lo:hi]), 16, SEED_SMALL)
        md.pose_forces(lo, poses, rigid=True)
        assert md.stats()["rebuild_count"] == rebuilds, "pose forces must not rebuild the list of a ready handle"
        e1, x1, f1, v1 = md.energy(), md.positions(), md.forces(), md.velocities()
        atomic_sums = ("kinetic", "temperature", "pressure")
        for k in e0:
            if k in atomic_sums:
                assert e1[k] == pytest.approx(e0[k], rel=1e-13), k
            else:
                assert e0[k] == e1[k], (k, e0[k], e1[k])
        assert np.array_equal(bits(v0), bits(v1))
        assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1))
        twin.energy(), twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        assert np.array_equal(bits(md.positions()), bits(twin.positions()))
        assert np.array_equal(bits(md.velocities()), bits(twin.velocities()))
        assert md.stats()["rebuild_count"] == twin.stats()["rebuild_count"]


def _refused(mdx, md, first, count, poses, n_groups, match, no_forces=False):
    lib = mdx.load_library()
    fp = C.POINTER(C.c_float)
    p = np.ascontiguousarray(poses, np.float32)
    rows = np.full((p.shape[0], max(n_groups, 1)), -7.0, np.float32)
    f = np.full((p.shape[0], max(p.shape[1], 1), 3), -7.0, np.float32)
    rigid = np.full((p.shape[0], 6), -7.0, np.float32)
    rc = lib.mdx_pose_forces(md._h, first, count, p.shape[0], p.ctypes.data_as(fp), rows.ctypes.data_as(fp), n_groups,
                             None if no_forces else f.ctypes.data_as(fp), rigid.ctypes.data_as(fp))
    msg = lib.mdx_last_error().decode()
    assert rc == -1, (rc, msg)
    assert (rows == -7.0).all() and (f == -7.0).all() and (rigid == -7.0).all(), "a refused call must leave its outputs untouched"
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
        assert md.pose_forces(lo, poses)[0].shape == (2, n, 3)
        _refused(mdx, md, lo, n, poses, 3, "null", no_forces=True)
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
        out = np.full(18, -7.0, np.float32)
        fp = C.POINTER(C.c_float)
        o = out.ctypes.data_as(fp)
        assert mdx.load_library().mdx_pose_forces(md._h, lo, n, 0, None, o, 3, o, o) == 0 and (out == -7.0).all()
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
