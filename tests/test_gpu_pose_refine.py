"""`mdx_refine_poses` / `MdState.refine_poses`: the device loop against the host loop it replaces (`MdState.pose_forces` + the numpy
stepper of tests/pose_refine_ref.py), against itself (rows and rigid are the bits `score_poses` / `pose_forces` return for the refined
pose), and against the fp64 oracle (tests/pose_force_ref.py, `oracle_row`).

Device loop against host loop: status and evaluation count equal for every pose, coordinates within 4 ulp32(max |coordinate|) - the
only admissible difference is an fp64 rounding (sin / cos / sqrt of the two maths libraries) that tips one fp32 rounding.  16 poses
on small_complex, at most 64 evaluations unless a test says otherwise.

Measured on an MI355X: see DESIGN.md section 7e."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, _abi, systems
from tests import pose_force_ref as R
from tests import pose_refine_ref as P
from tests.test_gpu_pose_batch import (SEED_FLEX, SEED_SMALL, assert_row, ligand_range, oracle_row, rigid_poses, small_configs, three_groups,
                                       usable, whole)
from tests.test_pose_refine_host import CRYSTAL_F_TOL, CRYSTAL_MAX_EVALS, CRYSTAL_TAU_TOL, crystal_case, crystal_poses

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def same_bits(a, b, what):
    for x, y, name in zip(a, b, ("poses", "rows", "rigid", "xform", "status", "evals")):
        assert np.array_equal(bits(x), bits(y)), f"{what}: {name} differ"


def against_the_host_loop(md, lo, poses, what, max_evals, f_tol=0.0, tau_tol=0.0, h_start=0.0, h_max=0.0):
    """Device loop and host loop on the same poses -> the device loop's outputs; asserts what the module's docstring states."""
    dev = md.refine_poses(lo, poses, max_evals, f_tol, tau_tol, h_start, h_max)
    n_groups = dev[1].shape[1]
    host = P.refine_batch(poses, P.host_evaluate(md, lo, n_groups), max_evals, f_tol, tau_tol, h_start, h_max)
    assert np.array_equal(dev[4], host[4]), f"{what}: status device {dev[4].tolist()} host {host[4].tolist()}"
    assert np.array_equal(dev[5], host[5]), f"{what}: evaluations device {dev[5].tolist()} host {host[5].tolist()}"
    differ = int((bits(dev[0]) != bits(host[0])).sum())
    worst = float(np.abs(dev[0].astype(np.float64) - host[0].astype(np.float64)).max()) / ulp32(host[0])
    print(f"{what}: status {dev[4].tolist()}, evaluations {dev[5].tolist()}; {differ} of {dev[0].size} coordinates not bit-equal to the "
          f"host loop's, worst difference {worst:.2f} ulp32(max |coordinate|)")
    assert worst <= 4.0, f"{what}: a coordinate differs from the host loop's by {worst:.1f} ulp32"
    assert np.abs(dev[3] - host[3]).max() <= 1e-5, f"{what}: xform {np.abs(dev[3] - host[3]).max()}"
    return dev


def self_consistent(md, lo, dev, what):
    """rows_out / rigid_out are the bits score_poses / pose_forces return for poses_out (finite poses only: pose_forces refuses the others)"""
    ok = dev[4] != P.NONFINITE
    y = np.ascontiguousarray(dev[0][ok])
    assert np.array_equal(bits(dev[1][ok]), bits(md.score_poses(lo, y))), f"{what}: rows_out is not score_poses(poses_out)"
    assert np.array_equal(bits(dev[2][ok]), bits(md.pose_forces(lo, y, rows=False, rigid=True)[1])), f"{what}: rigid_out is not that of pose_forces(poses_out)"


def test_equals_the_host_loop(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    for cfg in small_configs():
        with mdx.MdState(s, cfg) as md:
            md.set_energy_groups(g, 3)
            pos = md.positions()
            poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
            dev = against_the_host_loop(md, lo, poses, f"small complex, coulomb mode {cfg.coulomb_mode}", 12)
            assert dev[0].shape == poses.shape and dev[0].dtype == np.float32 and dev[1].shape == (16, 3) and dev[2].shape == (16, 6)
            assert dev[3].shape == (16, 7) and dev[4].dtype == np.uint32 and dev[5].dtype == np.uint32
            assert (dev[5] == 12).all() and (dev[4] == P.MAX_EVALS).all()
            self_consistent(md, lo, dev, f"coulomb mode {cfg.coulomb_mode}")


def test_equals_the_host_loop_through_rejects(mdx):
    """h_start = h_max = 0.2 A overshoots soon, so the 48 evaluations hold rejects; with f_tol 2 kcal/mol/A and tau_tol 6 kcal/mol poses
    converge and stall at many different evaluation counts, so live and frozen poses share the batch for most of the run."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        dev = against_the_host_loop(md, lo, poses, "h_start = h_max = 0.2 A", 48, f_tol=2.0, tau_tol=6.0, h_start=0.2, h_max=0.2)
        assert (dev[5] >= 1).all() and (dev[5] <= 48).all() and len(set(dev[5].tolist())) > 4
        assert (dev[4] == P.CONVERGED).any() and (dev[4] == P.STALLED).any()
        self_consistent(md, lo, dev, "h_start = h_max = 0.2 A")


def test_one_evaluation_returns_the_input(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        y, rows, rigid, xform, status, evals = md.refine_poses(lo, poses, 1, 0.0, 0.0)
        assert np.array_equal(bits(y), bits(poses)) and (evals == 1).all() and (status == P.MAX_EVALS).all()
        assert np.array_equal(bits(rows), bits(md.score_poses(lo, poses)))
        assert np.array_equal(bits(rigid), bits(md.pose_forces(lo, poses, rows=False, rigid=True)[1]))
        assert np.array_equal(xform, np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), (16, 1)))


def test_descent_and_rigidity(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        y, rows, rigid, xform, status, evals = md.refine_poses(lo, poses, 48, 0.0, 0.0)
        before = md.score_poses(lo, poses).astype(np.float64).sum(1)
        after = rows.astype(np.float64).sum(1)
        print("decrease of the row sum, kcal/mol:", np.round(before - after, 3).tolist(), "evaluations", evals.tolist())
        assert (after <= before).all()
        assert ((evals > 1) & (after < before)).any()
        for k in range(16):
            a, b = poses[k].astype(np.float64), y[k].astype(np.float64)
            d0 = np.linalg.norm(a[:, None] - a[None], axis=2)
            d1 = np.linalg.norm(b[:, None] - b[None], axis=2)
            tol = 4 * max(ulp32(a), ulp32(b))
            assert np.abs(d1 - d0).max() <= tol, f"pose {k}: a pair distance changed by {np.abs(d1 - d0).max():.2e} A (bound {tol:.2e})"
            again = P.coords(P.mean(a), xform[k, 4:].astype(np.float64), xform[k, :4].astype(np.float64), poses[k])
            assert np.abs(again.astype(np.float64) - b).max() <= 1e-4, f"pose {k}: coords(xform) misses poses_out by {np.abs(again - b).max():.2e} A"
            assert abs(np.linalg.norm(xform[k, :4].astype(np.float64)) - 1.0) <= 1e-6


def test_against_the_oracle(mdx, orc):
    """The refined poses' rows against the oracle's rows at the same coordinates, and the oracle's own row sums before and after: the
    decrease the device reports is real."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    cfg = small_configs()[0]
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        y, rows, rigid, xform, status, evals = md.refine_poses(lo, poses, 12, 0.0, 0.0)
        keep = usable(s, pos, lo, hi, y)
        for k in np.flatnonzero(keep):
            ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, y[k], 1)
            assert_row(rows[k], ro, gr, f"refined pose {k}")
            r0, _ = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, poses[k], 1)
            print(f"pose {k}: oracle row sum {r0.sum():.3f} -> {ro.sum():.3f}")
            assert ro.sum() < r0.sum(), f"pose {k}: the oracle's row sum did not go down ({r0.sum()} -> {ro.sum()})"


def test_convergence_on_the_crystal(mdx, orc):
    """One molecule of the crystal as the range; f_tol, tau_tol and max_evals as chosen on the CPU (tests/test_pose_refine_host.py: all 16
    converge with the oracle-driven loop).  What the device calls converged is converged by the oracle's forces, within their bounds."""
    s, cfg, g, lo, hi = crystal_case()
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 2)
        pos = md.positions()
        poses = crystal_poses(whole(s, pos[lo:hi]))
        y, rows, rigid, xform, status, evals = md.refine_poses(lo, poses, CRYSTAL_MAX_EVALS, CRYSTAL_F_TOL, CRYSTAL_TAU_TOL)
        conv = status == P.CONVERGED
        print(f"{int(conv.sum())} of 16 converged; status {status.tolist()}, evaluations {evals.tolist()}")
        assert conv.sum() >= 1
        for k in np.flatnonzero(conv):
            fo, tol, _ = R.reference(orc, s, cfg, pos, lo, hi, y[k])
            ro = R.rigid_of(y[k], fo)
            tf, tt = R.rigid_tolerance(y[k], tol)
            fn, tn = np.linalg.norm(ro[:3]), np.linalg.norm(ro[3:])
            print(f"pose {k}: oracle |F_net| {fn:.3f} (bound {CRYSTAL_F_TOL + tf:.3f}), |tau| {tn:.3f} (bound {CRYSTAL_TAU_TOL + tt:.3f}), "
                  f"{evals[k]} evaluations")
            assert fn <= CRYSTAL_F_TOL + tf and tn <= CRYSTAL_TAU_TOL + tt
            assert np.linalg.norm(rigid[k, :3]) <= CRYSTAL_F_TOL and np.linalg.norm(rigid[k, 3:]) <= CRYSTAL_TAU_TOL
        self_consistent(md, lo, (y, rows, rigid, xform, status, evals), "crystal")


def test_ranges_beyond_one_wave_and_below_one_strip(mdx):
    """The chain (120 atoms: 15 strips, two staging waves) and one water (3 atoms, a group of its own) as the range."""
    s = systems.small_complex()
    ms = s.mol_start
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(three_groups(s), 3)
        pos = md.positions()
        lo, hi = 0, int(ms[1])
        dev = against_the_host_loop(md, lo, R.chain_poses(whole(s, pos[lo:hi])), "the chain as the range", 12)
        self_consistent(md, lo, dev, "the chain as the range")
        assert (dev[1].astype(np.float64).sum(1) <= md.score_poses(lo, R.chain_poses(whole(s, pos[lo:hi]))).astype(np.float64).sum(1)).all()
        md.set_energy_groups(R.four_groups(s), 4)
        lo, hi = int(ms[2]), int(ms[3])
        assert hi - lo == 3
        dev = against_the_host_loop(md, lo, R.water_poses(whole(s, pos[lo:hi])), "one water as the range", 12)
        self_consistent(md, lo, dev, "one water as the range")


def test_vacuum_ligand_is_converged_at_once(mdx, orc):
    """lig50 in vacuum as one group: net force and torque are internal, zero within the oracle-derived rigid tolerance - with the
    tolerances set from it every pose is CONVERGED after one evaluation and comes back bit for bit."""
    s = systems.lig50()
    cfg = MdConfig(lj_cutoff=0, coulomb_cutoff=0)
    with mdx.MdState(s, cfg) as md:
        assert md.set_energy_groups(np.zeros(s.n_atoms, np.uint8), 1) == 1
        pos = md.positions()
        poses = rigid_poses(pos, 16, SEED_FLEX, jitter=0.05)
        tf = tt = 0.0
        for k in range(16):
            _, tol, _ = R.reference(orc, s, cfg, pos, 0, s.n_atoms, poses[k], use_cells=False)
            a, b = R.rigid_tolerance(poses[k], tol)
            tf, tt = max(tf, a), max(tt, b)
        y, rows, rigid, xform, status, evals = md.refine_poses(0, poses, 8, tf, tt)
        print(f"f_tol {tf:.3e}, tau_tol {tt:.3e}; largest |F_net| {np.linalg.norm(rigid[:, :3], axis=1).max():.2e}, |tau| {np.linalg.norm(rigid[:, 3:], axis=1).max():.2e}")
        assert (status == P.CONVERGED).all() and (evals == 1).all()
        assert np.array_equal(bits(y), bits(poses)) and rows.shape == (16, 1)
        assert np.array_equal(bits(rows), bits(md.score_poses(0, poses)))


def test_poses_straddling_a_box_face(mdx):
    s2 = systems.small_complex()
    g = three_groups(s2)
    lo, hi = ligand_range(s2)
    p2 = np.asarray(s2.pos, np.float32).copy()
    p2[:, 0] += np.float32(s2.box_hi[0]) - p2[lo:hi, 0].mean()
    s2.pos = p2
    with mdx.MdState(s2, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        poses = rigid_poses(p2[lo:hi], 16, SEED_SMALL)
        assert (poses[0][:, 0] > s2.box_hi[0]).any() and (poses[0][:, 0] < s2.box_hi[0]).any()
        dev = against_the_host_loop(md, lo, poses, "poses straddling the face x = box_hi", 12)
        self_consistent(md, lo, dev, "poses straddling the face x = box_hi")
        assert (dev[1].astype(np.float64).sum(1) < md.score_poses(lo, poses).astype(np.float64).sum(1)).any()


def test_a_pose_far_from_everything(mdx):
    """Non-periodic: 500 A away the ligand feels its own atoms only; net force and torque are rounding noise, which the stepper scales
    to a full step all the same - whatever it makes of that, the host loop must make the same."""
    s = systems.small_complex()
    s.periodic = False
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        far = (pos[lo:hi] + np.array([500.0, -300.0, 250.0], np.float32)).astype(np.float32)
        dev = against_the_host_loop(md, lo, np.stack([pos[lo:hi], far]), "non-periodic: start and far pose", 24)
        self_consistent(md, lo, dev, "non-periodic")
        assert dev[1][1].astype(np.float64).sum() <= md.score_poses(lo, far[None]).astype(np.float64).sum()


def test_a_non_finite_start_is_a_status_of_its_pose(mdx):
    """Pose 5 has its first atom on top of an atom of the receptor: NONFINITE after one evaluation with its input returned, the other
    fifteen poses bit for bit what they are without it."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
        clean = md.refine_poses(lo, poses, 12, 0.0, 0.0)
        bad = poses.copy()
        bad[5, 0] = pos[3]
        with pytest.raises(mdx.BlowUpError):
            md.pose_forces(lo, np.ascontiguousarray(bad[5:6]))
        out = md.refine_poses(lo, bad, 12, 0.0, 0.0)
        assert out[4][5] == P.NONFINITE and out[5][5] == 1 and np.array_equal(bits(out[0][5]), bits(bad[5]))
        others = np.arange(16) != 5
        same_bits([o[others] for o in out], [c[others] for c in clean], "the rest of the batch")
        assert (out[4][others] == P.MAX_EVALS).all()
        host = P.refine_batch(bad[5:6], P.host_evaluate(md, lo, 3), 12, 0.0, 0.0)
        assert host[4][0] == P.NONFINITE and host[5][0] == 1


def _raw(mdx, md, lo, poses, opts, rows=True, rigid=True, xform=True, status=True, evals=True):
    """The C entry point itself, with any of the optional outputs left out -> (rc, poses_out, rows, rigid, xform, status, evals)"""
    lib = mdx.load_library()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    p = np.ascontiguousarray(poses, np.float32)
    n = p.shape[0]
    o = [np.full(p.shape, -7.0, np.float32), np.full((n, 3), -7.0, np.float32), np.full((n, 6), -7.0, np.float32),
         np.full((n, 7), -7.0, np.float32), np.full(n, 77, np.uint32), np.full(n, 77, np.uint32)]
    rc = lib.mdx_refine_poses(md._h, lo, p.shape[1], n, p.ctypes.data_as(fp), C.byref(opts), o[0].ctypes.data_as(fp),
                              o[1].ctypes.data_as(fp) if rows else None, 3, o[2].ctypes.data_as(fp) if rigid else None,
                              o[3].ctypes.data_as(fp) if xform else None, o[4].ctypes.data_as(up) if status else None,
                              o[5].ctypes.data_as(up) if evals else None)
    return (rc,) + tuple(o)


def test_bitwise_behaviour(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 64, SEED_SMALL)
        args = (16, 50.0, 200.0, 0.05, 0.2)      # (of these 64 starts 19 are below the tolerances, by the oracle, the nearest 0.6 % off)
        first = md.refine_poses(lo, poses, *args)
        assert len(set(first[5].tolist())) > 1 or len(set(first[4].tolist())) > 1, "the batch should hold poses that end differently"
        same_bits(first, md.refine_poses(lo, poses, *args), "the same call twice")
        perm = np.random.default_rng(5).permutation(64)
        same_bits([a[perm] for a in first], md.refine_poses(lo, np.ascontiguousarray(poses[perm]), *args), "permuting the batch")
        for k in (0, 31, 63):
            same_bits([a[k:k + 1] for a in first], md.refine_poses(lo, np.ascontiguousarray(poses[k:k + 1]), *args), f"pose {k} alone")
        opts = _abi.CRefineOpts(*args)
        rc, *full = _raw(mdx, md, lo, poses, opts)
        assert rc == 0
        same_bits(first, full, "the C entry point")
        rc, y, rows, rigid, xform, status, evals = _raw(mdx, md, lo, poses, opts, rows=False, rigid=False, xform=False, status=False, evals=False)
        assert rc == 0 and np.array_equal(bits(y), bits(first[0])), "leaving the optional outputs out changes poses_out"
        assert (rows == -7.0).all() and (rigid == -7.0).all() and (xform == -7.0).all() and (status == 77).all() and (evals == 77).all()
        rc, y, rows, rigid, xform, status, evals = _raw(mdx, md, lo, poses, opts, rows=False, xform=False)
        assert rc == 0
        same_bits((first[0], first[2], first[4], first[5]), (y, rigid, status, evals), "some optional outputs left out")


def test_a_batch_across_the_chunk_boundary(mdx):
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        poses = rigid_poses(whole(s, pos[lo:hi]), 300, SEED_SMALL)
        whole_batch = md.refine_poses(lo, poses, 8, 0.0, 0.0)
        a = md.refine_poses(lo, np.ascontiguousarray(poses[:170]), 8, 0.0, 0.0)
        b = md.refine_poses(lo, np.ascontiguousarray(poses[170:]), 8, 0.0, 0.0)
        same_bits(whole_batch, [np.concatenate([x, y]) for x, y in zip(a, b)], "300 poses in one call and in two")
        assert (whole_batch[5] == 8).all()
        assert (whole_batch[1].astype(np.float64).sum(1) <= md.score_poses(lo, poses).astype(np.float64).sum(1)).all()


def test_the_handle_is_untouched(mdx):
    """The twin test of tests/test_gpu_pose_forces.py::test_the_handle_is_untouched with refine_poses in place of pose_forces: nb_variant 2,
    the deterministic pair kernel; `kinetic`, `temperature` and `pressure` are sums taken with atomics and get 1e-13 relative, their
    ingredients - the velocities - bit for bit (see there).  So are the bonded sums: energy() adds them with one fp64 atomic per block,
    two calls on an unchanged handle can differ in the last bit (seen on an MI355X: `angle` 594.7974077505681 / 594.797407750568), and
    what they are sums of - positions and forces - is held bit for bit below."""
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
        md.refine_poses(lo, poses, 12, 0.0, 0.0)
        assert md.stats()["rebuild_count"] == rebuilds, "refining poses must not rebuild the list of a ready handle"
        e1, x1, f1, v1 = md.energy(), md.positions(), md.forces(), md.velocities()
        atomic_sums = ("kinetic", "temperature", "pressure", "bond", "angle", "dihedral", "lj14", "coulomb14", "potential_bonded", "potential_nonbonded",
                       "potential")      # (the 1-4 terms are summed in the bonded pass too)
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


def _refused(mdx, md, first, count, poses, n_groups, match, opts=None, no_out=False, no_opts=False):
    lib = mdx.load_library()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    p = np.ascontiguousarray(poses, np.float32)
    n = p.shape[0]
    y = np.full((n, max(p.shape[1], 1), 3), -7.0, np.float32)
    rows = np.full((n, max(n_groups, 1)), -7.0, np.float32)
    rigid, xform = np.full((n, 6), -7.0, np.float32), np.full((n, 7), -7.0, np.float32)
    status, evals = np.full(n, 77, np.uint32), np.full(n, 77, np.uint32)
    opts = opts if opts is not None else _abi.CRefineOpts(12, 0.0, 0.0, 0.0, 0.0)
    rc = lib.mdx_refine_poses(md._h, first, count, n, p.ctypes.data_as(fp), None if no_opts else C.byref(opts),
                              None if no_out else y.ctypes.data_as(fp), rows.ctypes.data_as(fp), n_groups, rigid.ctypes.data_as(fp),
                              xform.ctypes.data_as(fp), status.ctypes.data_as(up), evals.ctypes.data_as(up))
    msg = lib.mdx_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all((a == -7.0).all() for a in (y, rows, rigid, xform)) and (status == 77).all() and (evals == 77).all(), \
        "a refused call must leave its outputs untouched"
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
        assert md.refine_poses(lo, poses, 2, 0.0, 0.0)[0].shape == (2, n, 3)
        # those of mdx_pose_forces
        _refused(mdx, md, lo, n, poses, 3, "null", no_out=True)
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
        g4 = g.copy()
        g4[lo + n // 2:hi] = 3
        md.set_energy_groups(g4, 4)
        _refused(mdx, md, lo, n // 2, poses[:, :n // 2], 4, "links the range")
        md.set_energy_groups(g, 3)
        # the new ones
        _refused(mdx, md, lo, n, poses, 3, "null", no_opts=True)
        _refused(mdx, md, lo, n, poses, 3, "max_evals", opts=_abi.CRefineOpts(0, 0.0, 0.0, 0.0, 0.0))
        _refused(mdx, md, lo, n, poses, 3, "max_evals", opts=_abi.CRefineOpts(_abi.REFINE_MAX_EVALS_CAP + 1, 0.0, 0.0, 0.0, 0.0))
        _refused(mdx, md, lo, n, poses, 3, "negative", opts=_abi.CRefineOpts(12, -1.0, 0.0, 0.0, 0.0))
        _refused(mdx, md, lo, n, poses, 3, "not finite", opts=_abi.CRefineOpts(12, 0.0, float("nan"), 0.0, 0.0))
        _refused(mdx, md, lo, n, poses, 3, "not finite", opts=_abi.CRefineOpts(12, 0.0, 0.0, float("inf"), 0.0))
        _refused(mdx, md, lo, n, poses, 3, "negative", opts=_abi.CRefineOpts(12, 0.0, 0.0, 0.0, -0.1))
        _refused(mdx, md, lo, n, poses, 3, "h_start", opts=_abi.CRefineOpts(12, 0.0, 0.0, 0.3, 0.25))
        # n_poses == 0 succeeds and does nothing
        out = np.full(18, -7.0, np.float32)
        o = out.ctypes.data_as(C.POINTER(C.c_float))
        assert mdx.load_library().mdx_refine_poses(md._h, lo, n, 0, None, None, o, o, 3, o, o, None, None) == 0 and (out == -7.0).all()
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
