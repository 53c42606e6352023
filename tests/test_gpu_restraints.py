"""Position restraints on the device (include/mdx.h: mdx_set_position_restraints): forces and energies against the float64
statement of tests/restraint_ref.py, analytic dynamics through every step arrangement, references that follow the box, the
restrained minimiser, decomposed handles, set / replace / clear and the refusals."""
import math
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, systems
from molchanica_amd._abi import OVR_BONDED_DISABLED, OVR_COULOMB_DISABLED, OVR_LJ_DISABLED, OVR_LONG_RANGE_RECIP_DISABLED
from tests.restraint_ref import restraint_efw, scale_about, verlet_free

pytestmark = pytest.mark.gpu

CFG = dict(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)
NOTHING = OVR_BONDED_DISABLED | OVR_COULOMB_DISABLED | OVR_LJ_DISABLED | OVR_LONG_RANGE_RECIP_DISABLED


def _box(s):
    lo, hi = np.asarray(s.box_lo, np.float64), np.asarray(s.box_hi, np.float64)
    per = (True, True, True) if s.periodic else (False, False, False)
    return lo, hi, per


def _heavy(s, n_max=None):
    """Atoms of the first molecule that are not hydrogens (lj_type 3 marks the chain's hydrogens in systems.py)."""
    n_sol = int(s.mol_start[1]) if s.mol_start is not None and len(s.mol_start) > 1 else s.n_atoms
    h = np.nonzero(s.lj_type[:n_sol] != 3)[0]
    return h if n_max is None else h[:n_max]


def _restraint_set(pos, idx, rng, lo=None, hi=None, seam=0):
    """References near the atoms, flat bottoms mixed (some atoms inside their radius, some outside); the first `seam` references
    sit one box edge away from their atoms (the minimum image has to bring them back)."""
    n = len(idx)
    ref = pos[idx].astype(np.float64) + rng.normal(0.0, 0.6, (n, 3))
    k = rng.uniform(1.0, 25.0, n)
    b = np.where(np.arange(n) % 3 == 0, 0.0, np.where(np.arange(n) % 3 == 1, 5.0, 0.25))      # 5 A: inside, 0.25: mostly outside
    if seam:
        L = hi - lo
        sgn = np.where(pos[idx[:seam]] - lo > 0.5 * L, -1.0, 1.0)
        ref[:seam] = pos[idx[:seam]] + 0.3 + sgn * L * np.array([1.0, 0.0, 1.0])
    return ref.astype(np.float32), k.astype(np.float32), b.astype(np.float32)


def _compare_forces(s, cfg, idx, rng, seam=0):
    """nb_variant 2 (the deterministic pair kernel): both handles sum the same pair forces in the same order, so F(with) - F(without)
    carries only the rounding of adding the restraint force to the gross force, and that of the restraint itself (its reference is
    box_lo + f L in fp32)."""
    from molchanica_amd.md_state import MdState
    cfg.nb_variant = 2
    lo, hi, per = _box(s)
    with MdState(s, cfg) as md0:
        f0 = md0.forces().astype(np.float64)
        pos = md0.positions()          # (after the force call: with constraints, the first one projects the initial positions)
        e0 = md0.energy()
    with MdState(s, cfg) as md:
        ref, k, b = _restraint_set(pos, idx, rng, lo, hi, seam)
        md.set_position_restraints(idx, ref, k, b)
        f1 = md.forces().astype(np.float64)
        e1 = md.energy()
        er = md.restraint_energy()
    e_np, f_np, w_np = restraint_efw(pos, idx, ref, k, b, lo, hi, per)
    assert e_np > 0 and (np.linalg.norm(f_np[idx], axis=1) == 0).any() and (np.linalg.norm(f_np[idx], axis=1) > 0).any()
    gross = np.abs(f0) + np.abs(f_np) + 1.0
    ulp_ref = np.zeros(s.n_atoms)
    ulp_ref[idx] = 2.0 * k * 2.4e-7 * (np.abs(ref).max(1) + np.abs(pos[idx]).max(1) + (np.abs(hi - lo).max() if s.periodic else 0.0))
    assert (np.abs((f1 - f0) - f_np) <= 4e-6 * gross + ulp_ref[:, None] + 1e-5).all(), np.max(np.abs((f1 - f0) - f_np) / gross)
    assert er["energy"] == pytest.approx(e_np, rel=2e-6, abs=1e-6)
    assert er["virial"] == pytest.approx(w_np, rel=2e-6, abs=1e-5)
    assert e1["potential"] - e0["potential"] == pytest.approx(e_np, rel=1e-6, abs=2e-6 * abs(e0["potential"]) + 1e-6)
    assert e1["potential_bonded"] - e0["potential_bonded"] == pytest.approx(er["energy"], rel=1e-9, abs=1e-12 * abs(e0["potential_bonded"]) + 1e-9)
    assert e1["lj"] == pytest.approx(e0["lj"], rel=1e-12) and e1["bond"] == pytest.approx(e0["bond"], rel=1e-12)


def test_force_difference_lig50_vacuum():
    s = systems.lig50()
    _compare_forces(s, MdConfig(lj_cutoff=0.0, coulomb_cutoff=0.0, skin=0.0), np.arange(0, s.n_atoms, 2), np.random.default_rng(1))


def test_force_difference_small_solvated_reaction_field_across_faces():
    s = systems.small_solvated()
    idx = np.concatenate([_heavy(s), np.arange(s.n_atoms - 300, s.n_atoms, 3)])
    _compare_forces(s, MdConfig(coulomb_mode=1, **CFG), idx, np.random.default_rng(2), seam=12)


def test_force_difference_ewald_spme():
    s = systems.small_solvated()
    cfg = MdConfig(coulomb_mode=2, ewald_alpha=0.32, overrides=0, pme_grid=(32, 32, 32), **CFG)
    _compare_forces(s, cfg, _heavy(s), np.random.default_rng(3), seam=5)


def _chain_in_rigid_water():
    """As tests/test_gpu_constraints.py builds it: a chain with X-H bonds constrained in rigid three-site water."""
    s = systems.small_solvated(n_chain=160, box=30.0)
    n_sol = int(s.mol_start[1])
    t = systems.TIP3P
    nw = (s.n_atoms - n_sol) // 3
    keep_a = (s.angle_idx < n_sol).all(1)
    h_side = np.nonzero(s.lj_type == 3)[0]
    is_h = np.zeros(s.n_atoms, bool); is_h[h_side] = True
    xh = (s.bond_idx < n_sol).all(1) & (is_h[s.bond_idx[:, 0]] | is_h[s.bond_idx[:, 1]])
    keep_b = (s.bond_idx < n_sol).all(1) & ~xh
    base = n_sol + 3 * np.arange(0, nw, dtype=np.int64)
    hh = 2 * t["r_oh"] * math.sin(t["theta"] / 2)
    wc = np.stack([np.stack([base, base + 1], 1), np.stack([base, base + 2], 1), np.stack([base + 1, base + 2], 1)], 1).reshape(-1, 2)
    s.constraint_idx = np.concatenate([s.bond_idx[xh].astype(np.int64), wc]).astype(np.uint32)
    s.constraint_len = np.concatenate([s.bond_r0[xh], np.tile([t["r_oh"], t["r_oh"], hh], len(base))]).astype(np.float32)
    s.bond_idx, s.bond_k, s.bond_r0 = s.bond_idx[keep_b], s.bond_k[keep_b], s.bond_r0[keep_b]
    s.angle_idx, s.angle_k, s.angle_theta0 = s.angle_idx[keep_a], s.angle_k[keep_a], s.angle_theta0[keep_a]
    return s, n_sol


def test_force_difference_shake_chain_in_rigid_water():
    s, n_sol = _chain_in_rigid_water()
    idx = np.nonzero(s.lj_type[:n_sol] != 3)[0]
    _compare_forces(s, MdConfig(coulomb_mode=1, **CFG), idx, np.random.default_rng(4))


# ---- analytic dynamics --------------------------------------------------------------------------------------------------------
def _oscillators(s, idx, md_kwargs, bursts, rng, big_steps=False, profile=False):
    """Everything but the restraints off: restrained atoms are 3-D oscillators, free atoms move in straight lines."""
    from molchanica_amd.md_state import MdState
    lo, hi, per = _box(s)
    cfg = MdConfig(overrides=NOTHING, **md_kwargs)
    dt = 0.001
    with MdState(s, cfg) as md:
        x0 = md.positions().astype(np.float64)
        v0 = rng.normal(0.0, 0.02, x0.shape).astype(np.float32)
        if big_steps:       # free atoms fast enough to leave their list skin: rebuilds re-fill the restraint roles
            v0[::7] *= 40.0
        md.set_velocities(v0)
        n = len(idx)
        ref = (x0[idx] + rng.normal(0.0, 0.4, (n, 3))).astype(np.float32)
        k = rng.uniform(2.0, 30.0, n).astype(np.float32)
        b = np.where(np.arange(n) % 2 == 0, 0.0, 0.3).astype(np.float32)
        md.set_position_restraints(idx, ref, k, b)
        r0 = md.stats()["rebuild_count"]
        if profile:
            md.profile(1)
        for nb in bursts:
            md.step(dt, None, nb)
        if profile:
            md.profile(0)
        st, info = md.stats(), md.pair_launch_info()
        x1, v1 = md.positions().astype(np.float64), md.velocities().astype(np.float64)
    m = np.asarray(s.mass, np.float64)
    xr, vr = verlet_free(x0, v0.astype(np.float64), m, idx, ref, k, b, dt, sum(bursts), lo, hi, per)
    d = x1 - xr
    if s.periodic:
        L = hi - lo
        d -= np.round(d / L) * L
    # stated bound: fp32 coordinates round by half an ulp of the box edge per drift; over n steps (phase errors of the oscillators
    # included) the drift of a trajectory stays below 4 ulp per step, and a velocity error is omega times a position error
    n_steps = sum(bursts)
    ulp = np.spacing(np.float32(max(np.abs(x0).max(), 1.0)))
    x_bound = 4.0 * float(ulp) * n_steps
    omega = math.sqrt(2.0 * float(k.max()) * 418.4 / float(m[idx].min()))
    return np.abs(d).max() / x_bound, np.abs(v1 - vr).max() / (omega * x_bound), st, info, st["rebuild_count"] - r0


@pytest.mark.parametrize("bursts", [(1,), (7,), (48,), (1, 7, 48)])
def test_analytic_oscillators_small_system(bursts):
    s = systems.small_solvated()
    idx = np.concatenate([_heavy(s), np.arange(s.n_atoms - 400, s.n_atoms, 4)])
    dx, dv, st, info, nreb = _oscillators(s, idx, CFG, bursts, np.random.default_rng(5), big_steps=True)
    assert st["n_tiles"] < 2048
    assert info["one_launch_steps"] == 0 and info["step"]["bonded_workgroups"] == 0     # separate passes: no ride-along, no one-pass step
    assert dx < 1.0 and dv < 1.0, (dx, dv)                                               # (fractions of the stated bound)
    if sum(bursts) >= 48:
        assert nreb >= 1                                                                  # the restraint roles were re-filled


@pytest.mark.parametrize("bursts", [(1, 7), (48,)])
def test_analytic_oscillators_fused_pass_water_box(bursts):
    s = systems.water_box(40)
    rng = np.random.default_rng(6)
    idx = np.sort(rng.choice(s.n_atoms, s.n_atoms // 12, replace=False))
    dx, dv, st, info, nreb = _oscillators(s, idx, dict(CFG, chunk_steps=16), bursts, rng, big_steps=sum(bursts) >= 48, profile=True)
    assert st["n_tiles"] >= 2048
    assert st["fused_launches"] > 0
    assert dx < 1.0 and dv < 1.0, (dx, dv)
    if sum(bursts) >= 48:
        assert nreb >= 1


# ---- references follow the box -------------------------------------------------------------------------------------------------
def test_references_follow_barostat_and_shrink():
    from molchanica_amd.md_state import MdState
    s = systems.small_solvated()
    cfg = MdConfig(coulomb_mode=1, **CFG)
    rng = np.random.default_rng(7)
    with MdState(s, cfg) as md:
        idx = _heavy(s)
        pos = md.positions()
        ref, k, b = _restraint_set(pos, idx, rng)
        md.set_position_restraints(idx, ref, k, b)
        lo0, hi0 = [np.asarray(v, np.float64) for v in md.cell()]
        got = md.position_restraints()
        assert np.allclose(got["ref"], ref, atol=2e-5) and (got["idx"] == idx).all() and np.allclose(got["k"], k) and np.allclose(got["flat_bottom"], b)
        md.set_barostat(1, pressure_target_bar=2000.0, tau_ps=0.05, compressibility_per_bar=4.5e-4, every_n_steps=5)
        md.step(0.0005, None, 20)
        md.set_barostat(0)
        lo1, hi1 = [np.asarray(v, np.float64) for v in md.cell()]
        assert not np.allclose(hi1 - lo1, hi0 - lo0)
        mu = (hi1 - lo1) / (hi0 - lo0)
        want = lo1 + mu * (ref.astype(np.float64) - lo0)
        assert np.abs(md.position_restraints()["ref"] - want).max() < 5e-5 * np.abs(want).max()
        shrank = md.shrink_cell_towards(lo1 + 0.2, hi1 - 0.2, 0.3)
        assert shrank
        lo2, hi2 = [np.asarray(v, np.float64) for v in md.cell()]
        c = 0.5 * (lo1 + hi1)
        want2 = c + (hi2 - lo2) / (hi1 - lo1) * (want - c)
        assert np.abs(md.position_restraints()["ref"] - want2).max() < 5e-5 * np.abs(want2).max()
        e = md.energy(); er = md.restraint_energy()
        e_np, _, _ = restraint_efw(md.positions(), idx, md.position_restraints()["ref"], k, b, lo2, hi2, (True, True, True))
        assert er["energy"] == pytest.approx(e_np, rel=1e-4, abs=1e-4) and np.isfinite(e["pressure"])


def test_virial_matches_energy_change_under_set_cell():
    from molchanica_amd.md_state import MdState
    s = systems.small_solvated()
    cfg = MdConfig(overrides=NOTHING, **CFG)
    rng = np.random.default_rng(8)
    with MdState(s, cfg) as md:
        pos = md.positions().astype(np.float64)
        idx = _heavy(s)
        ref = (pos[idx] + rng.normal(0, 1.0, (len(idx), 3))).astype(np.float32)
        k = rng.uniform(5.0, 20.0, len(idx)).astype(np.float32)
        b = np.where(np.arange(len(idx)) % 4 == 0, 0.4, 0.0).astype(np.float32)
        md.set_position_restraints(idx, ref, k, b)
        md.energy(); er0 = md.restraint_energy()
        lo, hi = [np.asarray(v, np.float64) for v in md.cell()]
        eps = 1e-4
        md.set_cell(lo, lo + (1 + eps) * (hi - lo))
        md.set_positions(scale_about(pos, lo, 1 + eps))
        md.energy(); er1 = md.restraint_energy()
    de = er1["energy"] - er0["energy"]
    assert de == pytest.approx(-er0["virial"] * eps, rel=2e-2, abs=1e-3), (de, -er0["virial"] * eps)


# ---- restrained minimiser -------------------------------------------------------------------------------------------------------
def test_restrained_minimiser_reaches_a_restrained_minimum():
    from molchanica_amd.md_state import MdState
    from oracle import oracle
    s = systems.lig50()
    cfg = MdConfig(lj_cutoff=0.0, coulomb_cutoff=0.0, skin=0.0)
    with MdState(s, cfg) as md:
        idx = np.nonzero(np.asarray(s.mass) > 2.0)[0]
        pos0 = md.positions()
        ref = (pos0[idx] + np.random.default_rng(9).normal(0, 0.3, (len(idx), 3))).astype(np.float32)
        md.set_position_restraints(idx, ref, 10.0)
        tol = 2.0
        e, it = md.minimize_energy(5000, None, tol)
        x = md.positions().astype(np.float64)
        er = md.restraint_energy()
    fo, _ = oracle.forces(s, cfg, pos=x)
    e_np, f_np, _ = restraint_efw(x, idx, ref, 10.0)
    assert np.abs(fo + f_np).max() < 1.5 * tol, np.abs(fo + f_np).max()
    assert er["energy"] == pytest.approx(e_np, rel=1e-5, abs=1e-5)


# ---- decomposed handles ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def _separate_kick(monkeypatch):
    monkeypatch.setenv("MDX_ONEPASS", "0")      # (same rounding on both sides: tests/test_gpu_comm.py)


def run_ranks(system, cfg, world, n_steps, dt=0.0005, before=None, after=None, want_forces=False):
    """As tests/test_gpu_comm.py::run_ranks; before(md, rank) / after(md, rank) configure a handle before / after it joins."""
    from molchanica_amd.md_state import Fabric, MdState
    fabric = Fabric(world)
    res, errs = {}, []

    def run(rank):
        try:
            with MdState(system, cfg) as md:
                if before:
                    before(md, rank)
                md.comm_init_fabric(fabric, rank)
                if after:
                    after(md, rank)
                e0 = md.energy()
                f0 = md.forces() if want_forces else None
                md.step(dt, None, n_steps)
                res[rank] = dict(pos=md.positions(), e0=e0, f0=f0, e1=md.energy(), er=md.restraint_energy(), stats=md.stats())
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]
    return res


def _rms(a, b, L):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    d -= np.round(d / L) * L
    return math.sqrt((d ** 2).sum(1).mean())


@pytest.mark.parametrize("world", [2, 4])
def test_decomposed_handles_match_one_gpu(_separate_kick, world):
    from molchanica_amd.md_state import MdState
    s = systems.water_box(14, seed=8)
    cfg = MdConfig(coulomb_mode=1, chunk_steps=8, **CFG)
    L = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    rng = np.random.default_rng(10)
    idx = np.sort(rng.choice(s.n_atoms, 300, replace=False))
    ref = (np.asarray(s.pos, np.float64)[idx] + rng.normal(0, 0.7, (300, 3))).astype(np.float32)
    ref[:10] += (L * np.array([1, 0, -1])).astype(np.float32)       # across the faces of the global box
    k = rng.uniform(2.0, 20.0, 300).astype(np.float32)
    b = np.where(np.arange(300) % 3 == 0, 0.5, 0.0).astype(np.float32)
    with MdState(s, cfg) as md:
        md.set_position_restraints(idx, ref, k, b)
        e_ref, f_ref, er_ref = md.energy(), md.forces(), md.restraint_energy()
        md.step(0.0005, None, 20)
        p_ref = md.positions()
    res = run_ranks(s, cfg, world, 20, want_forces=True,
                    before=lambda md, r: md.set_position_restraints(idx, ref, k, b) if r % 2 == 0 else None,
                    after=lambda md, r: md.set_position_restraints(idx, ref, k, b) if r % 2 == 1 else None)
    for r in range(world):
        assert res[r]["er"]["energy"] == pytest.approx(res[0]["er"]["energy"], rel=1e-9)
        df = np.linalg.norm(res[r]["f0"].astype(np.float64) - f_ref, axis=1)
        assert (df <= 2e-4 * np.maximum(np.linalg.norm(f_ref, axis=1), 1.0) + 2e-4).all()
        assert abs(res[r]["e0"]["potential"] - e_ref["potential"]) <= max(2e-2, 3e-6 * abs(e_ref["potential"]))
        assert rms_ok(res[r]["pos"], p_ref, L)
    assert res[0]["e0"]["potential_bonded"] == pytest.approx(e_ref["potential_bonded"], rel=1e-5, abs=1e-3)
    assert er_ref["energy"] > 0


def rms_ok(a, b, L):
    return _rms(a, b, L) < 2e-3


def test_decomposed_restraints_after_a_repartition(_separate_kick):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.water_box(14, seed=8)
    cfg = MdConfig(coulomb_mode=1, chunk_steps=8, **CFG)
    L = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    rng = np.random.default_rng(11)
    idx = np.sort(rng.choice(s.n_atoms, 200, replace=False))
    with MdState(s, cfg) as md:
        md.step(0.0005, None, 30)
        md.set_positions(md.positions())
        ref = md.positions()[idx] + rng.normal(0, 0.5, (200, 3)).astype(np.float32)
        md.set_position_restraints(idx, ref, 8.0)
        md.step(0.0005, None, 20)
        p_ref = md.positions()
    fabric = Fabric(2)
    res, errs = {}, []

    def run(rank):
        try:
            with MdState(s, cfg) as md:
                md.comm_init_fabric(fabric, rank)
                md.step(0.0005, None, 30)
                n_rep = md.stats()["repartitions"]
                md.set_positions(md.positions())              # (collective: the ranks repartition from the gathered state)
                assert md.stats()["repartitions"] > n_rep
                md.set_position_restraints(idx, ref, 8.0)
                md.step(0.0005, None, 20)
                res[rank] = md.positions()
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]
    assert _rms(res[0], p_ref, L) < 2e-3 and _rms(res[1], p_ref, L) < 2e-3


# ---- set, replace, clear --------------------------------------------------------------------------------------------------------
def test_set_then_clear_is_bitwise_a_never_restrained_handle():
    from molchanica_amd.md_state import MdState
    s = systems.small_solvated()
    cfg = MdConfig(coulomb_mode=1, nb_variant=2, **CFG)
    with MdState(s, cfg) as md:
        md.step(0.0005, None, 30)
        p0, v0 = md.positions(), md.velocities()
    with MdState(s, cfg) as md:
        md.set_position_restraints(_heavy(s), None, 5.0, 0.1)
        md.energy()
        md.clear_position_restraints()
        assert md.position_restraints()["idx"].size == 0
        md.step(0.0005, None, 30)
        p1, v1 = md.positions(), md.velocities()
        md.energy()
        assert md.restraint_energy() == {"energy": 0.0, "virial": 0.0}
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1)


def test_replacing_the_set_replaces_it():
    from molchanica_amd.md_state import MdState
    s = systems.lig50()
    cfg = MdConfig(lj_cutoff=0.0, coulomb_cutoff=0.0, skin=0.0)
    rng = np.random.default_rng(12)
    with MdState(s, cfg) as md:
        pos = md.positions()
        a, b_ = np.arange(0, 20), np.arange(10, 40)
        ra = pos[a] + rng.normal(0, 0.5, (20, 3)).astype(np.float32)
        rb = pos[b_] + rng.normal(0, 0.5, (30, 3)).astype(np.float32)
        md.set_position_restraints(a, ra, 3.0)
        md.set_position_restraints(b_, rb, np.linspace(1.0, 9.0, 30), flat_bottom=0.2)
        got = md.position_restraints()
        assert (got["idx"] == b_).all() and np.allclose(got["ref"], rb, atol=1e-5) and np.allclose(got["k"], np.linspace(1.0, 9.0, 30))
        md.energy()
        e_np, _, _ = restraint_efw(pos, b_, rb, np.linspace(1.0, 9.0, 30), 0.2)
        assert md.restraint_energy()["energy"] == pytest.approx(e_np, rel=2e-6, abs=1e-6)
        md.set_position_restraints(a[:5])                # ref None: the current positions - zero energy and force
        assert np.allclose(md.position_restraints()["ref"], pos[a[:5]], atol=1e-5)
        md.energy()
        assert md.restraint_energy()["energy"] == pytest.approx(0.0, abs=1e-8)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from molchanica_amd.md_state import MdState, ParamError
    s = systems.small_solvated()
    with MdState(s, MdConfig(coulomb_mode=1, **CFG)) as md:
        r = np.zeros((2, 3), np.float32)
        cases = [
            (dict(idx=[0, s.n_atoms], ref=r), "out of range"),
            (dict(idx=[3, 3], ref=r), "duplicate"),
            (dict(idx=[0, 1], ref=r, k=[1.0, 0.0]), "k must be"),
            (dict(idx=[0, 1], ref=r, k=[1.0, float("inf")]), "k must be"),
            (dict(idx=[0, 1], ref=np.array([[0, 0, 0], [0, np.nan, 0]], np.float32)), "non-finite reference"),
            (dict(idx=[0, 1], ref=r, flat_bottom=[0.0, -0.1]), "flat-bottom"),
        ]
        for kw, msg in cases:
            with pytest.raises(ParamError, match=msg):
                md.set_position_restraints(**kw)
        assert md.position_restraints()["idx"].size == 0        # a refused set leaves the handle as it was
    s2, n_sol = _chain_in_rigid_water()
    with MdState(s2, MdConfig(coulomb_mode=1, **CFG)) as md:
        if md.pair_launch_info()["water_step_launches"] == 0:
            md.step(0.0005, None, 2)
        with pytest.raises(ParamError, match="rigid water"):
            md.set_position_restraints([n_sol + 4], None, 1.0)
        md.set_position_restraints([0, 1], None, 1.0)            # the solute's atoms are fine
    s3 = systems.opc_water_box(6)
    with MdState(s3, MdConfig(coulomb_mode=1, lj_cutoff=5.0, coulomb_cutoff=5.0, skin=1.0)) as md:
        site = int(np.asarray(s3.vsite_idx).reshape(-1, 4)[0, 0])
        with pytest.raises(ParamError, match="virtual site"):
            md.set_position_restraints([site], None, 1.0)
