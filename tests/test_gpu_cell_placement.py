"""The periodic hot path in the cells a caller hands over: off the origin, with three different edges (tests/cell_cases.py).
Every generator of molchanica_amd/systems.py builds `box_lo = (0, 0, 0)`, nearly all a cube - there a `lo` applied to the wrong
axis, a barostat scaling about the origin, an `(int)` where `floorf` was meant or a swapped edge are invisible.  Everything here
is held against the fp64 oracle at the downloaded fp32 positions with the bounds the origin tests use (tests/test_gpu_parity.py,
test_gpu_edge_geometry.py, test_gpu_constraints.py, test_gpu_pressure.py), unchanged: the existing bounds are met with
coordinates up to 90 A (edge geometry) and 217 A (water1m), and every coordinate here stays below 100 A."""
import math

import numpy as np
import pytest

from molchanica_amd import MdConfig, SimBoxInit, systems
from molchanica_amd import _abi
from tests.cell_cases import NEG, PAD, cell_of, energy_ratio, force_ratios, placed, record, rms_dev
from tests.test_gpu_constraints import bond_errors
from tests.test_gpu_edge_geometry import CASES, case_system, single_point_and_step_loop
from tests.test_gpu_parity import assert_energies, assert_forces

pytestmark = pytest.mark.gpu

GROW = (0.0, 3.5, 8.0)      # small_solvated: 26 x 29.5 x 34 A, a vacuum slab along y and z


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1
    return md_state


def single_point(mdx, orc, s, cfg, what):
    """tests.test_gpu_parity.check_single_point, with the margins noted and the cell read back."""
    with mdx.MdState(s, cfg) as md:
        pos, f, e = md.positions(), md.forces(), md.energy()
        lo, L = cell_of(md)
    assert np.array_equal(lo, np.asarray(s.box_lo, np.float32).astype(np.float64))
    assert ((pos >= lo - 1e-4) & (pos <= lo + L + 1e-4)).all(), "the engine hands back positions wrapped into ITS cell"
    fo, eo = orc.forces(s, cfg, pos=pos.astype(np.float64), use_cells=False)
    slack = orc.cutoff_slack(s, cfg, pos=pos)
    r_atom, r_rms = force_ratios(f, fo, slack)
    record(what, force_atom=r_atom, force_rms=r_rms, energy=energy_ratio(e, eo))
    assert_forces(f, fo, slack, what)
    assert_energies(e, eo, what)
    return pos


@pytest.mark.parametrize("name", list(CASES))
def test_edge_geometry_cases_off_origin(mdx, orc, name):
    """Strongly orthorhombic, smallest cell for the list radius, sparse - at PAD: single point, neighbour list bit for bit,
    60 steps through the step loop."""
    s, rc, skin = case_system(name)
    single_point_and_step_loop(mdx, orc, placed(s, PAD), rc, skin, name + " at PAD")


@pytest.mark.parametrize("where", ["origin", "PAD", "NEG"])
@pytest.mark.parametrize("mode,alpha", [(0, 0.0), (1, 0.0), (2, 0.35)])
def test_solvated_chain_in_an_orthorhombic_cell(mdx, orc, mode, alpha, where):
    """Dihedrals, 1-4 pairs, exclusions; shifted, reaction-field and Ewald real-space Coulomb.  (origin: the same grown cell at
    (0, 0, 0) - the figure the placed ones stand beside.)"""
    s = placed(systems.small_solvated(), {"origin": (0, 0, 0), "PAD": PAD, "NEG": NEG}[where], grow=GROW)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=mode, ewald_alpha=alpha,
                   overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED)
    pos = single_point(mdx, orc, s, cfg, f"small_solvated grown, mode {mode}, {where}")
    if where == "NEG":
        assert (pos < 0).all()


def test_the_default_padded_cell_of_a_ligand(mdx, orc):
    """`SimBoxInit::Pad(12)`, the reference's default cell: the extent of the atoms plus 12 A a side."""
    s = systems.lig50().apply_sim_box(SimBoxInit.Pad(12.0))
    lo, hi = np.asarray(s.box_lo), np.asarray(s.box_hi)
    assert (lo < -10).all() and len(set(np.round(hi - lo, 3))) == 3
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1)
    single_point(mdx, orc, s, cfg, "lig50 in Pad(12)")
    with mdx.MdState(s, cfg) as md:
        pos = md.positions()
        off, idx = md.neighbor_list()
        ooff, oidx = orc.neighbor_list(s, 10.5, pos=pos, use_cells=False)
        assert idx.size > 0 and np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        x0, v0 = pos.astype(np.float64), md.velocities().astype(np.float64)
        md.step(0.0005, None, 50)
        x = md.positions().astype(np.float64)
        _, L = cell_of(md)
    xo, _, _ = orc.step(s, cfg, 0.0005, 50, pos=x0, vel=v0)
    rms = rms_dev(x, xo, L)
    record("lig50 in Pad(12): 50 steps", rms_over_2e4=rms / 2e-4)
    assert rms < 2e-4, rms      # (the bound of tests/test_gpu_parity.py::test_golden_vectors[lig50])


@pytest.mark.parametrize("where", ["origin", "PAD"])
@pytest.mark.parametrize("model", ["tip3p_rigid", "opc"])
def test_rigid_waters_straddling_faces_off_origin(mdx, orc, model, where):
    """tests/test_gpu_constraints.py::test_rigid_waters_straddling_box_faces in a cell that does not start at zero: SHAKE moves
    atoms by corrections, and a virtual site must be rebuilt in the image it is stored in."""
    s = systems.water_box(6, seed=7, rigid=True) if model == "tip3p_rigid" else systems.opc_water_box(6, seed=7)
    L = np.array(s.box_hi, dtype=np.float64)
    lo = np.asarray(PAD if where == "PAD" else (0, 0, 0), np.float64)
    s.pos = (np.mod(np.asarray(s.pos, dtype=np.float64) + 1.25, L) + lo).astype(np.float32)
    s.box_lo, s.box_hi = tuple(lo), tuple(lo + L)
    nsite = 3 if model == "tip3p_rigid" else 4
    w = s.pos.reshape(-1, nsite, 3)
    assert (np.abs(w[:, 1:] - w[:, :1]).max(axis=(1, 2)) > 0.5 * L[0]).sum() > 30, "no water straddles a face"
    cfg = MdConfig(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=1)
    with mdx.MdState(s, cfg) as md:
        _, Lc = cell_of(md)
        f, e = md.forces().astype(np.float64), md.energy()
        x0, v0 = md.positions().astype(np.float64), md.velocities().astype(np.float64)
        fo, eo = orc.forces(s, cfg, pos=x0)
        err = np.linalg.norm(f - fo, axis=1)
        tol = 1e-4 * np.maximum(np.linalg.norm(fo, axis=1), 1.0) + orc.cutoff_slack(s, cfg, pos=x0)
        record(f"straddling {model} {where}: forces", ratio=float((err / tol).max()))
        assert (err <= tol).all(), float((err / tol).max())
        for k in ("lj", "coulomb"):
            assert e[k] == pytest.approx(eo[k], rel=5e-6, abs=2e-2)
        t0 = e["potential"] + e["kinetic"]
        md.step(0.002, None, 60)
        x = md.positions().astype(np.float64)
        e1 = md.energy()
        assert md.stats()["rebuild_count"] >= 3
        assert bond_errors(s, x).max() < 3e-5
    xo, vo, _ = orc.step(s, cfg, 0.002, 60, pos=x0, vel=v0, use_cells=True)
    rms = rms_dev(x, xo, Lc)
    drift = abs(e1["potential"] + e1["kinetic"] - t0) / (0.02 * e["kinetic"])
    record(f"straddling {model} {where}: 60 steps", rms_over_2e3=rms / 2e-3, bond=float(bond_errors(s, x).max() / 3e-5), drift=drift)
    assert rms < 2e-3, f"trajectory deviates from the oracle: {rms:.2e} A"
    assert drift < 1.0, "energy not conserved over 60 steps of NVE"


def test_barostat_scales_about_box_lo(mdx, orc):
    """tests/test_gpu_pressure.py::test_barostat_follows_the_oracle at PAD: the weak-coupling barostat scales coordinates and
    edges about `box_lo` (the oracle's rule, oracle/mdx_oracle.c), which therefore stays where it is, bit for bit."""
    s = placed(systems.water_box(6, seed=7), PAD)
    cfg = MdConfig(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=1)
    dt, n = 0.0005, 60
    baro = (1, 1.0, 0.05, 4.5e-5, 10)
    with mdx.MdState(s, cfg) as md:
        lo0, _ = md.cell()
        md.set_barostat(*baro)
        md.step(dt, None, n)
        pos = md.positions().astype(np.float64); lo, hi = md.cell(); e = md.energy()
    xo, vo, hio, ps, vs = orc.step_npt(s, cfg, dt, n, barostat=baro, use_cells=True)
    assert len(ps) == 6
    assert np.array_equal(lo, lo0) and np.array_equal(lo, np.asarray(PAD, np.float32))
    edge0 = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    edge, edge_o = hi.astype(np.float64) - lo, hio.astype(np.float64) - lo
    assert (np.abs(edge_o / edge0 - 1.0) > 1e-4).all(), "the test must actually move the box"
    for d in range(3):
        assert float(hi[d]) == pytest.approx(float(hio[d]), rel=2e-6)
    assert e["volume"] == pytest.approx(vs[-1], rel=1e-5)
    rms = rms_dev(pos, xo, edge)
    record("barostat at PAD", hi=float(np.abs(hi.astype(np.float64) / hio - 1.0).max() / 2e-6), volume=abs(e["volume"] / vs[-1] - 1.0) / 1e-5,
           rms_over_1e3=rms / 1e-3)
    assert rms < 1e-3
