"""GPU parity of the SPME reciprocal sum: against the numpy SPME restatement
on the same mesh (tight) and against the textbook Ewald sum (loose: mesh discretisation)."""
import dataclasses
import math

import numpy as np
import pytest

from molchanica_amd import MdConfig, systems
from molchanica_amd import _abi
from tests.cell_cases import PAD, approx_ratio, cell_of, placed, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1
    return md_state


def excluded_pairs(s):
    ii = np.repeat(np.arange(s.n_atoms), np.diff(s.excl_offsets.astype(np.int64)))
    jj = s.excl_idx.astype(np.int64)
    m = ii < jj
    pairs = np.stack([ii[m], jj[m]], 1)
    if s.pairs14_idx.shape[0]:
        pairs = np.concatenate([pairs, s.pairs14_idx.astype(np.int64)])
    return pairs


BETA_S, GRID_S = 0.40, (30, 32, 36)      # all K differ, all K / L differ, K0 = 2 * 3 * 5 factors into the x pass's radices
BASE_S = dict(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=BETA_S)
_S = {}


def system_s(mdx):
    """S: small_solvated at PAD in a 26 x 29.5 x 34 A cell, with what every test of it shares computed once: the positions and cell the
    handle holds, the real-space forces and energies, the excluded-pair correction and the textbook Ewald sum (3 s)."""
    if not _S:
        from oracle import pme_ref as P
        s = placed(systems.small_solvated(), PAD, grow=(0.0, 3.5, 8.0))
        with mdx.MdState(s, MdConfig(overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED, **BASE_S)) as md:
            pos = md.positions()
            lo, L = cell_of(md)
            f_real, e_real = md.forces().astype(np.float64), md.energy()
        assert np.allclose(L, (26.0, 29.5, 34.0), atol=1e-4) and np.array_equal(lo, np.asarray(PAD, np.float32).astype(np.float64))
        q = s.charge.astype(np.float64)
        e_x, f_x = P.excluded_pair_correction(pos.astype(np.float64), q, excluded_pairs(s), L, BETA_S)
        e_d, f_d = P.ewald_recip_direct(pos.astype(np.float64), q, L, BETA_S)
        _S.update(s=s, pos=pos, lo=lo, L=L, f_real=f_real, e_real=e_real, q=q, e_x=e_x, f_x=f_x, f_d=f_d + f_x, ref={})
    return _S


def numpy_reference_s(S, grid):
    """-> (coulomb_recip, reciprocal forces incl. the excluded-pair correction) of S on `grid`, computed once per mesh."""
    from oracle import pme_ref as P
    if grid not in S["ref"]:
        e, f = P.spme_recip(S["pos"].astype(np.float64), S["q"], S["lo"], S["L"], BETA_S, grid, 4)
        S["ref"][grid] = (e + S["e_x"] + P.ewald_self_energy(S["q"], BETA_S) + P.ewald_background_energy(S["q"], S["L"], BETA_S), f + S["f_x"])
    return S["ref"][grid]


def rel_rms(f, f_ref):
    return math.sqrt(((f - f_ref) ** 2).sum(1).mean()) / math.sqrt((f_ref ** 2).sum(1).mean())


S_ARMS = {      # spread / gather arm of a single-GPU handle: environment read when the handle sets its mesh up
    "S:tile": {"MDX_PME_SPREAD_BRICK": "0"},
    "S:brick8": {"MDX_PME_SPREAD_BRICK": "1", "MDX_PME_BRICK_EDGE": "8"},
    "S:brick11": {"MDX_PME_SPREAD_BRICK": "1", "MDX_PME_BRICK_EDGE": "11"},
    "S:brick16": {"MDX_PME_SPREAD_BRICK": "1", "MDX_PME_BRICK_EDGE": "16"},
    "S:cap8": {"MDX_PME_SPREAD_BRICK": "1", "MDX_PME_BRICK_CAP": "8"},      # most atoms travel through the overflow list
}


def set_arm(monkeypatch, env):
    for k in ("MDX_PME_SPREAD_BRICK", "MDX_PME_BRICK_EDGE", "MDX_PME_BRICK_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("which,side_stream", [("water", "0"), ("chain", "0"), ("chain", "1"),
                                               ("S:tile", "0"), ("S:tile", "1"), ("S:brick8", "0"), ("S:brick11", "0"), ("S:brick16", "1"), ("S:cap8", "0")])
def test_spme_matches_numpy_restatement_and_ewald(mdx, orc, which, side_stream, monkeypatch):
    """side_stream: the reciprocal-space chain beside the pair kernel on its own stream (the default from 65 k atoms up)
    or on the handle's stream (the default below) - MDX_PME_OVERLAP is read when a handle sets its mesh up.
    S:<arm>: the orthorhombic cell off the origin (system_s), every spread / gather arm, each against numpy absolutely - in a cube at
    the origin a swapped edge, a `lo` on the wrong axis or a brick table built from the wrong edge change nothing."""
    from oracle import pme_ref as P
    monkeypatch.setenv("MDX_PME_OVERLAP", side_stream)
    if which.startswith("S:"):
        S = system_s(mdx)
        set_arm(monkeypatch, S_ARMS[which])
        s, pos, f_real, e_real = S["s"], S["pos"], S["f_real"], S["e_real"]
        with mdx.MdState(s, MdConfig(overrides=0, pme_grid=GRID_S, **BASE_S)) as md:
            f_full = md.forces().astype(np.float64)
            e_full = md.energy()
            assert np.array_equal(md.positions(), pos)
            md.step(0.0005, None, 20)
            e20 = md.energy()
            assert (md.pme_brick_overflows() > 0) == (which == "S:cap8")
        e_ref, f_ref = numpy_reference_s(S, GRID_S)
        f_d = S["f_d"]
    else:
        s = systems.water_box(6, seed=3) if which == "water" else systems.small_solvated()
        L = float(s.box_hi[0])
        beta, grid = 0.40, (24, 24, 24) if which == "water" else (32, 32, 32)
        base = dict(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=beta)
        cfg_real = MdConfig(overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED, **base)
        cfg_full = MdConfig(overrides=0, pme_grid=grid, **base)
        with mdx.MdState(s, cfg_real) as md:
            pos = md.positions()
            f_real = md.forces().astype(np.float64)
            e_real = md.energy()
        with mdx.MdState(s, cfg_full) as md:
            f_full = md.forces().astype(np.float64)
            e_full = md.energy()
            assert np.array_equal(md.positions(), pos)
            md.step(0.0005, None, 20)                       # steps with the mesh in the loop
            e20 = md.energy()
        box = np.full(3, L)
        q = s.charge.astype(np.float64)
        e_ref, f_ref = P.spme_recip(pos.astype(np.float64), q, (0, 0, 0), box, beta, grid, 4)
        e_x, f_x = P.excluded_pair_correction(pos.astype(np.float64), q, excluded_pairs(s), box, beta)
        e_ref += e_x + P.ewald_self_energy(q, beta) + P.ewald_background_energy(q, box, beta)
        f_ref += f_x
        # textbook sum: only the mesh error separates the two
        e_d, f_d = P.ewald_recip_direct(pos.astype(np.float64), q, box, beta)
        f_d += f_x
    assert e_full["coulomb"] == pytest.approx(e_real["coulomb"], rel=1e-6, abs=1e-3) and e_real["coulomb_recip"] == 0.0
    f_rec = f_full - f_real
    err = rel_rms(f_rec, f_ref)
    err_d = rel_rms(f_rec, f_d)
    drift = abs((e20["potential"] + e20["kinetic"]) - (e_full["potential"] + e_full["kinetic"])) / s.n_atoms
    record(f"spme vs numpy [{which}, side stream {side_stream}]", force_rms=err / 2e-4, energy=approx_ratio(e_full["coulomb_recip"], e_ref, 2e-5, 5e-2),
           ewald=err_d / 2e-2, net_force=float(np.abs(f_rec.sum(0) - f_ref.sum(0) if which.startswith("S:") else f_full.sum(0)).max() / 0.5), drift=drift / 0.05)
    assert err < 2e-4, f"reciprocal force rms error {err:.2e} vs the numpy SPME on the same mesh"
    assert e_full["coulomb_recip"] == pytest.approx(e_ref, rel=2e-5, abs=5e-2)
    assert e_full["potential"] == pytest.approx(e_real["potential"] + e_full["coulomb_recip"], rel=1e-7, abs=1e-3)
    assert err_d < 2e-2, err_d
    if which.startswith("S:"):
        # momentum: SPME does not conserve it, and how far off it is belongs to the mesh - on this one the fp64 restatement itself has a net
        # force of (0.186, -2.025, -0.813) kcal/mol/A (the cube's (32, 32, 32) mesh: (0.27, 0.20, -0.38)); the bound holds the kernels'
        # net force to the restatement's
        assert np.abs(f_rec.sum(0) - f_ref.sum(0)).max() < 0.5 and np.abs(f_real.sum(0)).max() < 0.5
    else:
        assert np.abs(f_full.sum(0)).max() < 0.5                               # momentum (mesh: not exact)
    # the jittered lattice releases ~2 kcal/mol/atom in these 20 steps; same bound as the cutoff runs
    assert drift < 0.05


def test_spme_of_a_charged_orthorhombic_cell(mdx):
    """S with a net charge of +7 e: the uniform neutralising background -pi k_e Q^2 / (2 V beta^2) takes V of a cell whose edges all
    differ, and scales as 1 / V: 3 E_background in the virial (mdx_api.hip, mdx_energy).  Energy, forces and the reciprocal virial
    against numpy, with the bounds of the neutral tests."""
    from oracle import pme_ref as P
    from scipy.special import erf
    S = system_s(mdx)
    s = dataclasses.replace(S["s"], charge=S["s"].charge.copy())
    ions = np.random.default_rng(5).choice(s.n_atoms, 7, replace=False)
    s.charge[ions] += np.float32(1.0)
    q, pos, lo, L = s.charge.astype(np.float64), S["pos"].astype(np.float64), S["lo"], S["L"]
    assert q.sum() == pytest.approx(7.0 + S["q"].sum(), abs=1e-4)
    with mdx.MdState(s, MdConfig(overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED, **BASE_S)) as md:
        assert np.array_equal(md.positions(), S["pos"])
        f_real, w_real = md.forces().astype(np.float64), md.energy()["virial"]
    with mdx.MdState(s, MdConfig(overrides=0, pme_grid=GRID_S, **BASE_S)) as md:
        f_full, e_full = md.forces().astype(np.float64), md.energy()
    pairs = excluded_pairs(s)
    e_rec, f_ref = P.spme_recip(pos, q, lo, L, BETA_S, GRID_S, 4)
    e_x, f_x = P.excluded_pair_correction(pos, q, pairs, L, BETA_S)
    e_bg = P.ewald_background_energy(q, L, BETA_S)
    assert e_bg < -1.0, "the background term must be large enough to be seen"
    e_ref = e_rec + e_x + P.ewald_self_energy(q, BETA_S) + e_bg
    err = rel_rms(f_full - f_real, f_ref + f_x)
    # virial (tests/test_gpu_pressure.py::test_spme_reciprocal_virial_matches_numpy): the mesh term, the excluded pairs' sum fs r^2, 3 E_background
    w_rec = P.spme_recip_virial(pos, q, lo, L, BETA_S, GRID_S, 4)
    d = pos[pairs[:, 0]] - pos[pairs[:, 1]]; d -= np.round(d / L) * L
    r = np.linalg.norm(d, axis=1); kqq = P.KE * q[pairs[:, 0]] * q[pairs[:, 1]]
    w_x = float((-kqq * (erf(BETA_S * r) / r ** 3 - 2 * BETA_S / math.sqrt(math.pi) * np.exp(-(BETA_S * r) ** 2) / r ** 2) * r * r).sum())
    w_ref = w_rec + w_x + 3.0 * e_bg
    record("spme, net charge +7 e, S", force_rms=err / 2e-4, energy=approx_ratio(e_full["coulomb_recip"], e_ref, 2e-5, 5e-2),
           virial=approx_ratio(e_full["virial"] - w_real, w_ref, 2e-4, 0.5), e_background=e_bg)
    assert err < 2e-4, err
    assert e_full["coulomb_recip"] == pytest.approx(e_ref, rel=2e-5, abs=5e-2)
    assert e_full["virial"] - w_real == pytest.approx(w_ref, rel=2e-4, abs=0.5)


@pytest.mark.parametrize("grid,edge,cap,side", [((24, 24, 24), None, None, False), ((50, 36, 30), "16", None, False), ((50, 36, 30), "11", None, True),
                                                ((27, 20, 45), "8", None, False), ((32, 32, 32), None, "8", False), ((16, 8, 12), "16", "8", True)])
def test_brick_spread_equals_the_tile_spread(mdx, grid, edge, cap, side, monkeypatch):
    """The charge spread of a single-GPU handle (mdx_pme.hip "Brick spread": bin -> canvas -> combine, no global atomics) and the
    gather through the same bricks (pme_gather_brick_kernel) against the tile kernel and the per-slot gather they replaced, on meshes
    whose edges the bricks do not divide, with every brick edge, with buckets so small that most atoms travel through the overflow
    lists, and (side) with the chain on its side stream, where the reciprocal force has an array of its own."""
    s = systems.small_solvated()
    base = dict(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=0.4, overrides=0, pme_grid=grid)
    out = {}
    for arm in ("tile", "brick"):
        monkeypatch.setenv("MDX_PME_SPREAD_BRICK", "0" if arm == "tile" else "1")
        monkeypatch.setenv("MDX_PME_OVERLAP", "1" if (side and arm == "brick") else "0")
        for k, v in (("MDX_PME_BRICK_EDGE", edge), ("MDX_PME_BRICK_CAP", cap)):
            monkeypatch.delenv(k, raising=False)
            if v is not None and arm == "brick":
                monkeypatch.setenv(k, v)
        with mdx.MdState(s, MdConfig(**base)) as md:
            f = md.forces().astype(np.float64)
            e = md.energy()
            md.step(0.0005, None, 12)
            out[arm] = (f, e, md.positions().astype(np.float64), md.pme_brick_overflows())
    (ft, et, pt, ot), (fb, eb, pb, ob) = out["tile"], out["brick"]
    assert ot == 0 and (ob > 0) == (cap is not None), (ot, ob)
    assert eb["coulomb_recip"] == pytest.approx(et["coulomb_recip"], rel=5e-6)      # (fp32 mesh, sums in another order)
    scale = np.maximum(np.abs(ft).max(1), 1.0)
    assert (np.abs(fb - ft).max(1) / scale).max() < 2e-5          # fp32 sums in another order on the mesh
    assert np.abs(pb - pt).max() < 2e-4


XPASS_GRIDS = [(27, 20, 45), (50, 36, 30), (48, 24, 40), (30, 30, 30), (64, 64, 64), (20, 96, 10), (480, 16, 20)]      # (480: more than 64 KB of LDS per workgroup)
_XPASS = {}


def xpass_arms(mdx, grid, monkeypatch):
    """Both arms of MDX_PME_XPASS on S and `grid` -> {arm: (forces, energies)}, run once per mesh.  The variable is read whenever a
    handle lays its mesh out, so each arm is the code it names."""
    if grid not in _XPASS:
        S = system_s(mdx)
        out = {}
        for arm in ("0", "1"):
            monkeypatch.setenv("MDX_PME_XPASS", arm)
            with mdx.MdState(S["s"], MdConfig(overrides=0, pme_grid=grid, **BASE_S)) as md:
                assert np.array_equal(md.positions(), S["pos"])
                out[arm] = (md.forces().astype(np.float64), md.energy())
        _XPASS[grid] = out
    return _XPASS[grid]


@pytest.mark.parametrize("grid", XPASS_GRIDS)
def test_fused_x_pass_equals_the_library_transform(mdx, grid, monkeypatch):
    """pme_xpass_solve_kernel (batched 2-D hipFFT + hand-written x pass with the solve inside; radices 4, 2, 3, 5, padded rows) against
    hipFFT's 3-D plan + pme_solve_kernel on the same handle inputs: energies (incl. the virial's pressure) and every force - in the
    orthorhombic cell off the origin (system_s), where the solve's three 1 / L differ, and each arm against the numpy restatement on
    the same mesh as well: two arms that agree may still both be wrong."""
    S = system_s(mdx)
    out = xpass_arms(mdx, grid, monkeypatch)
    (f0, e0), (f1, e1) = out["0"], out["1"]
    record(f"x pass vs library transform {grid}", energy=approx_ratio(e1["coulomb_recip"], e0["coulomb_recip"], 2e-6),
           pressure=approx_ratio(e1["pressure"], e0["pressure"], 1e-5, 1e-3), force=float(np.abs(f1 - f0).max() / (2e-5 * max(1.0, np.abs(f0).max()))),
           differ_bitwise=bool((f0.astype(np.float32) != f1.astype(np.float32)).any()))
    assert e1["coulomb_recip"] == pytest.approx(e0["coulomb_recip"], rel=2e-6)
    assert e1["pressure"] == pytest.approx(e0["pressure"], rel=1e-5, abs=1e-3)
    assert np.abs(f1 - f0).max() <= 2e-5 * max(1.0, np.abs(f0).max())
    # against numpy: the bounds of test_spme_matches_numpy_restatement_and_ewald, or those of test_large_like_signed_charges_on_a_coarse_mesh
    # where an axis has more than 1.5 A per mesh point
    coarse = (S["L"] / np.asarray(grid)).max() > 1.5
    f_tol, e_rel = (3e-4, 3e-5) if coarse else (2e-4, 2e-5)
    e_ref, f_ref = numpy_reference_s(S, grid)
    for arm, (f, e) in out.items():
        err = rel_rms(f - S["f_real"], f_ref)
        record(f"x pass arm {arm} vs numpy {grid}{' (coarse)' if coarse else ''}", force_rms=err / f_tol, energy=approx_ratio(e["coulomb_recip"], e_ref, e_rel, 5e-2))
        assert err < f_tol, (arm, err)
        assert e["coulomb_recip"] == pytest.approx(e_ref, rel=e_rel, abs=5e-2), arm


def test_x_pass_arms_are_different_code(mdx, monkeypatch):
    """MDX_PME_XPASS used to be read once per process: the test above then compared a code path with itself.  A hand-written Stockham
    pass and rocFFT's do not round alike: over the seven meshes together at least one force component differs bitwise."""
    differ = {g: bool((xpass_arms(mdx, g, monkeypatch)["0"][0] != xpass_arms(mdx, g, monkeypatch)["1"][0]).any()) for g in XPASS_GRIDS}
    record("x pass arms differ bitwise on", **{"x".join(map(str, g)): v for g, v in differ.items()})
    assert any(differ.values()), "the two arms of MDX_PME_XPASS are bit for bit the same on every mesh: the variable selects nothing"


@pytest.mark.parametrize("beta,rc", [(0.25, 9.0), (0.30, 10.0), (0.34, 9.0), (0.42, 8.0), (0.50, 7.5), (0.30, 12.0)])
def test_ewald_force_table_equals_the_closed_form(mdx, beta, rc, monkeypatch):
    """The force-only Ewald flavour of the pair kernel (CM_EWALD_TAB: g(r^2) of qq (1/r^3 - g) from the bit-indexed LDS table of
    parabolas, mdx_pair_dev.h) against the closed form it replaces (erfc by A&S 7.1.26, MDX_EWALD_TABLE=0) on the same handle
    inputs, real space only, over the betas and cut-offs a caller may configure; and through a short trajectory."""
    s = systems.small_solvated(seed=17)
    cfg = MdConfig(lj_cutoff=rc, coulomb_cutoff=rc, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=beta,
                   overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED)
    out = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("MDX_EWALD_TABLE", arm)
        with mdx.MdState(s, cfg) as md:
            f = md.forces().astype(np.float64)
            md.step(0.0005, None, 20)
            out[arm] = (f, md.positions().astype(np.float64))
    (f0, p0), (f1, p1) = out["0"], out["1"]
    # per pair the table is good to 2e-6 of the pair's force and the closed form to 1.5e-7 in erfc; an atom sums ~200-400 pairs
    err = np.abs(f1 - f0).max(1) / np.maximum(np.abs(f0).max(1), 1.0)
    assert err.max() < 2e-5, err.max()
    assert np.abs(p1 - p0).max() < 1e-4


def _arm_vs_arm(e, f, e_ref, f_ref, what):
    """The arm-against-arm bounds of test_brick_spread_equals_the_tile_spread (two fp32 evaluations of the same mesh)."""
    scale = np.maximum(np.abs(f_ref).max(1), 1.0)
    record(what, energy=approx_ratio(e["coulomb_recip"], e_ref["coulomb_recip"], 5e-6), force=float((np.abs(f - f_ref).max(1) / scale).max() / 2e-5))
    assert e["coulomb_recip"] == pytest.approx(e_ref["coulomb_recip"], rel=5e-6), what
    assert (np.abs(f - f_ref).max(1) / scale).max() < 2e-5, what


def test_spme_follows_the_box_and_rejects_bad_setups(mdx, monkeypatch):
    """`md.cell = SimBox::new(..)` on a live SPME handle: theta, the brick tables and - when the default mesh size of an edge changes -
    plans and buffers follow the cell.  Held against a fresh handle created in the new cell, and against numpy."""
    from oracle import pme_ref as P
    beta = 0.4
    base = dict(lj_cutoff=7.0, coulomb_cutoff=7.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=beta)
    s = placed(systems.water_box(6, seed=3), PAD)
    lo, hi = np.asarray(s.box_lo, np.float64), np.asarray(s.box_hi, np.float64)
    # (a) an anisotropic rescaling about the origin of the coordinates - lo moves too - with the mesh given
    grid = (24, 20, 18)
    k = np.array([1.01, 1.03, 0.98])
    cfg = MdConfig(overrides=0, pme_grid=grid, **base)
    with mdx.MdState(s, cfg) as md:
        e0 = md.energy()
        pos2 = (md.positions().astype(np.float64) * k).astype(np.float32)
        md.set_positions(pos2)
        md.set_cell(tuple(lo * k), tuple(hi * k))
        e1, f1 = md.energy(), md.forces().astype(np.float64)
    assert e1["volume"] == pytest.approx(e0["volume"] * k.prod(), rel=1e-5)
    s2 = dataclasses.replace(s, pos=pos2, box_lo=tuple(lo * k), box_hi=tuple(hi * k))
    with mdx.MdState(s2, cfg) as md:
        pos, (lo2, L2) = md.positions(), cell_of(md)
        e2, f2 = md.energy(), md.forces().astype(np.float64)
    with mdx.MdState(s2, MdConfig(overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED, **base)) as md:
        assert np.array_equal(md.positions(), pos)
        f_real = md.forces().astype(np.float64)
    assert np.allclose(L2, (hi - lo) * k, rtol=1e-6)
    _arm_vs_arm(e1, f1, e2, f2, "set_cell, anisotropic: live handle vs fresh")
    q = s.charge.astype(np.float64)
    e_ref, f_ref = P.spme_recip(pos.astype(np.float64), q, lo2, L2, beta, grid, 4)
    e_x, f_x = P.excluded_pair_correction(pos.astype(np.float64), q, excluded_pairs(s), L2, beta)
    e_ref += e_x + P.ewald_self_energy(q, beta) + P.ewald_background_energy(q, L2, beta)
    err = rel_rms(f1 - f_real, f_ref + f_x)
    record("set_cell, anisotropic: live handle vs numpy", force_rms=err / 2e-4, energy=approx_ratio(e1["coulomb_recip"], e_ref, 2e-5, 5e-2))
    assert err < 2e-4, err
    assert e1["coulomb_recip"] == pytest.approx(e_ref, rel=2e-5, abs=5e-2)
    # (b) the default mesh (one point per A, rounded up to a 2-3-5-smooth size): a vacuum slab takes the z edge from 18.6 to 21.0 A and
    # its mesh from 20 to 24 points - plans, theta, brick tables and buffers are rebuilt on the live handle
    cfg = MdConfig(overrides=0, **base)
    hi3 = hi + np.array([0.0, 0.0, 2.4])
    s3 = dataclasses.replace(s, box_hi=tuple(hi3))
    for brick in ("0", "1"):
        monkeypatch.setenv("MDX_PME_SPREAD_BRICK", brick)
        with mdx.MdState(s, cfg) as md:
            pos = md.positions()
            e0 = md.energy()
            md.set_cell(tuple(lo), tuple(hi3))
            assert np.array_equal(md.positions(), pos)
            e1, f1 = md.energy(), md.forces().astype(np.float64)
        with mdx.MdState(s3, cfg) as md:
            assert np.array_equal(md.positions(), pos)
            lo3, L3 = cell_of(md)
            e2, f2 = md.energy(), md.forces().astype(np.float64)
        _arm_vs_arm(e1, f1, e2, f2, f"set_cell, mesh 20 -> 24 along z, brick spread {brick}: live handle vs fresh")
        # ... and both are the (20, 20, 24) mesh: numpy on it, the energy bound of the tests above
        e_ref, _ = P.spme_recip(pos.astype(np.float64), q, lo3, L3, beta, (20, 20, 24), 4)
        e_x, _ = P.excluded_pair_correction(pos.astype(np.float64), q, excluded_pairs(s), L3, beta)
        e_ref += e_x + P.ewald_self_energy(q, beta) + P.ewald_background_energy(q, L3, beta)
        record(f"set_cell, mesh 20 -> 24 along z, brick spread {brick}: vs numpy on (20, 20, 24)", energy=approx_ratio(e1["coulomb_recip"], e_ref, 2e-5, 5e-2))
        assert e1["coulomb_recip"] == pytest.approx(e_ref, rel=2e-5, abs=5e-2)
        assert e1["coulomb_recip"] != e0["coulomb_recip"]
    with pytest.raises(mdx.ParamError):
        mdx.MdState(s, MdConfig(lj_cutoff=7.0, coulomb_cutoff=7.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD,
                                ewald_alpha=0.4, overrides=0, pme_order=6))


@pytest.mark.parametrize("brick", ["0", "1"])
def test_large_like_signed_charges_on_a_coarse_mesh(mdx, brick, monkeypatch):
    """The LDS canvases of the charge spread accumulate in 32-bit fixed point (mdx_pme.hip, PME_FIX).  The scale is chosen per handle
    from the largest |q sqrt(k_e)| of the system: charges of +-4 e on a 2.3 A mesh - more spline-weighted charge per mesh point than
    the fixed 2^25 of round 4 could hold (it wrapped, silently, beyond +-3.5 e) - must give the mesh the fp64 restatement gives."""
    from oracle import pme_ref as P
    monkeypatch.setenv("MDX_PME_SPREAD_BRICK", brick)
    s = systems.water_box(6, seed=4)
    rng = np.random.default_rng(2)
    q = s.charge.copy()
    big = rng.choice(s.n_atoms, size=40, replace=False)
    q[big] = 4.0
    q[rng.choice(np.setdiff1d(np.arange(s.n_atoms), big), size=40, replace=False)] = -4.0
    q -= q.mean()                                   # neutral cell
    s.charge = q.astype(np.float32)
    L = float(s.box_hi[0])
    beta, grid = 0.35, (8, 8, 8)                    # 18.6 A / 8 = 2.3 A per mesh point (the smallest mesh the library takes): many atoms per point
    base = dict(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=beta)
    with mdx.MdState(s, MdConfig(overrides=_abi.OVR_LONG_RANGE_RECIP_DISABLED, **base)) as md:
        pos = md.positions()
        f_real = md.forces().astype(np.float64)
    with mdx.MdState(s, MdConfig(overrides=0, pme_grid=grid, **base)) as md:
        f_full = md.forces().astype(np.float64)
        e_full = md.energy()
    box = np.full(3, L)
    q64 = s.charge.astype(np.float64)
    e_ref, f_ref = P.spme_recip(pos.astype(np.float64), q64, (0, 0, 0), box, beta, grid, 4)
    e_x, f_x = P.excluded_pair_correction(pos.astype(np.float64), q64, excluded_pairs(s), box, beta)
    e_ref += e_x + P.ewald_self_energy(q64, beta) + P.ewald_background_energy(q64, box, beta)
    f_ref += f_x
    f_rec = f_full - f_real
    err = math.sqrt(((f_rec - f_ref) ** 2).sum(1).mean()) / math.sqrt((f_ref ** 2).sum(1).mean())
    assert err < 3e-4, f"reciprocal force rms error {err:.2e} vs the numpy SPME on the same mesh"
    assert e_full["coulomb_recip"] == pytest.approx(e_ref, rel=3e-5, abs=5e-2)
