"""`mdx_set_solute_copies` / `mdx_solubility_mixing` / `mdx_snapshot_read_solubility` through `MdState` on the device, against the numpy
restatement of the rule (tests/mixing_ref.py) on the positions the handle holds.

Per-atom sums: both sides add in fp64; the device forms every term in fp32.  The bound on a sum is computed from the case itself
(mixing_ref.sum_bounds: the case's own coordinates, minimum-image distances and x = d2 / 2 sigma^2 of every term; DESIGN.md section 7k
derives it), never tuned.  The bound it implies for local_mixing is held at or below 1e-4, a tenth of the reference's own tolerance
(tests/test_mixing_host.py holds that without a GPU).  Every case prints its worst deviation as a fraction of its bound.  The three
aggregation fractions are bit-equal to the fp32 ratios of the same integers; the other fields lie within the bounds that follow from the
sums (mixing_ref.field_bounds).  As measured on an MI355X: sums within 0.02-0.13 of their bounds (relative 3e-8 ... 6.5e-7), bound on
local_mixing 1.2e-7 ... 1.4e-6, its deviation 0 in every case.

The reference's two pinned vectors (an 80,000 A cube) run on the device in that very cell: a handle of 8 + 8 x 3 atoms in it can be
built - the cell grid is capped, not refused."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, _abi, systems
from tests import mixing_cases as mc
from tests import mixing_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def open_case(mdx, case, nb_variant=0):
    md = mdx.MdState(case.system(), case.cfg(nb_variant))
    md.set_water_layout(case.water_first, case.n_waters, 3)
    md.set_solute_copies(0, case.copies, case.apc, case.sel)
    return md


def restate(case, pos, lo, hi):
    sol, wat = case.split(pos)
    want, ex = ref.diagnostics(sol, wat, lo, hi, full=True)
    bounds = ref.sum_bounds(sol, wat, lo, hi)
    fb = ref.field_bounds(want, ref.local_mixing_bound(ex["sums"], bounds, sol.shape[0], sol.shape[1], len(wat)))
    return want, ex, bounds, fb


def check_fields(got, want, fb, what=""):
    for f in ("largest_cluster_fraction", "contacted_fraction", "contact_pair_fraction"):
        assert np.float32(got[f]).view(np.uint32) == np.float32(want[f]).view(np.uint32), (what, f, got[f], want[f])
    worst = 0.0
    for f in ref.FIELDS:
        err = abs(float(got[f]) - float(want[f]))
        assert err <= fb[f], (what, f, got[f], want[f], fb[f])
        if fb[f] > 0:
            worst = max(worst, err / fb[f])
    return worst


def field_bits(d):
    return [np.float32(d[f]).view(np.uint32) for f in ref.FIELDS]


# ---- per-atom sums and the ten fields against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_sums_and_fields_against_the_restatement(mdx, case):
    with open_case(mdx, case) as md:
        md.set_positions(case.system().pos)      # (a new handle holds its atoms wrapped into the cell; an upload is kept as it is)
        pos = md.positions()
        lo, hi = md.cell()
        got, sums = md.solubility(atom_sums=True)
    assert np.array_equal(pos, case.system().pos)      # nothing has wrapped or moved the atoms: the device read what was uploaded
    want, ex, bounds, fb = restate(case, pos, lo, hi)
    assert sums.shape == ex["sums"].shape
    err = np.abs(sums - ex["sums"])
    frac = float((err / np.maximum(bounds, 1e-300)).max())
    rel = float((err / np.maximum(ex["sums"], 1e-300))[ex["sums"] > 1e-6].max()) if (ex["sums"] > 1e-6).any() else 0.0
    print(f"\n[mixing] {case.name}: rows {sums.shape[0]}, worst sum deviation {frac:.3f} of its bound (relative {rel:.2e}), "
          f"local_mixing bound {fb['local_mixing']:.2e}, deviation {abs(float(got['local_mixing']) - float(want['local_mixing'])):.2e}")
    assert (err <= bounds).all(), frac
    assert fb["local_mixing"] <= 1e-4
    check_fields(got, want, fb, case.name)
    if case.sharp:
        assert 0.02 < float(got["local_mixing"]) < 0.98


# ---- the reference's two pinned vectors, in the reference's own 80,000 A cell -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["mixed", "split"])
def test_pinned_vectors_on_the_device(mdx, which):
    _, _, lo, hi, want = mc.pinned(which)
    with mdx.MdState(mc.pinned_system(which), MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.0)) as md:
        md.set_water_layout(8, 8, 3)
        md.set_solute_copies(0, 8, 1)
        l, h = md.cell()
        assert np.array_equal(l, np.float32(lo)) and np.array_equal(h, np.float32(hi))
        got = md.solubility()
    assert abs(float(got["score"]) - want) <= mc.PINNED_EPS, got
    assert abs(float(got["local_mixing"]) - want) <= mc.PINNED_EPS and float(got["aggregation_factor"]) == 1.0
    assert float(got["solute_dispersion"]) == 1.0 and float(got["contacted_fraction"]) == 0.0


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------------------
CASE = mc.BY_NAME["cubic30_clustered"]


def test_two_calls_give_equal_bits(mdx):
    with open_case(mdx, CASE) as md:
        a, sa = md.solubility(atom_sums=True)
        b, sb = md.solubility(atom_sums=True)
        assert field_bits(a) == field_bits(b) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
        md.step(0.0005, None, 4)      # ... and in slot order, behind the step loop
        c, sc = md.solubility(atom_sums=True)
        d, sd = md.solubility(atom_sums=True)
        assert field_bits(c) == field_bits(d) and np.array_equal(sc.view(np.uint64), sd.view(np.uint64))
        assert not np.array_equal(sa, sc)
        want, ex, bounds, fb = restate(CASE, md.positions(), *md.cell())
        assert (np.abs(sc - ex["sums"]) <= bounds).all()
        check_fields(c, want, fb, "after 4 steps")


def test_the_handle_continues_bit_for_bit(mdx):
    """20 steps with and without calls in between, under the pair kernel with fixed-order force sums (as the twin tests of the pose
    passes run): positions and velocities bit for bit"""
    with open_case(mdx, CASE, nb_variant=2) as md:
        for _ in range(4):
            md.step(0.0005, None, 5)
        plain_p, plain_v = md.positions(), md.velocities()
    with open_case(mdx, CASE, nb_variant=2) as md:
        md.solubility()
        for _ in range(4):
            md.step(0.0005, None, 5)
            md.solubility(atom_sums=True)
        p, v = md.positions(), md.velocities()
    assert np.array_equal(p.view(np.uint32), plain_p.view(np.uint32)) and np.array_equal(v.view(np.uint32), plain_v.view(np.uint32))


def test_set_box_to_a_smaller_cell_follows_the_new_clipping(mdx):
    with open_case(mdx, CASE) as md:
        before = md.solubility()
        md.set_cell((4.5, 4.5, 4.5), (25.5, 25.5, 25.5))      # 21 A: sigma = 10 becomes 9.45
        lo, hi = md.cell()
        got, sums = md.solubility(atom_sums=True)
        want, ex, bounds, fb = restate(CASE, md.positions(), lo, hi)
    assert ref.sigmas(ref.cell_edges(lo, hi))[2] < 10.0
    assert (np.abs(sums - ex["sums"]) <= bounds).all()
    check_fields(got, want, fb, "21 A cell")
    assert field_bits(got) != field_bits(before)
    # the restatement with the widths of the old cell is NOT what the device returned
    old = ref.diagnostics(*CASE.split(CASE.system().pos), (0, 0, 0), (30, 30, 30))
    assert abs(float(old["local_mixing"]) - float(got["local_mixing"])) > 10 * fb["local_mixing"]


def test_snapshots_carry_the_record(mdx):
    with open_case(mdx, CASE) as md:
        md.set_snapshot_cadence(10)
        md.step(0.0005, None, 20)
        live = md.solubility()
        snaps = md.snapshots
        lo, hi = md.cell()
        assert [s["step"] for s in snaps] == [10, 20]
        for s in snaps:
            want, _, _, fb = restate(CASE, s["all_posits"], lo, hi)
            check_fields(s["solubility"], want, fb, f"snapshot at step {s['step']}")
        assert field_bits(snaps[1]["solubility"]) == field_bits(live)
        assert field_bits(snaps[0]["solubility"]) != field_bits(live)
        # a snapshot taken while the layout is off carries none
        md.set_solute_copies(0, 0, 0)
        md.step(0.0005, None, 10)
        out = _abi.CSolubility(*([7.0] * 10))
        lib = mdx.load_library()
        assert lib.mdx_snapshot_read_solubility(md._h, 2, C.byref(out)) == _abi.MDX_EPARAM
        assert b"without a solute layout" in lib.mdx_last_error() and [getattr(out, f) for f in ref.FIELDS] == [7.0] * 10
        assert lib.mdx_snapshot_read_solubility(md._h, 1, C.byref(out)) == _abi.MDX_OK and out.score == live["score"]


def refused(mdx, md, match):
    """mdx_solubility_mixing is refused with MDX_EPARAM, says why, and leaves out and atom_sums untouched"""
    lib = mdx.load_library()
    out = _abi.CSolubility(*([7.0] * 10))
    sums = np.full(6 * 400, 7.0)
    assert lib.mdx_solubility_mixing(md._h, C.byref(out), sums.ctypes.data_as(C.POINTER(C.c_double))) == _abi.MDX_EPARAM
    assert match in lib.mdx_last_error().decode(), lib.mdx_last_error()
    assert [getattr(out, f) for f in ref.FIELDS] == [7.0] * 10 and (sums == 7.0).all()


def test_refusals_leave_out_untouched(mdx):
    P = mdx.ParamError
    s = CASE.system()
    n_sol, n_w = CASE.water_first, CASE.n_waters
    with mdx.MdState(s, CASE.cfg()) as md:
        refused(mdx, md, "no solute layout")
        with pytest.raises(P, match="no water layout"):
            md.set_solute_copies(0, CASE.k, mc.APC)
        md.set_water_layout(n_sol, n_w, 3)
        for args, why in (((0, CASE.k, mc.APC + 1), "overlaps the water range"), ((n_sol - 1, 1, 2), "overlaps the water range"),
                          ((n_sol + 3 * n_w - 1, 1, 2), "beyond the atom array"), ((0, CASE.k, mc.APC, [0, 12]), "not an index inside a copy"),
                          ((0, CASE.k, mc.APC, [3, 5, 3]), "repeats an index"), ((0, CASE.k, 0), "atoms_per_copy"),
                          ((0, 4097, 1), "n_copies")):
            with pytest.raises(P, match=why):
                md.set_solute_copies(*args)
            refused(mdx, md, "no solute layout")      # a refused layout is not set
        md.set_solute_copies(0, CASE.k, mc.APC)
        md.solubility()
        md.set_water_layout(n_sol - 6, n_w + 2, 3)      # the water layout moved onto the solute behind the layout's back
        refused(mdx, md, "overlaps the water range")
        md.set_water_layout(0, 0, 3)
        refused(mdx, md, "no water layout")
        md.set_water_layout(n_sol, n_w, 3)
        md.solubility()
        md.set_solute_copies(0, 0, 0)
        refused(mdx, md, "no solute layout")
    with mdx.MdState(systems.lig50(), MdConfig(lj_cutoff=0, coulomb_cutoff=0)) as md:      # vacuum: the score needs a cell
        md.set_water_layout(44, 2, 3)
        with pytest.raises(P, match="non-periodic"):
            md.set_solute_copies(0, 2, 12)
        refused(mdx, md, "non-periodic")


def test_refused_on_a_decomposed_handle(mdx):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    first_w = int(s.mol_start[2])
    world = 2
    fabric = Fabric(world)
    errs = []

    def run(rank):
        try:
            with MdState(s, cfg) as md:
                md.set_water_layout(first_w, (s.n_atoms - first_w) // 3, 3)
                md.set_solute_copies(0, 10, 12)
                md.comm_init_fabric(fabric, rank)
                refused(mdx, md, "decomposed")
                with pytest.raises(mdx.ParamError, match="decomposed"):
                    md.set_solute_copies(0, 5, 12)
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]


def blown_up(mdx, case, atom):
    """A handle whose atom `atom` holds a non-finite coordinate.  Uploads refuse NaN and inf, so the state is made the way a run makes
    it: the atom is sent off at 3e38 A/ps and one step of 4 ps overflows its coordinate.  -> (md, non-finite atoms bool [N])"""
    md = open_case(mdx, case)
    v = np.zeros((case.system().n_atoms, 3), np.float32)
    v[atom, 0] = 3.0e38
    md.set_velocities(v)
    try:
        md.step(4.0, None, 1)
    except mdx.BlowUpError:
        pass
    bad = ~np.isfinite(md.positions()).all(1)
    assert bad[atom]
    return md, bad


NAN_CASE = mc.BY_NAME["rows63_orth21"]      # sel = (0, 2, 3, 5, 8, 9, 11)


def _read_by_the_call(case):
    m = np.zeros(case.system().n_atoms, bool)
    for c in range(case.copies):
        m[[c * case.apc + k for k in (case.sel if case.sel is not None else range(case.apc))]] = True
    m[case.water_first + 3 * np.arange(case.n_waters)] = True
    return m


@pytest.mark.parametrize("atom", [2 * mc.APC + 3, NAN_CASE.water_first + 3 * 7], ids=["selected_atom", "water_oxygen"])
def test_a_non_finite_coordinate_is_a_blow_up(mdx, atom):
    md, bad = blown_up(mdx, NAN_CASE, atom)
    with md:
        lib = mdx.load_library()
        out = _abi.CSolubility(*([7.0] * 10))
        sums = np.full(6 * 63, 7.0)
        assert lib.mdx_solubility_mixing(md._h, C.byref(out), sums.ctypes.data_as(C.POINTER(C.c_double))) == _abi.MDX_ENAN
        assert [getattr(out, f) for f in ref.FIELDS] == [7.0] * 10 and (sums == 7.0).all()
        with pytest.raises(mdx.BlowUpError, match="non-finite"):
            md.solubility()


@pytest.mark.parametrize("atom", [2 * mc.APC + 1, NAN_CASE.water_first + 3 * 7 + 1], ids=["unselected_atom", "water_hydrogen"])
def test_a_non_finite_coordinate_the_call_does_not_read(mdx, atom):
    md, bad = blown_up(mdx, NAN_CASE, atom)
    with md:
        assert not (bad & _read_by_the_call(NAN_CASE)).any()
        got = md.solubility()
        assert all(np.isfinite(float(got[f])) for f in ref.FIELDS)
