"""`mdx_search_poses` / `MdState.search_poses`: the device search against the host loop it replaces (one `MdState.refine_poses_flex`
call per round + the move and the decision of tests/pose_search_ref.py), against `refine_poses_flex` (one round: the same bits), against
itself (a walker alone, anywhere in a batch, repeated, with optional outputs left out; a shorter search is the prefix of a longer one)
and against the fp64 oracle.

Device search against host loop: best round and the four counters equal for every walker, best coordinates within 4 ulp32(max
|coordinate|) - the bound of tests/test_gpu_pose_flex.py: the only admissible difference is an fp64 last bit of the two maths libraries
that tips one fp32 rounding -, best row, dihedral energy and score the bits `refine_poses_flex` returned for that round in the host arm
where the coordinates are its bits, else within `assert_row`'s tolerance.  A Metropolis decision whose host-arm margin |u_acc - exp(.)|
is below 1e-9 could flip on the last bit of exp: a walker with such a decision is left out, at most one of eight.

Measured on an MI355X: see DESIGN.md section 7g."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, _abi, systems
from tests import pose_flex_ref as F
from tests import pose_refine_ref as P
from tests import pose_search_ref as S
from tests.test_gpu_pose_batch import assert_row, ligand_range, oracle_row, small_configs, three_groups, usable, whole
from tests.test_pose_flex_host import ligand_case, oracle_dihedral, start_poses
from tests.test_pose_refine_host import crystal_case

pytestmark = pytest.mark.gpu

NAMES = ("best", "rows", "score", "dih", "best_round", "stats")
NO_TORSIONS = np.zeros((0, 2), np.uint32)
SUBSET = [20, 3, 11, 29, 7, 0, 16, 25]      # 8 of the ligand's 31 torsions, out of order
MOVES = (0.5, 0.15, 0.4)                    # trans_amp A, rot_amp rad, tors_amp rad
KT = 100.0                                  # kcal/mol: of the order of the round-to-round differences of S after 8 evaluations (40 - 250; section 7g)
SEED = 78                                   # (with it the 8 x 4 moves of the host-loop tests hold all three kinds, for 31 torsions and for 8)
MARGIN = 1e-9


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


@pytest.fixture(scope="module")
def lig():
    """(system, lo, hi, bonds, torsion bonds, moving sides, dihedral terms, box) of the ligand of small_complex - computed once"""
    s, lo, hi, bonds, tb, tors, terms = ligand_case()
    return s, lo, hi, bonds, tb, tors, terms, np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def same_bits(a, b, what, names=NAMES):
    for x, y, name in zip(a, b, names):
        assert np.array_equal(bits(x), bits(y)), f"{what}: {name} differ"


def host_arm(md, lo, starts, tb, tors, n_rounds, kT, ids, max_evals, dihedrals=True, moves=MOVES, seed=SEED):
    """The host loop, walker by walker -> [dict of pose_search_ref.search + trace]"""
    refine = S.flex_refiner(md, lo, 0, tb, max_evals, 0.0, 0.0, 0.0, dihedrals=dihedrals)
    out = []
    for w in range(len(starts)):
        trace = []
        res = S.search(starts[w], refine, tors, n_rounds, *moves, kT, seed, int(ids[w]), trace=trace)
        res["trace"] = trace
        out.append(res)
    return out


def counters(trace, n_rounds):
    """best round and the four counters of the first n_rounds rounds of a host-arm trace"""
    t = trace[:n_rounds]
    best = max(r for r, x in enumerate(t) if x["best"])
    return best, [sum(x["accept"] for x in t[1:]), sum(x["uphill"] for x in t[1:]), sum(not x["result"]["finite"] for x in t),
                  sum(x["result"]["evals"] for x in t)]


def against_the_host_loop(md, orc, s, cfg, g, lo, hi, dev, host, what):
    """asserts what the module's docstring states -> the walkers compared"""
    best, rows, score, dih, best_round, stats = dev
    tight = [w for w, h in enumerate(host) if h["min_margin"] < MARGIN]
    assert len(tight) <= 1, f"{what}: walkers {tight} hold a decision within {MARGIN} of its threshold"
    differ, worst, kept = 0, 0.0, [w for w in range(len(host)) if w not in tight]
    for w in kept:
        h = host[w]
        flags = [int(x["accept"]) + 2 * int(x["uphill"]) for x in h["trace"]]
        print(f"{what}, walker {w}: S per round {[round(float(x['result']['S']), 2) for x in h['trace']]}, decisions {flags}, best round {h['best_round']}, "
              f"counters {h['stats'].tolist()}, device {int(best_round[w])} {stats[w].tolist()}")
        assert int(best_round[w]) == h["best_round"], f"{what}, walker {w}: best round device {best_round[w]} host {h['best_round']}"
        assert stats[w].tolist() == h["stats"].tolist(), f"{what}, walker {w}: counters device {stats[w].tolist()} host {h['stats'].tolist()}"
        ne = int((bits(best[w]) != bits(h["pose"])).sum())
        differ += ne
        worst = max(worst, float(np.abs(best[w].astype(np.float64) - h["pose"].astype(np.float64)).max()) / ulp32(h["pose"]))
        if ne == 0:
            assert np.array_equal(bits(rows[w]), bits(h["row"])) and bits(dih[w:w + 1])[0] == bits(np.float32(h["edih"]).reshape(1))[0], f"{what}, walker {w}: row or E_dih"
            assert score[w] == h["S"], f"{what}, walker {w}: score {score[w]!r} host {h['S']!r}"
        else:
            _, gr = oracle_row(orc, s, cfg, g, 3, md.positions(), lo, hi, h["pose"], 1)
            assert_row(rows[w], h["row"].astype(np.float64), gr, f"{what}, walker {w}: row against the host arm's")
            tol = float((2e-6 * np.abs(h["row"]) + 1e-6 * gr + 1e-3).sum()) + 1e-3
            assert abs(float(dih[w]) - float(h["edih"])) <= 1e-3 and abs(score[w] - h["S"]) <= tol
    print(f"{what}: {len(kept)} walkers compared, {differ} of {sum(best[w].size for w in kept)} best coordinates not bit-equal to the host loop's, "
          f"worst difference {worst:.2f} ulp32(max |coordinate|)")
    assert worst <= 4.0, f"{what}: a best coordinate differs from the host loop's by {worst:.1f} ulp32"
    return kept


@pytest.mark.parametrize("n_tors,dihedrals", [(31, True), (8, False)])
def test_equals_the_host_loop(mdx, orc, lig, n_tors, dihedrals):
    """8 walkers, 5 rounds x 8 evaluations, all three kinds of move, kT = 100 kcal/mol"""
    s, lo, hi, bonds, tb, tors, terms, box = lig
    if n_tors == 8:
        tb = tb[SUBSET]
        tors = F.moving_sides(hi - lo, bonds, 0, tb)
    cfg = small_configs()[0]
    g = three_groups(s)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        starts = start_poses(s, md.positions(), lo, hi, lig[5])[:8]
        what = f"{n_tors} torsions, dihedral terms {'on' if dihedrals else 'off'}"
        dev = md.search_poses(lo, starts, 0, tb, 5, *MOVES, KT, SEED, 8, 0.0, 0.0, 0.0, dihedrals=dihedrals)
        assert dev[0].shape == starts.shape and dev[0].dtype == np.float32 and dev[1].shape == (8, 3) and dev[2].shape == (8,) and dev[2].dtype == np.float64
        assert dev[3].shape == (8,) and dev[4].shape == (8,) and dev[5].shape == (8, 4) and dev[5].dtype == np.uint32
        host = host_arm(md, lo, starts, tb, tors, 5, KT, np.arange(8), 8, dihedrals)
        kept = against_the_host_loop(md, orc, s, cfg, g, lo, hi, dev, host, what)
        st = dev[5][kept]
        kinds = {x["move"]["kind"] for w in kept for x in host[w]["trace"][1:]}
        assert kinds == {S.TRANSLATION, S.ROTATION, S.TORSION}, kinds
        assert (st[:, 3] == 40).all() and (st[:, 2] == 0).all()
        assert st[:, 0].sum() > 0 and (st[:, 0] < 4).any(), "the runs should hold accepted and rejected rounds"
        assert (dev[3] > 0).all() if dihedrals else (dev[3] == 0).all()


def test_the_prefix_property(mdx, lig):
    """R = 3 against R = 5: a walker whose best of five rounds lies in rounds 0 .. 2 has that best after three; the counters of the
    three-round run are the host arm's cut at three."""
    s, lo, hi, bonds, tb, tors, terms, box = lig
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(three_groups(s), 3)
        starts = start_poses(s, md.positions(), lo, hi, tors)[:8]
        args = (*MOVES, KT, SEED, 8, 0.0, 0.0, 0.0)
        five = md.search_poses(lo, starts, 0, tb, 5, *args)
        three = md.search_poses(lo, starts, 0, tb, 3, *args)
        early = five[4] <= 2
        print(f"best rounds of five {five[4].tolist()}, of three {three[4].tolist()}")
        assert early.any(), "some walker should have its best in the first three rounds"
        same_bits([a[early] for a in three[:5]], [a[early] for a in five[:5]], "walkers with their best in rounds 0 .. 2", NAMES[:5])
        assert (three[2] >= five[2]).all() and (three[4][~early] <= 2).all()
        host = host_arm(md, lo, starts, tb, tors, 5, KT, np.arange(8), 8)
        safe = [w for w, h in enumerate(host) if h["min_margin"] >= MARGIN]
        assert len(safe) >= 7
        for w in safe:
            for n, run in ((3, three), (5, five)):
                br, st = counters(host[w]["trace"], n)
                assert int(run[4][w]) == br and run[5][w].tolist() == st, (w, n, run[4][w], run[5][w].tolist(), br, st)


def test_one_round_is_refine_poses_flex_bit_for_bit(mdx, lig):
    s, lo, hi, bonds, tb, tors, terms, box = lig
    g = three_groups(s)
    for cfg in small_configs():
        with mdx.MdState(s, cfg) as md:
            md.set_energy_groups(g, 3)
            poses = start_poses(s, md.positions(), lo, hi, tors)
            for n_t, evals, dihedrals in ((31, 12, True), (8, 5, False)):
                t = tb if n_t == 31 else tb[SUBSET]
                flex = md.refine_poses_flex(lo, poses, 0, t, evals, 0.0, 0.0, 0.0, dihedrals=dihedrals)
                best, rows, score, dih, best_round, stats = md.search_poses(lo, poses, 0, t, 1, *MOVES, KT, SEED, evals, 0.0, 0.0, 0.0, dihedrals=dihedrals)
                same_bits((best, rows, dih), (flex[0], flex[1], flex[4]), f"coulomb mode {cfg.coulomb_mode}, {n_t} torsions", ("best", "rows", "dih"))
                assert (best_round == 0).all() and np.array_equal(stats, np.stack([np.zeros(16), np.zeros(16), np.zeros(16), flex[7]], 1).astype(np.uint32))
                S_ref = np.array([sum((float(v) for v in r), 0.0) + float(e) for r, e in zip(flex[1], flex[4])])
                assert np.array_equal(score, S_ref)


def _raw(mdx, md, lo, starts, tb, opts, ids=None, root=0, keep=(True,) * 5, n_groups=3, no_out=False, no_opts=False, count=None):
    """The C entry point itself, with any of the five optional outputs left out -> (rc, message, the six output buffers)"""
    lib = mdx.load_library()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    p = np.ascontiguousarray(starts, np.float32)
    tb = np.ascontiguousarray(tb, np.uint32).reshape(-1, 2)
    n, T = p.shape[0], tb.shape[0]
    o = [np.full((n, max(p.shape[1], 1), 3), -7.0, np.float32), np.full((n, max(n_groups, 1)), -7.0, np.float32), np.full(n, -7.0, np.float64),
         np.full(n, -7.0, np.float32), np.full(n, 77, np.uint32), np.full((n, 4), 77, np.uint32)]
    kinds = {np.dtype(np.uint32): up, np.dtype(np.float32): fp, np.dtype(np.float64): C.POINTER(C.c_double), np.dtype(np.uint64): C.POINTER(C.c_uint64)}
    ptr = lambda a, on=True: (a.ctypes.data_as(kinds[a.dtype]) if on else None)
    ids = None if ids is None else np.ascontiguousarray(ids, np.uint64)
    rc = lib.mdx_search_poses(md._h, lo, p.shape[1] if count is None else count, n, ptr(p), None if ids is None else ptr(ids), root, T, ptr(tb, T > 0),
                              None if no_opts else C.byref(opts), ptr(o[0], not no_out), ptr(o[1], keep[0]), n_groups, ptr(o[2], keep[1]),
                              ptr(o[3], keep[2]), ptr(o[4], keep[3]), ptr(o[5], keep[4]))
    return rc, lib.mdx_last_error().decode(), o


def _opts(n_rounds=2, moves=MOVES, kT=KT, evals=4, seed=SEED, **kw):
    return _abi.CSearchOpts(n_rounds, *moves, kT, seed, _abi.CFlexOpts(evals, kw.get("f_tol", 0.0), 0.0, kw.get("tors_tol", 0.0), kw.get("h_start", 0.0),
                                                                      kw.get("h_max", 0.0), kw.get("flags", 1)))


def test_a_walker_gives_the_same_bits_anywhere(mdx):
    """One molecule of the crystal (12 atoms, five torsions), 2 rounds x 4 evaluations: the walker with stream id 7 alone, at positions 0,
    255 and 256 of a batch of 257 - either side of the chunk boundary -, repeated, without stream ids where its place is its id, and
    with any subset of the optional outputs left out."""
    s, cfg, g, lo, hi = crystal_case()
    bonds = F.local_bonds(s, lo, hi)
    tb = F.rotatable_bonds(hi - lo, bonds, 0)
    tors = F.moving_sides(hi - lo, bonds, 0, tb)
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 2)
        start = whole(s, md.positions()[lo:hi])
        starts = F.flex_poses(start, tors, 257, 1, 0.3, max_rot=0.3, max_tr=1.0)
        ids = np.arange(1000, 1257, dtype=np.uint64)
        for k in (0, 255, 256):
            starts[k], ids[k] = starts[9], 7
        args = (2, 1.0, 0.3, 0.5, 5.0, SEED, 4, 0.0, 0.0, 0.0)
        batch = md.search_poses(lo, starts, 0, tb, *args, streams=ids)
        alone = md.search_poses(lo, np.ascontiguousarray(starts[9:10]), 0, tb, *args, streams=np.array([7], np.uint64))
        for k in (0, 255, 256):
            same_bits([a[k:k + 1] for a in batch], alone, f"stream 7 at position {k} of 257 and alone")
        same_bits(batch, md.search_poses(lo, starts, 0, tb, *args, streams=ids), "the same call twice")
        # no stream ids: walker w draws from stream w
        eight = md.search_poses(lo, np.ascontiguousarray(np.stack([starts[9]] * 8)), 0, tb, *args)
        same_bits([a[7:8] for a in eight], alone, "walker 7 without stream ids")
        print(f"eight streams from one start: best rounds {eight[4].tolist()}, counters {eight[5].tolist()}")
        assert (batch[5][:, 3] >= 2).all() and (batch[5][:, 3] <= 8).all()
        # the C entry point, with optional outputs left out
        o = _opts(2, (1.0, 0.3, 0.5), 5.0, 4)
        sub = np.ascontiguousarray(starts[250:257])
        rc, msg, full = _raw(mdx, md, lo, sub, tb, o, ids=ids[250:257], n_groups=2)
        assert rc == 0, msg
        same_bits(full, [a[250:257] for a in batch], "the C entry point")
        for keep in ((False,) * 5, (True, False, True, False, True), (False, True, False, True, False)):
            rc, msg, part = _raw(mdx, md, lo, sub, tb, o, ids=ids[250:257], n_groups=2, keep=keep)
            assert rc == 0 and np.array_equal(bits(part[0]), bits(full[0])), "leaving optional outputs out changes best_out"
            for j, on in enumerate(keep):
                if on:
                    assert np.array_equal(bits(part[1 + j]), bits(full[1 + j])), NAMES[1 + j]
                else:
                    assert (part[1 + j] == (77 if part[1 + j].dtype == np.uint32 else -7.0)).all(), NAMES[1 + j]


def test_the_best_is_no_worse_than_the_refinement_and_the_oracle_agrees(mdx, orc, lig):
    s, lo, hi, bonds, tb, tors, terms, box = lig
    g = three_groups(s)
    cfg = small_configs()[0]
    vsum = float((2.0 * np.abs(terms[1])).sum())
    with mdx.MdState(s, cfg) as md:
        md.set_energy_groups(g, 3)
        pos = md.positions()
        starts = start_poses(s, pos, lo, hi, tors)[:8]
        args = (*MOVES, KT, SEED, 8, 0.0, 0.0, 0.0)
        one = md.search_poses(lo, starts, 0, tb, 1, *args)
        best, rows, score, dih, best_round, stats = md.search_poses(lo, starts, 0, tb, 5, *args)
        print(f"score after one round {np.round(one[2], 2).tolist()}, best of five {np.round(score, 2).tolist()}, best rounds {best_round.tolist()}")
        assert (score <= one[2]).all() and (score < one[2]).any() and np.isfinite(score).all()
        assert np.array_equal(score, np.array([sum((float(v) for v in r), 0.0) + float(e) for r, e in zip(rows, dih)]))
        keep = usable(s, pos, lo, hi, best)
        for k in np.flatnonzero(keep)[:4]:
            ro, gr = oracle_row(orc, s, cfg, g, 3, pos, lo, hi, best[k], 1)
            assert_row(rows[k], ro, gr, f"best pose of walker {k}")
            Eo = oracle_dihedral(orc, s, cfg, pos, lo, hi, best[k])[0]
            assert abs(float(dih[k]) - Eo) <= 2.0 ** -23 * abs(Eo) + 1e-9 * vsum, (k, dih[k], Eo)


def test_the_handle_is_untouched(mdx, lig):
    """The twin test of tests/test_gpu_pose_flex.py::test_the_handle_is_untouched with search_poses in place of refine_poses_flex"""
    s, lo, hi, bonds, tb, tors, terms, box = lig
    g = three_groups(s)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)
    with mdx.MdState(s, cfg) as md, mdx.MdState(s, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(g, 3)
            m.step(0.0005, None, 4)
        e0, x0, f0, v0 = md.energy(), md.positions(), md.forces(), md.velocities()
        rebuilds = md.stats()["rebuild_count"]
        starts = start_poses(s, x0, lo, hi, tors)
        md.search_poses(lo, starts, 0, tb, 3, *MOVES, KT, SEED, 6, 0.0, 0.0, 0.0)
        assert md.stats()["rebuild_count"] == rebuilds, "searching poses must not rebuild the list of a ready handle"
        e1, x1, f1, v1 = md.energy(), md.positions(), md.forces(), md.velocities()
        atomic_sums = ("kinetic", "temperature", "pressure", "bond", "angle", "dihedral", "lj14", "coulomb14", "potential_bonded", "potential_nonbonded",
                       "potential")
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


def test_a_non_finite_start(mdx, lig):
    """A start with an atom on top of a receptor atom: round 0 ends NONFINITE after one evaluation.  Alone in a search of one round the
    best is the input and the score +inf; in a longer search the first finite round replaces it, as in the host arm; the other walkers
    keep their bits; the call returns MDX_OK."""
    s, lo, hi, bonds, tb, tors, terms, box = lig
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(three_groups(s), 3)
        pos = md.positions()
        starts = start_poses(s, pos, lo, hi, tors)[:4]
        bad = starts.copy()
        bad[2, 0] = pos[3]
        with pytest.raises(mdx.BlowUpError):
            md.pose_forces(lo, np.ascontiguousarray(bad[2:3]))
        args = (*MOVES, KT, SEED, 6, 0.0, 0.0, 0.0)
        one = md.search_poses(lo, bad, 0, tb, 1, *args)
        assert one[2][2] == math.inf and one[4][2] == 0 and one[5][2].tolist() == [0, 0, 1, 1] and np.array_equal(bits(one[0][2]), bits(bad[2]))
        clean = md.search_poses(lo, starts, 0, tb, 4, *args)
        out = md.search_poses(lo, bad, 0, tb, 4, *args)
        others = np.arange(4) != 2
        same_bits([o[others] for o in out], [c[others] for c in clean], "the rest of the batch")
        host = host_arm(md, lo, bad[2:3], tb, tors, 4, KT, [2], 6)[0]
        fin = [x["result"]["finite"] for x in host["trace"]]
        print(f"non-finite start: finite rounds {fin}, host best round {host['best_round']} S {host['S']}, device {out[4][2]} {out[2][2]} {out[5][2].tolist()}")
        assert not fin[0] and host["min_margin"] >= MARGIN
        assert int(out[4][2]) == host["best_round"] and out[5][2].tolist() == host["stats"].tolist()
        if any(fin):
            assert out[4][2] == fin.index(True) or host["best_round"] > fin.index(True)
            assert math.isfinite(out[2][2]) and out[2][2] == host["S"] and np.abs(out[0][2].astype(np.float64) - host["pose"]).max() <= 4 * ulp32(host["pose"])
        else:
            assert out[2][2] == math.inf and np.array_equal(bits(out[0][2]), bits(bad[2]))


def _refused(mdx, md, lo, starts, tb, match, opts=None, **kw):
    rc, msg, o = _raw(mdx, md, lo, starts, tb, opts if opts is not None else _opts(), **kw)
    assert rc == -1, (rc, msg)
    assert all((a == -7.0).all() for a in o[:4]) and (o[4] == 77).all() and (o[5] == 77).all(), "a refused call must leave its outputs untouched"
    assert match in msg, msg


def test_refusals(mdx, lig):
    s, lo, hi, bonds, tb, tors, terms, box = lig
    g = three_groups(s)
    n = hi - lo
    with mdx.MdState(s, small_configs()[0]) as md:
        pos = md.positions()
        starts = np.stack([pos[lo:hi]] * 2)
        _refused(mdx, md, lo, starts, tb, "no energy groups")
        md.set_energy_groups(g, 3)
        assert md.search_poses(lo, starts, 0, tb, 2, *MOVES, KT, SEED, 2, 0.0, 0.0, 0.0)[0].shape == (2, n, 3)
        # the search's own
        _refused(mdx, md, lo, starts, tb, "n_rounds", opts=_opts(0))
        _refused(mdx, md, lo, starts, tb, "n_rounds", opts=_opts(_abi.SEARCH_MAX_ROUNDS + 1))
        _refused(mdx, md, lo, starts, tb, "65536", opts=_opts(1024, evals=65))
        _refused(mdx, md, lo, starts, tb, "negative", opts=_opts(moves=(-0.5, 0.1, 0.1)))
        _refused(mdx, md, lo, starts, tb, "not finite", opts=_opts(moves=(0.5, float("nan"), 0.1)))
        _refused(mdx, md, lo, starts, tb, "not finite", opts=_opts(moves=(0.5, 0.1, float("inf"))))
        _refused(mdx, md, lo, starts, tb, "negative", opts=_opts(kT=-1.0))
        _refused(mdx, md, lo, starts, tb, "not finite", opts=_opts(kT=float("nan")))
        _refused(mdx, md, lo, starts, tb, "pi", opts=_opts(moves=(0.5, 0.1, 3.2)))
        _refused(mdx, md, lo, starts, tb, "no move", opts=_opts(moves=(0.0, 0.0, 0.0)))
        _refused(mdx, md, lo, starts, NO_TORSIONS, "no move", opts=_opts(moves=(0.0, 0.0, 0.5)))
        # those of mdx_refine_poses_flex
        _refused(mdx, md, lo, starts, tb, "null", no_out=True)
        _refused(mdx, md, lo, starts, tb, "null", no_opts=True)
        _refused(mdx, md, lo, starts, tb, "n_groups", n_groups=2)
        _refused(mdx, md, lo - 1, np.stack([pos[lo - 1:hi]] * 2), NO_TORSIONS, "exactly one energy group")
        _refused(mdx, md, lo, np.zeros((2, 1, 3), np.float32), NO_TORSIONS, "count", count=0)
        _refused(mdx, md, 0, np.zeros((1, 257, 3), np.float32), NO_TORSIONS, "count")
        _refused(mdx, md, s.n_atoms - 10, starts, NO_TORSIONS, "out of bounds")
        bad = starts.copy()
        bad[1, 7, 2] = np.nan
        _refused(mdx, md, lo, bad, tb, "non-finite")
        _refused(mdx, md, lo, starts, tb, "max_evals", opts=_opts(evals=0))
        _refused(mdx, md, lo, starts, tb, "max_evals", opts=_opts(1, evals=_abi.REFINE_MAX_EVALS_CAP + 1))
        _refused(mdx, md, lo, starts, tb, "negative", opts=_opts(f_tol=-1.0))
        _refused(mdx, md, lo, starts, tb, "not finite", opts=_opts(tors_tol=float("nan")))
        _refused(mdx, md, lo, starts, tb, "h_start", opts=_opts(h_start=0.3, h_max=0.25))
        _refused(mdx, md, lo, starts, tb, "flag", opts=_opts(flags=3))
        _refused(mdx, md, lo, starts, np.tile(tb[:1], (33, 1)), "MDX_POSE_MAX_TORSIONS")
        _refused(mdx, md, lo, starts, tb, "root", root=n)
        a, b = int(tb[4][0]), int(tb[4][1])
        _refused(mdx, md, lo, starts, [(a, n)], "torsion 0 names an atom index")
        _refused(mdx, md, lo, starts, [tb[0], tb[1], (b, a), tb[4]], "torsion 3: the bond is listed twice")
        deg = np.bincount(bonds.reshape(-1), minlength=n)
        leaf = next(p for p in bonds if deg[p[0]] == 1 or deg[p[1]] == 1)
        _refused(mdx, md, lo, starts, [tb[0], leaf], "torsion 1: one side of the bond is a single atom")
        # n_walkers == 0 succeeds and does nothing
        out = np.full(18, -7.0, np.float32)
        o = out.ctypes.data_as(C.POINTER(C.c_float))
        assert mdx.load_library().mdx_search_poses(md._h, lo, n, 0, None, None, 0, 0, None, None, o, o, 3, None, o, None, None) == 0 and (out == -7.0).all()
        md.configure_alchemical_window(1, 0.5)      # the ligand is molecule 1
        _refused(mdx, md, lo, starts, tb, "alchemical")


def test_refused_on_a_decomposed_handle(mdx, lig):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    g = three_groups(s)
    lo, hi = ligand_range(s)
    tb = lig[4]
    starts = np.stack([np.asarray(s.pos, np.float32)[lo:hi]] * 2)
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
                    _refused(mdx, md, lo, starts, tb, "decomposed")
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]
