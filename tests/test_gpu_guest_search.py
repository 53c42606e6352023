"""`mdx_search_guests` / `MdState.search_guests`: the pose search of a library of guest ligands on the device.

Against the host loop it replaces - `pose_search_ref.search` per walker with one `MdState.refine_guests_flex` call per round behind it
(tests/guest_search_cases.py) - by the criteria of tests/test_gpu_pose_search.py: best round and the four counters equal for every
walker, best coordinates within 4 ulp32(max |coordinate|), best row, dihedral energy and score the bits `refine_guests_flex` returned
for that round in the host arm where the coordinates are its bits, else within `assert_row`'s bound.  A walker whose host-arm Metropolis
margin |u - exp(.)| is below 1e-9 is left out, at most one of eight.  Against `refine_guests_flex`: one round is the same bits, best
walker and score included.  Against itself: a (ligand, walker) gives the same bits alone, in the library forward and reversed; a shorter
search is the prefix of a longer one; the per-ligand pick is the host argmin of the walkers' scores.  No tolerance of its own: all are
imported."""
import threading

import numpy as np
import pytest

from molchanica_amd import GuestFlex, GuestLigand, MdConfig, _abi, systems
from tests import guest_cases as gc
from tests import guest_flex_cases as fc
from tests import guest_search_cases as sc
from tests import pose_search_ref as S
from tests.test_gpu_pose_search import KT, MARGIN, MOVES, SEED, bits, counters

pytestmark = pytest.mark.gpu

t = gc.pose_batch_module()
NAMES = sc.NAMES


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


def row_sum(rows, dih):
    """S of every walker as a host gets it from the returned row and dihedral energy: the columns in order, then E_dih"""
    return np.array([sum((float(v) for v in r), 0.0) + float(e) for r, e in zip(rows, dih)])


# ---- 1: against the host loop it replaces ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tors,dihedrals", [(31, True), (8, False)])
def test_equals_the_host_loop(mdx, orc, n_tors, dihedrals):
    """The small complex (R + the guest's pose = S), 8 walkers, 5 rounds x 8 evaluations, all three kinds of move, kT = 100 kcal/mol"""
    S_, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    flex = fc.small_flex(n_tors)
    cfg = t.small_configs()[0]
    eight = lig.with_poses(np.ascontiguousarray(lig.poses[:8]))
    guest_sys = gc.only_molecules(S_, [1])
    what = f"{n_tors} torsions, dihedral terms {'on' if dihedrals else 'off'}"
    with mdx.MdState(R, cfg) as md:
        md.set_energy_groups(gR, 2)
        dev = [v[0] for v in md.search_guests([eight], [flex], 5, *MOVES, KT, SEED, 8, 0.0, 0.0, 0.0, dihedrals=dihedrals)]
        assert dev[0].shape == eight.poses.shape and dev[0].dtype == np.float32 and dev[1].shape == (8, 3) and dev[2].shape == (8,) and dev[2].dtype == np.float64
        assert dev[3].shape == (8,) and dev[4].shape == (8,) and dev[5].shape == (8, 4) and dev[5].dtype == np.uint32
        host = sc.host_arm(md, eight, flex, eight.poses, 5, np.arange(8), 8, dihedrals)
        pos = md.positions()
        kept = sc.against_the_host_loop(dev, host, lambda pose: gc.guest_oracle_row(orc, R, gR, pos, guest_sys, pose, cfg)[1], what)
        st = dev[5][kept]
        kinds = {x["move"]["kind"] for w in kept for x in host[w]["trace"][1:]}
        assert kinds == {S.TRANSLATION, S.ROTATION, S.TORSION}, kinds
        assert (st[:, 3] == 40).all() and (st[:, 2] == 0).all()
        assert st[:, 0].sum() > 0 and (st[:, 0] < 4).any(), "the runs should hold accepted and rejected rounds"
        assert (dev[3] > 0).all() if dihedrals else (dev[3] == 0).all()
        assert np.array_equal(dev[2], row_sum(dev[1], dev[3])), "the score is the sum of the returned row and dihedral energy"


# ---- 2: one round --------------------------------------------------------------------------------------------------------------------------------
def test_one_round_is_refine_guests_flex_bit_for_bit(mdx):
    env, groups, lib_, flex = fc.mixed_flex_case()
    with mdx.MdState(env, t.small_configs()[0]) as md:
        md.set_energy_groups(groups, 2)
        for evals, dihedrals in ((6, True), (3, False)):
            *ref, (bp, bs) = md.refine_guests_flex(lib_, flex, evals, 0.0, 0.0, 0.0, dihedrals=dihedrals, best=True)
            *dev, (bw, bl) = md.search_guests(lib_, flex, 1, *MOVES, KT, SEED, evals, 0.0, 0.0, 0.0, dihedrals=dihedrals, best=True)
            for m, lig in enumerate(lib_):
                sc.same_bits((dev[0][m], dev[1][m], dev[3][m]), (ref[0][m], ref[1][m], ref[4][m]), f"ligand {m} ({lig.count} atoms), {evals} evaluations",
                             ("best", "rows", "dih"))
                n = lig.n_poses
                assert (dev[4][m] == 0).all() and np.array_equal(dev[5][m], np.stack([np.zeros(n), np.zeros(n), np.zeros(n), ref[7][m]], 1).astype(np.uint32))
                assert np.array_equal(dev[2][m], row_sum(ref[1][m], ref[4][m]))
            assert np.array_equal(bw, bp) and np.array_equal(bits(bl), bits(bs)), (bw, bp, bl, bs)
            assert bw[2] == 0xFFFFFFFF and bl[2] == np.inf and (np.delete(bw, 2) != 0xFFFFFFFF).all()


# ---- 3: batch independence, the prefix, the stream ids, the host loop on the mixed library -----------------------------------------------------
def test_mixed_library_in_any_order_and_against_the_host_loop(mdx, orc):
    env, groups, lib_, flex = fc.mixed_flex_case()
    guest_systems = list(gc.mixed_case()[2]) + [systems.lig50(fc.CHAIN_SEED, 4)]
    counts = [l.n_poses for l in lib_]
    edges = np.concatenate([[0], np.cumsum(counts)])
    assert edges[-1] > 256 and edges[7] < 256 < edges[8], "two chunks, and the 64-atom ligand's walkers straddle walker 256"
    cfg = t.small_configs()[0]
    args = (*MOVES, KT, SEED, 4, 0.0, 0.0, 0.0)
    with mdx.MdState(env, cfg) as md:
        assert md.set_energy_groups(groups, 2) == 2
        *full, (bw, bl) = md.search_guests(lib_, flex, 3, *args, best=True)
        *back, (rbw, rbl) = md.search_guests(lib_[::-1], flex[::-1], 3, *args, best=True)
        back = [v[::-1] for v in back]
        assert np.array_equal(bw, rbw[::-1]) and np.array_equal(bits(bl), bits(rbl[::-1]))
        local = np.concatenate([np.arange(n, dtype=np.uint64) for n in counts])
        explicit = md.search_guests(lib_, flex, 3, *args, streams=local)
        other = md.search_guests(lib_, flex, 3, *args, streams=local + np.uint64(1000))
        two = md.search_guests(lib_, flex, 2, *args)
        pos = md.positions()
        changed = 0
        for m, (lig, fx) in enumerate(zip(lib_, flex)):
            mine = [v[m] for v in full]
            what = f"ligand {m} ({lig.count} atoms, {fx.n_torsions} torsions)"
            sc.same_bits(mine, [v[m] for v in back], what + " in the reversed library")
            sc.same_bits(mine, [v[m] for v in explicit], what + " with its ligand-local indices as explicit stream ids")
            if lig.n_poses == 0:
                assert mine[0].shape == (0, lig.count, 3) and bw[m] == 0xFFFFFFFF and bl[m] == np.inf
                continue
            *alone, (abw, abl) = md.search_guests([lig], [fx], 3, *args, best=True)
            sc.same_bits(mine, [v[0] for v in alone], what + " by itself")
            assert abw[0] == bw[m] and bits(abl)[0] == bits(bl)[m]
            changed += int(any(not np.array_equal(bits(a), bits(b)) for a, b in zip(mine[2:], [v[m] for v in other][2:])))
            # the per-ligand pick and the score
            assert np.array_equal(mine[2], row_sum(mine[1], mine[3])) and np.isfinite(mine[2]).all()
            assert bw[m] == int(np.argmin(mine[2])) and bits(bl)[m] == bits(mine[2])[bw[m]]
            # the prefix: a walker whose best of three rounds lies in rounds 0 .. 1 has that best after two
            short = [v[m] for v in two]
            early = mine[4] <= 1
            sc.same_bits([a[early] for a in short[:5]], [a[early] for a in mine[:5]], what + ": walkers with their best in rounds 0 .. 1", NAMES[:5])
            assert (short[2] >= mine[2]).all() and (short[4][~early] <= 1).all()
            # the host loop on the ligand's first and last walker and on the library's walkers 255 and 256
            pick = sorted({0, lig.n_poses - 1} | {p - int(edges[m]) for p in (255, 256) if edges[m] <= p < edges[m + 1]})
            host = sc.host_arm(md, lig, fx, lig.poses[pick], 3, pick, 4)
            gross = lambda pose, m=m: gc.guest_oracle_row(orc, env, groups, pos, guest_systems[m], pose, cfg)[1]
            # (the cap of one walker left out is for eight; of these two to four none may be, walkers 255 and 256 least of all)
            kept = sc.against_the_host_loop([v[pick] for v in mine], host, gross, what + f", walkers {pick}", max_tight=0)
            assert kept == list(range(len(pick)))
            for w in kept:
                for n, run in ((2, short), (3, mine)):
                    br, st = counters(host[w]["trace"], n)
                    assert int(run[4][pick[w]]) == br and run[5][pick[w]].tolist() == st, (m, pick[w], n, br, st)
            if lig.count == 1:      # the ion: no torsion, and a rotation about its own centre moves nothing - yet it is searched like the others
                assert fx.n_torsions == 0
                for h in host:
                    cur = None
                    for x in h["trace"]:
                        if x["move"] is not None:
                            assert x["move"]["kind"] in (S.TRANSLATION, S.ROTATION)
                            if x["move"]["kind"] == S.ROTATION:
                                assert np.array_equal(bits(x["start"]), bits(cur)), "a rotation moves an ion"
                        if x["accept"]:
                            cur = x["result"]["pose"]
        assert changed >= len([n for n in counts if n]) - 1, "other stream ids must give other searches"


# ---- 4: the per-ligand pick --------------------------------------------------------------------------------------------------------------------
def test_best_walker_is_the_host_argmin_of_the_scores(mdx):
    S_, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    poses = lig.poses
    fx = fc.small_flex(31)
    ion = gc.ion_system()
    with mdx.MdState(R, t.small_configs()[1]) as md:
        md.set_energy_groups(gR, 2)
        on_top = poses[5].copy()
        on_top[0] = md.positions()[3]      # its first atom on an atom of the receptor: not finite at round 0
        # an ion on a receptor atom, and rotations as the only move: a rotation moves no ion, so no round of it is ever finite
        stuck = GuestLigand.from_system(ion, 0, 1, poses=np.stack([md.positions()[3:4], md.positions()[40:41]]))
        lib_ = [lig.with_poses(poses[:4]), lig.with_poses(None), lig.with_poses(np.concatenate([poses[7:8], poses[:8]])), lig.with_poses(on_top[None]),
                lig.with_poses(np.stack([on_top, poses[2], on_top, poses[2]])), stuck]
        flex = [fx, fx, fx, fx, fx, GuestFlex()]
        ids = np.concatenate([np.arange(4), [7], np.arange(8), [0], [0, 5, 1, 5], [0, 1]]).astype(np.uint64)      # ligand 2: walkers 0 and 8 share stream 7
        *out, (bw, bl) = md.search_guests(lib_, flex, 3, 0.0, 0.3, 0.0, KT, SEED, 6, 0.0, 0.0, 0.0, streams=ids, best=True)
        best, rows, score, dih, best_round, stats = out
        assert bw.dtype == np.uint32 and bl.dtype == np.float64 and bw.shape == bl.shape == (len(lib_),)
        for m, s in enumerate(score):
            print(f"ligand {m}: scores {s.tolist()}, non-finite rounds {stats[m][:, 2].tolist() if len(s) else []}, picked {bw[m]} {bl[m]}")
            if not np.isfinite(s).any():
                assert bw[m] == 0xFFFFFFFF and bl[m] == np.inf, (m, bw[m], bl[m])
                continue
            assert bw[m] == int(np.argmin(s)) and bits(bl)[m] == bits(s)[bw[m]], (m, bw[m], s)
            assert np.isfinite(s[bw[m]])
        assert bw[1] == 0xFFFFFFFF and bw[5] == 0xFFFFFFFF, "a ligand without a walker, and one without a finite walker"
        assert (score[5] == np.inf).all() and (stats[5][:, 2] == 3).all() and (stats[5][:, 0] == 0).all()
        assert np.array_equal(bits(best[5]), bits(stuck.poses)) and (best_round[5] == 0).all(), "a walker without a finite round keeps its start pose"
        assert (stats[3][:, 2] >= 1).all() and (stats[4][[0, 2], 2] >= 1).all(), "the walkers on a receptor atom are not finite at round 0"
        assert (np.isfinite(score[3]) | (stats[3][:, 2] == 3)).all(), "still +inf only if no later round was finite"
        sc.same_bits([v[2][0:1] for v in out], [v[2][8:9] for v in out], "the same start with the same stream id")
        assert bw[2] != 8, "the lower index wins the tie"
        sc.same_bits([v[4][1:2] for v in out], [v[4][3:4] for v in out], "the same start with the same stream id (ligand 4)")
        assert bw[4] != 3
        plain = md.search_guests(lib_, flex, 3, 0.0, 0.3, 0.0, KT, SEED, 6, 0.0, 0.0, 0.0, streams=ids)
        for m in range(len(lib_)):
            sc.same_bits([v[m] for v in out], [v[m] for v in plain], f"ligand {m} with and without best")


# ---- 5: a start that is not finite recovers ---------------------------------------------------------------------------------------------------
def test_a_start_that_is_not_finite_recovers(mdx):
    """Four walkers from one start whose first atom lies on a receptor atom, translations only: round 0 is not finite, the first finite
    round becomes current and best.  Which rounds are finite is read from the host arm; the device search must agree with it."""
    S_, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    fx = fc.small_flex(8)
    moves = (0.5, 0.0, 0.0)
    with mdx.MdState(R, t.small_configs()[0]) as md:
        md.set_energy_groups(gR, 2)
        on_top = lig.poses[5].copy()
        on_top[0] = md.positions()[3]
        four = lig.with_poses(np.stack([on_top] * 4))
        host = sc.host_arm(md, four, fx, four.poses, 4, np.arange(4), 6, moves=moves)
        recovered = [w for w, h in enumerate(host) if not h["trace"][0]["result"]["finite"] and np.isfinite(h["S"]) and h["min_margin"] >= MARGIN]
        assert all(not h["trace"][0]["result"]["finite"] for h in host) and recovered, "the host arm should hold a walker that recovers"
        dev = [v[0] for v in md.search_guests([four], [fx], 4, *moves, KT, SEED, 6, 0.0, 0.0, 0.0)]
        for w in recovered:
            h = host[w]
            first = min(r for r, x in enumerate(h["trace"]) if x["result"]["finite"])
            print(f"walker {w}: finite per round {[bool(x['result']['finite']) for x in h['trace']]}, host best round {h['best_round']} counters {h['stats'].tolist()}, "
                  f"device {int(dev[4][w])} {dev[5][w].tolist()}")
            assert first >= 1 and h["trace"][first]["accept"] and h["trace"][first]["best"], "the first finite round becomes current and best"
            assert int(dev[4][w]) == h["best_round"] >= 1 and dev[5][w].tolist() == h["stats"].tolist() and dev[5][w][2] >= 1
            assert np.isfinite(dev[2][w]) and dev[2][w] == row_sum(dev[1][w:w + 1], dev[3][w:w + 1])[0]


# ---- 6: the handle ----------------------------------------------------------------------------------------------------------------------------
def test_the_handle_is_untouched(mdx):
    S_, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    fx = fc.small_flex(31)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)      # the fixed-order pair kernel
    args = (3, *MOVES, KT, SEED, 6, 0.0, 0.0, 0.0)
    with mdx.MdState(R, cfg) as md, mdx.MdState(R, cfg) as twin:
        for m in (md, twin):
            m.set_energy_groups(gR, 2)
            m.step(0.0005, None, 4)
        rebuilds = md.stats()["rebuild_count"]
        x0, f0, v0 = md.positions(), md.forces(), md.velocities()
        md.search_guests([lig], [fx], *args, best=True)
        assert md.stats()["rebuild_count"] == rebuilds, "the guest search must not rebuild the list of a ready handle"
        x1, f1, v1 = md.positions(), md.forces(), md.velocities()
        assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1)) and np.array_equal(bits(v0), bits(v1))
        twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        for what in ("positions", "velocities", "forces"):
            assert np.array_equal(bits(getattr(md, what)()), bits(getattr(twin, what)())), what
    # the resident-pose caches of a handle (the range's table, the torsion table, the resident search block) survive the call
    with mdx.MdState(S_, cfg) as md:
        md.set_energy_groups(t.three_groups(S_), 3)
        before = md.search_poses(lo, lig.poses, 0, tb, *args)
        other = lig.with_poses(lig.poses + np.array([0, 0, 9.0], np.float32))
        md.search_guests([other], [fc.small_flex(8)], *args, best=True)
        sc.same_bits(before, md.search_poses(lo, lig.poses, 0, tb, *args), "search_poses after the guest search")


# ---- 7: the refusals that need a device ---------------------------------------------------------------------------------------------------------
def raw_call(mdx, md, ligs, flex, n_groups, opts=None, patch=None, ids=None, no_best_out=False):
    """mdx_search_guests through ctypes with every output preset -> (return code, message, whether all outputs are as they were);
    patch(records): changes the mdx_guest_flex records behind the wrapper's own checks"""
    lib = mdx.load_library()
    M, recs, counts, (sizes, _keep) = md._guest_records("test", ligs)
    frecs, T, _fkeep = md._guest_flex_records("test", flex, sizes)
    if patch:
        patch(frecs)
    o, clean = sc.preset_outputs(sum(counts), sum(3 * a * p for a, p in zip(sizes, counts)), max(n_groups, 1) + 1, M)
    rc, msg = sc.raw_search(lib, md._h, M, recs, frecs, sc.search_opts(2, evals=4) if opts is None else opts, o, n_groups, ids, no_best_out)
    return rc, msg, clean()


def test_refusals_that_need_a_device_write_nothing(mdx):
    S_, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    fx = fc.small_flex(8)
    two = lig.with_poses(lig.poses[:2])
    cfg = t.small_configs()[0]

    def refused(md, ligs, flex, n_groups, match, named=True, **kw):
        rc, msg, clean = raw_call(mdx, md, ligs, flex, n_groups, **kw)
        assert rc == _abi.MDX_EPARAM and match in msg and ("mdx_search_guests" in msg or not named), (rc, msg)
        assert clean, f"a refused mdx_search_guests must leave every output untouched ({match})"

    with mdx.MdState(R, cfg) as md:
        refused(md, [two], [fx], 2, "no energy groups", named=False)      # (the two messages every group-keyed call shares)
        md.set_energy_groups(gR, 2)
        refused(md, [two], [fx], 3, "n_groups", named=False)
        # torsion moves alone, and a ligand that has poses but no torsion; without poses the same ligand is no obstacle
        rigid = fc.small_flex(0)
        tors_only = sc.search_opts(2, moves=(0.0, 0.0, 0.4), evals=4)
        refused(md, [two, two], [fx, rigid], 2, "ligand 1: no move is enabled", opts=tors_only)
        assert raw_call(mdx, md, [two, two.with_poses(None)], [fx, rigid], 2, opts=tors_only)[0] == 0
        refused(md, [two], [fx], 2, "null", no_best_out=True)
        # every refusal of mdx_guest_flex, through this entry point
        ring = GuestFlex(bonds=np.array([[0, 1], [1, 2], [2, 3], [3, 0], [3, 4], [4, 5]] + [[k, k + 1] for k in range(5, lig.count - 1)], np.uint32),
                         torsion_bonds=np.array([[3, 4], [1, 2]], np.uint32))
        refused(md, [two, two], [fx, ring], 2, "ligand 1: torsion 1")
        n = lig.count
        chain = np.array([[k, k + 1] for k in range(n - 1)], np.uint32)
        term = dict(dihedral_idx=np.array([[0, 1, 2, 3]], np.uint32), dihedral_v=np.ones(1, np.float32), dihedral_phase=np.zeros(1, np.float32),
                    dihedral_n=np.ones(1, np.int32))
        tbs = lambda *pairs: np.array(pairs, np.uint32).reshape(-1, 2)
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
        bad_pose = two.with_poses(np.full((1, n, 3), np.nan, np.float32))
        refused(md, [two, bad_pose], [fx, fx], 2, "ligand 1: non-finite pose coordinate")
        refused(md, [two], [fx], 2, "unknown flag", opts=sc.search_opts(2, evals=4, flags=2))
        refused(md, [two], [fx], 2, "negative", opts=sc.search_opts(2, evals=4, tors_tol=-1.0))
        rc, msg, clean = raw_call(mdx, md, [two.with_poses(None)], [fx], 2)
        assert rc == 0 and clean, "a library without a walker succeeds and writes nothing"
        rc, msg, clean = raw_call(mdx, md, [two], [ok], 2)
        assert rc == 0 and not clean, msg
    with mdx.MdState(S_, cfg) as md:
        md.set_energy_groups(t.three_groups(S_), 3)
        md.configure_alchemical_window(1, 0.5)
        refused(md, [two], [fx], 3, "alchemical")


def test_refused_on_a_decomposed_handle(mdx):
    from molchanica_amd.md_state import Fabric, MdState
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    g = t.three_groups(s)
    S_, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
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
                    assert rc == _abi.MDX_EPARAM and "decomposed" in msg and "mdx_search_guests" in msg and clean, (rc, msg, clean)
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [x.start() for x in th]
    [x.join() for x in th]
    if errs:
        raise errs[0]
