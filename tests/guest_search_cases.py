"""What tests/test_guest_search_host.py (CPU) and tests/test_gpu_guest_search.py (GPU) share for `mdx_search_guests` /
`MdState.search_guests`: the host loop the call replaces - `pose_search_ref.search` per walker with one `MdState.refine_guests_flex`
call per round behind it -, the comparison against it by the criteria of tests/test_gpu_pose_search.py, and the C entry point through
ctypes with every output preset.  No tolerance of its own: all are imported."""
import ctypes as C

import numpy as np

from molchanica_amd import _abi
from tests import guest_cases as gc
from tests import guest_flex_cases as fc
from tests import pose_refine_ref as P
from tests import pose_search_ref as S
from tests.test_gpu_pose_search import KT, MARGIN, MOVES, SEED, bits, ulp32

t = gc.pose_batch_module()
NAMES = ("best", "rows", "score", "dih", "best_round", "stats")


def same_bits(a, b, what, names=NAMES):
    for x, y, name in zip(a, b, names):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), f"{what}: {name} differ"


def guest_refiner(md, lig, flex, max_evals, dihedrals=True):
    """`refine` of the host loop: one `MdState.refine_guests_flex` call per round"""
    def refine(X0):
        y, rows, rigid, xform, dih, tgrad, status, ev = (v[0] for v in md.refine_guests_flex(
            [lig.with_poses(np.ascontiguousarray(X0[None]))], [flex], max_evals, 0.0, 0.0, 0.0, dihedrals=dihedrals))
        s = 0.0
        for v in rows[0]:
            s += float(v)
        s += float(dih[0])
        return dict(pose=y[0], row=rows[0], edih=dih[0], S=s, finite=int(status[0]) != P.NONFINITE, evals=int(ev[0]))
    return refine


def host_arm(md, lig, flex, starts, n_rounds, ids, max_evals, dihedrals=True, moves=MOVES, kT=KT, seed=SEED):
    """The host loop, walker by walker -> [dict of pose_search_ref.search + trace]"""
    refine = guest_refiner(md, lig, flex, max_evals, dihedrals)
    tors = fc.sides_of(flex, lig.count)
    out = []
    for w in range(len(starts)):
        trace = []
        res = S.search(starts[w], refine, tors, n_rounds, *moves, kT, seed, int(ids[w]), trace=trace)
        res["trace"] = trace
        out.append(res)
    return out


def against_the_host_loop(dev, host, gross_of, what, max_tight=1):
    """The criteria of tests/test_gpu_pose_search.py::against_the_host_loop for one ligand's walkers.  dev: (best, rows, score, dih,
    best_round, stats) of those walkers; gross_of(pose) -> the oracle's gross sums of the row at that pose (asked only where the best
    coordinates are not the host arm's bits).  A walker whose host-arm Metropolis margin is below MARGIN is left out, at most
    max_tight of them.  -> the walkers compared"""
    best, rows, score, dih, best_round, stats = dev
    tight = [w for w, h in enumerate(host) if h["min_margin"] < MARGIN]
    assert len(tight) <= max_tight, f"{what}: walkers {tight} hold a decision within {MARGIN} of its threshold"
    differ, worst, kept = 0, 0.0, [w for w in range(len(host)) if w not in tight]
    for w in kept:
        h = host[w]
        flags = [int(x["accept"]) + 2 * int(x["uphill"]) for x in h["trace"]]
        print(f"{what}, walker {w}: S per round {[round(float(x['result']['S']), 2) for x in h['trace']]}, decisions {flags}, best round {h['best_round']}, "
              f"counters {h['stats'].tolist()}, device {int(best_round[w])} {stats[w].tolist()}")
        assert int(best_round[w]) == h["best_round"], f"{what}, walker {w}: best round device {best_round[w]} host {h['best_round']}"
        assert stats[w].tolist() == h["stats"].tolist(), f"{what}, walker {w}: counters device {stats[w].tolist()} host {h['stats'].tolist()}"
        if not np.isfinite(h["S"]):
            assert score[w] == np.inf, f"{what}, walker {w}: no finite round in the host arm, score {score[w]}"
            continue
        ne = int((bits(best[w]) != bits(h["pose"])).sum())
        differ += ne
        worst = max(worst, float(np.abs(best[w].astype(np.float64) - h["pose"].astype(np.float64)).max()) / ulp32(h["pose"]))
        if ne == 0:
            assert np.array_equal(bits(rows[w]), bits(h["row"])) and bits(dih[w:w + 1])[0] == bits(np.float32(h["edih"]).reshape(1))[0], f"{what}, walker {w}: row or E_dih"
            assert score[w] == h["S"], f"{what}, walker {w}: score {score[w]!r} host {h['S']!r}"
        else:
            gr = gross_of(h["pose"])
            t.assert_row(rows[w], h["row"].astype(np.float64), gr, f"{what}, walker {w}: row against the host arm's")
            tol = float((2e-6 * np.abs(h["row"]) + 1e-6 * gr + 1e-3).sum()) + 1e-3
            assert abs(float(dih[w]) - float(h["edih"])) <= 1e-3 and abs(score[w] - h["S"]) <= tol
    print(f"{what}: {len(kept)} walkers compared, {differ} of {sum(best[w].size for w in kept)} best coordinates not bit-equal to the host loop's, "
          f"worst difference {worst:.2f} ulp32(max |coordinate|)")
    assert worst <= 4.0, f"{what}: a best coordinate differs from the host loop's by {worst:.1f} ulp32"
    return kept


def search_opts(n_rounds=2, moves=MOVES, kT=KT, evals=4, seed=SEED, tors_tol=0.0, h_start=0.0, h_max=0.0, flags=1):
    return _abi.CSearchOpts(n_rounds, *moves, kT, seed, _abi.CFlexOpts(evals, 0.0, 0.0, tors_tol, h_start, h_max, flags))


def preset_outputs(n, nx, W, M):
    """the nine outputs of mdx_search_guests, preset -> (arrays, whether they are all still as preset)"""
    o = [np.full(max(nx, 1), -7.0, np.float32), np.full((max(n, 1), W), -7.0, np.float32), np.full(max(n, 1), -7.0, np.float64),
         np.full(max(n, 1), -7.0, np.float32), np.full(max(n, 1), 77, np.uint32), np.full((max(n, 1), 4), 77, np.uint32),
         np.full(max(M, 1), 77, np.uint32), np.full(max(M, 1), -7.0, np.float64)]
    clean = lambda: all((v == (77 if v.dtype == np.uint32 else -7.0)).all() for v in o)
    return o, clean


def raw_search(lib, h, M, recs, frecs, opts, o, n_groups, ids=None, no_best_out=False):
    """mdx_search_guests through ctypes -> (return code, message)"""
    kinds = {np.dtype(np.uint32): C.POINTER(C.c_uint32), np.dtype(np.float32): C.POINTER(C.c_float), np.dtype(np.float64): C.POINTER(C.c_double),
             np.dtype(np.uint64): C.POINTER(C.c_uint64)}
    ptr = lambda a: a.ctypes.data_as(kinds[a.dtype])
    rc = lib.mdx_search_guests(h, M, recs, frecs, None if ids is None else ptr(ids), None if opts is None else C.byref(opts),
                               None if no_best_out else ptr(o[0]), ptr(o[1]), n_groups, ptr(o[2]), ptr(o[3]), ptr(o[4]), ptr(o[5]), ptr(o[6]), ptr(o[7]))
    return rc, lib.mdx_last_error().decode()
