"""The rule of `mdx_search_poses` (include/mdx.h states it) in numpy fp64 and Python integers, shared by tests/test_pose_search_host.py
(no GPU), tests/test_gpu_pose_search.py and tools/pose_search_rates.py: the stream of (seed, stream id, round), the move, the new start
and the decision.  It is parameterised by `refine(X0) -> dict(pose, row, edih, S, finite, evals)`: with `MdState.refine_poses_flex`
behind it, it is the host loop the device search replaces; with the numpy stepper of tests/pose_flex_ref.py behind it, it is
independent of the library.

Statement by statement it follows molchanica_amd/csrc/mdx_search_step.h; the new start is `coords` of tests/pose_flex_ref.py with the
(q, t) of one `trial` of tests/pose_refine_ref.py, as the header takes it from the two steppers."""
import math

import numpy as np

from tests import pose_flex_ref as F
from tests import pose_refine_ref as P

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
BALL_TRIES = 16
DRAW_CHOICE, DRAW_BALL, DRAW_TORSION, DRAW_ACCEPT = 0, 1, 1 + 3 * BALL_TRIES, 2 + 3 * BALL_TRIES
NONE, TRANSLATION, ROTATION, TORSION = 0, 1, 2, 3
MAX_ROUNDS = 1024


def mix(x):
    """the splitmix64 output of one step from state x"""
    z = (x + GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream(seed, sid, r):
    return mix(mix(mix(int(seed) & M64) ^ (int(sid) & M64)) ^ int(r))


def bits(s0, k):
    return mix((s0 + GOLD * k) & M64)


def u01(x):
    return (float(x >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def draw(s0, k):
    return u01(bits(s0, k))


def choices(trans_amp, rot_amp, tors_amp, T):
    return (1 if trans_amp > 0 else 0) + (1 if rot_amp > 0 else 0) + (T if tors_amp > 0 else 0)


def move(trans_amp, rot_amp, tors_amp, T, s0):
    """-> dict(kind, torsion, choice, tries, v [3], w [3], dtheta); amplitudes as the fp32 values the options hold"""
    ta, ra, ka = (float(np.float32(v)) for v in (trans_amp, rot_amp, tors_amp))
    nt, nr = (1 if ta > 0 else 0), (1 if ra > 0 else 0)
    n = choices(ta, ra, ka, T)
    mv = dict(kind=NONE, torsion=0, choice=0, tries=BALL_TRIES, v=np.zeros(3), w=np.zeros(3), dtheta=0.0)
    if n == 0:
        return mv
    j = min(int(draw(s0, DRAW_CHOICE) * float(n)), n - 1)
    mv["choice"] = j
    p = np.zeros(3)
    for i in range(BALL_TRIES):
        a, b, c = (2.0 * draw(s0, DRAW_BALL + 3 * i + d) - 1.0 for d in range(3))
        if (a * a + b * b) + c * c <= 1.0:
            p, mv["tries"] = np.array([a, b, c]), i
            break
    if j < nt:
        mv.update(kind=TRANSLATION, v=ta * p)
    elif j < nt + nr:
        mv.update(kind=ROTATION, w=ra * p)
    else:
        mv.update(kind=TORSION, torsion=j - nt - nr, dtheta=(2.0 * draw(s0, DRAW_TORSION) - 1.0) * ka)
    return mv


def perturb(ycur, tors, mv):
    """X0' = fp32(coords(dq, dt, dtheta)) of the flexible stepper with the accepted pose ycur as its input"""
    ycur = np.ascontiguousarray(ycur, np.float32)
    theta = np.zeros(len(tors))
    if mv["kind"] == TORSION:
        theta[mv["torsion"]] = mv["dtheta"]
    c0 = P.mean(ycur.astype(np.float64))
    q, t = P.trial(np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), mv["v"], mv["w"], 1.0, 1.0)
    return F.coords(c0, t, q, ycur, tors, theta)


def decide(rec, r, S, finite, kT, s0):
    """The decision on round r; rec: dict(S_cur, S_best, best_round, accepted, uphill, nonfinite) -> (accept, uphill, best, margin):
    margin = |u_acc - exp(.)| where the Metropolis condition was asked, else None"""
    kT = float(np.float32(kT))
    if r == 0:
        rec.update(S_cur=S if finite else math.inf, S_best=S if finite else math.inf, best_round=0, accepted=0, uphill=0,
                   nonfinite=0 if finite else 1)
        return True, False, True, None
    if not finite:
        rec["nonfinite"] += 1
        return False, False, False, None
    margin, accept, uphill = None, S < rec["S_cur"], False
    if not accept and kT > 0.0:
        u, e = draw(s0, DRAW_ACCEPT), math.exp(-(S - rec["S_cur"]) / kT)
        margin, accept = abs(u - e), u < e
        uphill = accept
    if not accept:
        return False, False, False, margin
    rec["accepted"] += 1
    rec["uphill"] += 1 if uphill else 0
    rec["S_cur"] = S
    best = S < rec["S_best"]
    if best:
        rec.update(S_best=S, best_round=r)
    return True, uphill, best, margin


def search(x0, refine, tors, n_rounds, trans_amp, rot_amp, tors_amp, kT, seed, sid, trace=None):
    """One walker.  refine(X0 float32 [n, 3]) -> dict(pose, row, edih, S, finite, evals) of the refinement's accepted state.
    trace, if a list, receives per round dict(move, start, result, accept, uphill, best, margin).
    -> dict(pose, row, edih, S, best_round, stats [4], rounds: the refinement's result per round, min_margin)"""
    T = len(tors)
    rec, cur, best = {}, None, None
    evals, rounds, min_margin = 0, [], math.inf
    for r in range(n_rounds):
        s0 = stream(seed, sid, r)
        mv, start = None, np.ascontiguousarray(x0, np.float32)
        if r > 0:
            mv = move(trans_amp, rot_amp, tors_amp, T, s0)
            start = perturb(cur, tors, mv)
        res = refine(start)
        rounds.append(res)
        evals += int(res["evals"])
        accept, uphill, is_best, margin = decide(rec, r, float(res["S"]), bool(res["finite"]), kT, s0)
        if margin is not None:
            min_margin = min(min_margin, margin)
        if accept:
            cur = np.array(res["pose"], np.float32)
        if is_best:
            best = dict(pose=np.array(res["pose"], np.float32), row=res["row"], edih=res["edih"], round=r)
        if trace is not None:
            trace.append(dict(move=mv, start=start, result=res, accept=accept, uphill=uphill, best=is_best, margin=margin))
    return dict(pose=best["pose"], row=best["row"], edih=best["edih"], S=rec["S_best"], best_round=rec["best_round"],
                stats=np.array([rec["accepted"], rec["uphill"], rec["nonfinite"], evals], np.uint32), rounds=rounds, min_margin=min_margin)


def search_batch(starts, refine_all, tors, n_rounds, trans_amp, rot_amp, tors_amp, kT, seed, ids=None):
    """Every walker, the rounds in step: refine_all(X float32 [W, n, 3]) -> (poses, rows, dih, status, evals) is one
    `MdState.refine_poses_flex` call per round for the whole batch - the host loop as a caller would write it.
    -> (best [W, n, 3], rows, score, dih, best_round, stats [W, 4], smallest Metropolis margin)"""
    starts = np.ascontiguousarray(starts, np.float32)
    W, T = len(starts), len(tors)
    ids = np.arange(W) if ids is None else ids
    recs = [dict(evals=0) for _ in range(W)]
    cur, best, rows_b, dih_b = starts.copy(), starts.copy(), None, np.zeros(W, np.float32)
    min_margin = math.inf
    for r in range(n_rounds):
        s0 = [stream(seed, int(ids[w]), r) for w in range(W)]
        X = starts if r == 0 else np.stack([perturb(cur[w], tors, move(trans_amp, rot_amp, tors_amp, T, s0[w])) for w in range(W)])
        y, rows, dih, status, evals = refine_all(X)
        if rows_b is None:
            rows_b = np.zeros_like(rows)
        for w in range(W):
            Sw = 0.0
            for v in rows[w]:
                Sw += float(v)
            Sw += float(dih[w])
            recs[w]["evals"] += int(evals[w])
            accept, uphill, is_best, margin = decide(recs[w], r, Sw, int(status[w]) != P.NONFINITE, kT, s0[w])
            if margin is not None:
                min_margin = min(min_margin, margin)
            if accept:
                cur[w] = y[w]
            if is_best:
                best[w], rows_b[w], dih_b[w] = y[w], rows[w], dih[w]
    return (best, rows_b, np.array([q["S_best"] for q in recs]), dih_b, np.array([q["best_round"] for q in recs], np.uint32),
            np.array([[q["accepted"], q["uphill"], q["nonfinite"], q["evals"]] for q in recs], np.uint32), min_margin)


def flex_refiner(md, first, root, tb, max_evals, f_tol, tau_tol, tors_tol, h_start=0.0, h_max=0.0, dihedrals=True):
    """`refine` of the host loop the device search replaces: one `MdState.refine_poses_flex` call per round"""
    def refine(X0):
        y, rows, rigid, xform, dih, tgrad, status, ev = md.refine_poses_flex(first, np.ascontiguousarray(X0[None]), root, tb, max_evals, f_tol,
                                                                            tau_tol, tors_tol, h_start, h_max, dihedrals)
        S = 0.0
        for v in rows[0]:
            S += float(v)
        S += float(dih[0])
        return dict(pose=y[0], row=rows[0], edih=dih[0], S=S, finite=int(status[0]) != P.NONFINITE, evals=int(ev[0]))
    return refine


def numpy_refiner(evaluate, tors, terms, max_evals, f_tol, tau_tol, tors_tol, h_start=0.0, h_max=0.0, box=None):
    """`refine` from the numpy flexible stepper alone (tests/pose_flex_ref.py: refine) around evaluate(Y) -> (row, rigid, forces)"""
    def refine(X0):
        res = F.refine(X0, evaluate, tors, terms, max_evals, f_tol, tau_tol, tors_tol, h_start, h_max, box)
        return dict(pose=res["pose"], row=res["row"], edih=res["edih"], S=res["S"], finite=res["status"] != P.NONFINITE, evals=res["evals"])
    return refine
