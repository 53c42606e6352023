#!/usr/bin/env python
"""Ligands per second and evaluations per second of `mdx_search_guests` (arm A: one call searches the whole library) against the host
loop it replaces (arm B: per round one `refine_guests_flex` call for the whole library, then the move and the Metropolis decision of
tests/pose_search_ref.py per walker in numpy - what a caller writes without the call; it needs nothing a build before
`mdx_search_guests` lacks).  The workload is that of tools/guest_flex_rates.py: complex50k without its ligand; 50-atom guests (lig50 of
--kinds seeds) with 16 walkers each about the ligand's site, all rotatable bonds; --n-rounds rounds of --max-evals evaluations with
tolerances of 0; moves and kT as in tests/test_gpu_pose_search.py.  The arms are interleaved over --rounds; every wall time ends in the
call's own device wait.  Arm B's time is given whole and as the part spent inside its refine_guests_flex calls.  Appends one JSON line
per round to profiles/guest_search_rates.jsonl.

--ab: instead, the times of the calls this work must leave as they were - `refine_poses_flex` and `search_poses` on the resident ligand
of complex50k, `screen_ligands`, `refine_guests` and `refine_guests_flex` on the library - --reps calls each after a warm-up, one JSON
line to --out.  It uses nothing a build before `mdx_search_guests` lacks: copy it into the other tree's tools/, run it from the two
trees alternately and compare (profiles/guest_search_resident_ab.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from guest_flex_rates import library, timed          # noqa: E402  (the sibling tool: the same library, the same way of timing a call)
from molchanica_amd import GuestFlex, MdConfig, systems          # noqa: E402
from molchanica_amd.md_state import LIB_PATH, MdState          # noqa: E402
from tests import guest_cases as gc          # noqa: E402
from tests import guest_flex_cases as fc          # noqa: E402
from tests import pose_flex_ref as F          # noqa: E402
from tests import pose_refine_ref as P          # noqa: E402
from tests import pose_search_ref as S          # noqa: E402
from tests.test_gpu_pose_batch import ligand_range, rigid_poses, three_groups, whole          # noqa: E402

MOVES, KT, SEED = (0.5, 0.15, 0.4), 100.0, 78      # (tests/test_gpu_pose_search.py)


def flexible(a, kinds):
    """One GuestFlex per ligand of library(a, .): all rotatable bonds (at most 32) -> (per kind, per ligand)"""
    kflex = [GuestFlex.from_system(g, 0, g.n_atoms) for g in kinds]
    return kflex, [kflex[m % a.kinds] for m in range(a.ligands)]


def receptor():
    s = systems.complex50k()
    lo, hi = ligand_range(s)
    R = gc.without_molecules(s, [1])
    gR = np.ones(R.n_atoms, np.uint8)
    gR[:lo] = 0
    return s, lo, hi, R, gR


def ab(a):
    s, lo, hi, R, gR = receptor()
    rec = {"what": "calls that must stay as they were, complex50k", "label": a.label, "lib": LIB_PATH, "reps": a.reps, "max_evals": a.max_evals}
    tb = F.rotatable_bonds(hi - lo, F.local_bonds(s, lo, hi), 0)[:32]
    with MdState(s, MdConfig()) as md:
        md.set_energy_groups(three_groups(s), 3)
        poses = rigid_poses(whole(s, md.positions()[lo:hi]), 256, 2)
        rec["refine_poses_flex"] = timed(lambda: md.refine_poses_flex(lo, poses, 0, tb, a.max_evals, 0.0, 0.0, 0.0), a.reps)
        rec["search_poses"] = timed(lambda: md.search_poses(lo, poses, 0, tb, 4, 0.5, 0.2, 0.3, 0.6, 7, 8, 0.0, 0.0, 0.0), a.reps)
    kinds, lib_ = library(a, np.asarray(s.pos, np.float64)[lo:hi].mean(0))
    _, flex = flexible(a, kinds)
    with MdState(R, MdConfig()) as md:
        md.set_energy_groups(gR, 2)
        rec["screen_ligands"] = timed(lambda: md.screen_ligands(lib_, best=True), a.reps)
        rec["refine_guests"] = timed(lambda: md.refine_guests(lib_, a.max_evals, 0.0, 0.0, best=True), a.reps)
        rec["refine_guests_flex"] = timed(lambda: md.refine_guests_flex(lib_, flex, a.max_evals, 0.0, 0.0, 0.0, best=True), a.reps)
    print(json.dumps(rec), flush=True)
    return rec


def host_loop(md, lib_, flex, tors, n_rounds, max_evals):
    """Arm B -> (score per ligand, best round per ligand, evaluations in all, seconds inside the refine_guests_flex calls)"""
    M = len(lib_)
    starts = [np.ascontiguousarray(l.poses, np.float32) for l in lib_]
    cur = [x.copy() for x in starts]
    recs = [[dict() for _ in range(len(x))] for x in starts]
    evals, t_dev = 0, 0.0
    for r in range(n_rounds):
        s0 = [[S.stream(SEED, w, r) for w in range(len(starts[m]))] for m in range(M)]
        if r == 0:
            X = starts
        else:
            X = [np.stack([S.perturb(cur[m][w], tors[m], S.move(*MOVES, len(tors[m]), s0[m][w])) for w in range(len(cur[m]))]) for m in range(M)]
        t0 = time.perf_counter()
        y, rows, rigid, xform, dih, tgrad, status, ev = md.refine_guests_flex([l.with_poses(x) for l, x in zip(lib_, X)], flex, max_evals, 0.0, 0.0, 0.0)
        t_dev += time.perf_counter() - t0
        for m in range(M):
            Sm = rows[m].astype(np.float64).cumsum(1)[:, -1] + dih[m].astype(np.float64)      # (columns in order, then E_dih)
            evals += int(ev[m].sum())
            for w in range(len(Sm)):
                accept, uphill, is_best, margin = S.decide(recs[m][w], r, float(Sm[w]), int(status[m][w]) != P.NONFINITE, KT, s0[m][w])
                if accept:
                    cur[m][w] = y[m][w]
    score = [np.array([q["S_best"] for q in rm]) for rm in recs]
    rounds = [np.array([q["best_round"] for q in rm], np.uint32) for rm in recs]
    return score, rounds, evals, t_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of the two arms, interleaved")
    ap.add_argument("--ligands", type=int, default=256, help="guests in the library")
    ap.add_argument("--kinds", type=int, default=8, help="distinct lig50 seeds the library cycles through")
    ap.add_argument("--poses", type=int, default=16, help="walkers per ligand")
    ap.add_argument("--max-evals", type=int, default=24)
    ap.add_argument("--n-rounds", type=int, default=8, help="rounds of the search")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "guest_search_resident_ab.jsonl" if a.ab else "guest_search_rates.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if a.ab:
        rec = ab(a)
        with open(out, "a") as fo:
            fo.write(json.dumps(rec) + "\n")
        return
    s, lo, hi, R, gR = receptor()
    kinds, lib_ = library(a, np.asarray(s.pos, np.float64)[lo:hi].mean(0))
    kflex, flex = flexible(a, kinds)
    ktors = [fc.sides_of(f, g.n_atoms) for f, g in zip(kflex, kinds)]
    tors = [ktors[m % a.kinds] for m in range(a.ligands)]
    args = (a.n_rounds, *MOVES, KT, SEED, a.max_evals, 0.0, 0.0, 0.0)
    walkers = a.ligands * a.poses
    with MdState(R, MdConfig()) as md:
        md.set_energy_groups(gR, 2)
        md.search_guests(lib_[:2], flex[:2], *args, best=True)      # warm-up: code objects, the first rebuild
        md.refine_guests_flex(lib_[:2], flex[:2], a.max_evals, 0.0, 0.0, 0.0)
        for rnd in range(a.rounds):
            t0 = time.perf_counter()
            *dev, (bw, bl) = md.search_guests(lib_, flex, *args, best=True)
            t_a = time.perf_counter() - t0
            evals_a = int(sum(int(v[:, 3].sum()) for v in dev[5]))
            t0 = time.perf_counter()
            score, rounds, evals_b, t_dev = host_loop(md, lib_, flex, tors, a.n_rounds, a.max_evals)
            t_b = time.perf_counter() - t0
            same_round = sum(int((x == y).sum()) for x, y in zip(dev[4], rounds))
            same_score = sum(int((x == y).sum()) for x, y in zip(dev[2], score))
            rec = {"system": "complex50k without its ligand", "n_resident_atoms": R.n_atoms, "ligands": a.ligands, "walkers_per_ligand": a.poses,
                   "torsions_per_ligand": [f.n_torsions for f in kflex], "n_rounds": a.n_rounds, "max_evals": a.max_evals, "moves": MOVES, "kT": KT,
                   "round": rnd, "search_guests_wall_s": t_a, "search_guests_ligands_per_s": a.ligands / t_a, "search_guests_evaluations_per_s": evals_a / t_a,
                   "host_loop_wall_s": t_b, "host_loop_ligands_per_s": a.ligands / t_b, "host_loop_evaluations_per_s": evals_b / t_b,
                   "host_loop_s_inside_refine_guests_flex": t_dev, "ratio_host_loop_over_search_guests": t_b / t_a,
                   "ratio_refine_calls_of_the_host_loop_over_search_guests": t_dev / t_a, "evaluations_search_guests": evals_a,
                   "evaluations_host_loop": evals_b, "walkers": walkers, "walkers_with_the_same_best_round": same_round,
                   "walkers_with_the_same_score_bits": same_score, "best_walker_of_ligand_0": int(bw[0]), "best_score_of_ligand_0": float(bl[0])}
            print(json.dumps(rec), flush=True)
            with open(out, "a") as fo:
                fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
