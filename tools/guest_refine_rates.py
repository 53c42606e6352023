#!/usr/bin/env python
"""Ligands per second and evaluations per second of `mdx_refine_guests` (one handle of receptor + solvent, the library as guests)
against the route a caller has without it: per candidate one `MdState(complex)` - receptor, solvent and the candidate as residents -
plus `set_energy_groups`, one `refine_poses`, then the handle is dropped.  System and library are those of tools/guest_screen_rates.py:
complex50k without its ligand; 50-atom guests (lig50 of --kinds seeds) with 16 poses each about the ligand's site; a fixed --max-evals
with tolerances of 0, so that every pose spends them unless it stalls.  The arms are interleaved over --rounds; every wall time ends in
the call's own device wait.  Appends one JSON line per round to profiles/guest_refine_rates.jsonl.

--resident: instead, the times of `score_poses` and `refine_poses` with 256 poses of the RESIDENT ligand of complex50k (the kernels both
ligand sources compile from), --reps calls each after a warm-up; run it alternately with MDX_LIB pointing at two builds to compare them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from molchanica_amd import GuestLigand, MdConfig, systems          # noqa: E402
from molchanica_amd.md_state import LIB_PATH, MdState          # noqa: E402
from tests import guest_cases as gc          # noqa: E402
from tests.test_gpu_pose_batch import ligand_range, rigid_poses, three_groups, whole          # noqa: E402


def resident(a):
    s = systems.complex50k()
    lo, hi = ligand_range(s)
    rec = {"what": "256 resident poses, complex50k", "lib": LIB_PATH, "reps": a.reps, "max_evals": a.max_evals}
    with MdState(s, MdConfig()) as md:
        md.set_energy_groups(three_groups(s), 3)
        poses = rigid_poses(whole(s, md.positions()[lo:hi]), 256, 2)
        for name, call in (("score_poses", lambda: md.score_poses(lo, poses)),
                           ("refine_poses", lambda: md.refine_poses(lo, poses, a.max_evals, 0.0, 0.0))):
            call()
            call()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = call()
                ts.append(time.perf_counter() - t0)
            ts = np.asarray(ts) * 1e3
            rec[name] = {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_p90": float(np.percentile(ts, 90))}
            rows = out if name == "score_poses" else out[1]
            rec[name]["row0"] = [float(v) for v in rows[0]]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ligands", type=int, default=256, help="guests in the library")
    ap.add_argument("--kinds", type=int, default=8, help="distinct lig50 seeds the library cycles through")
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--max-evals", type=int, default=24)
    ap.add_argument("--per-candidate", type=int, default=4, help="candidates the create-per-candidate arm runs per round")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guest_refine_rates.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.resident:
        rec = resident(a)
        with open(a.out, "a") as fo:
            fo.write(json.dumps(rec) + "\n")
        return
    S = systems.complex50k()
    lo, hi = ligand_range(S)
    R = gc.without_molecules(S, [1])
    gR = np.ones(R.n_atoms, np.uint8)
    gR[:lo] = 0
    site = np.asarray(S.pos, np.float64)[lo:hi].mean(0)
    kinds = [systems.lig50(seed=100 + k) for k in range(a.kinds)]
    lib_, residents = [], []
    for m in range(a.ligands):
        g = kinds[m % a.kinds]
        start = np.asarray(g.pos, np.float64) - np.asarray(g.pos, np.float64).mean(0) + site
        lib_.append(GuestLigand.from_system(g, 0, g.n_atoms, poses=rigid_poses(start, a.poses, 1000 + m)))
    for m in range(a.per_candidate):
        g = kinds[m % a.kinds]
        g.pos = lib_[m].poses[0]
        residents.append(gc.concat_systems([R, g], R))
    g3 = np.concatenate([gR, np.full(50, 2, np.uint8)])
    cfg = MdConfig()
    args = (a.max_evals, 0.0, 0.0)
    t0 = time.perf_counter()
    md = MdState(R, cfg)
    md.set_energy_groups(gR, 2)
    md.refine_guests(lib_[:2], *args, best=True)      # warm-up: code objects, the first rebuild
    t_create = time.perf_counter() - t0
    with MdState(residents[0], cfg) as w:      # warm-up of the other arm
        w.set_energy_groups(g3, 3)
        w.refine_poses(R.n_atoms, lib_[0].poses, *args)
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        *out, (bp, bs) = md.refine_guests(lib_, *args, best=True)
        t_guest = time.perf_counter() - t0
        evals_guest = int(sum(int(e.sum()) for e in out[5]))
        t0 = time.perf_counter()
        evals_each = 0
        for m in range(a.per_candidate):
            with MdState(residents[m], cfg) as one:
                one.set_energy_groups(g3, 3)
                res = one.refine_poses(R.n_atoms, lib_[m].poses, *args)
                evals_each += int(res[5].sum())
        t_each = (time.perf_counter() - t0) / a.per_candidate
        # the two routes answer the same question: the accepted rows of the last candidate (resident columns: receptor, solvent, ligand)
        m = a.per_candidate - 1
        d = np.abs(out[1][m].astype(np.float64) - res[1][:, [0, 1, 2]].astype(np.float64)).max()
        rec = {"system": "complex50k without its ligand", "n_resident_atoms": R.n_atoms, "ligands": a.ligands, "poses_per_ligand": a.poses,
               "max_evals": a.max_evals, "round": rnd, "handle_create_and_warm_up_s": t_create, "refine_guests_wall_s": t_guest,
               "refine_guests_ligands_per_s": a.ligands / t_guest, "refine_guests_evaluations_per_s": evals_guest / t_guest,
               "create_per_candidate_s": t_each, "create_per_candidate_ligands_per_s": 1.0 / t_each,
               "create_per_candidate_evaluations_per_s": evals_each / a.per_candidate / t_each, "ligands_per_s_ratio": t_each * a.ligands / t_guest,
               "evaluations_guests": evals_guest, "status_counts_guests": np.bincount(np.concatenate(out[4]), minlength=4).tolist(),
               "largest_accepted_row_difference_between_the_routes": float(d), "evaluations_equal_for_that_candidate": bool(np.array_equal(out[5][m], res[5])),
               "best_pose_of_ligand_0": int(bp[0]), "best_score_of_ligand_0": float(bs[0])}
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fo:
            fo.write(json.dumps(rec) + "\n")
    md.close()


if __name__ == "__main__":
    main()
