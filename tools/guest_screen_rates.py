#!/usr/bin/env python
"""Ligands per second and poses per second of `mdx_screen_ligands` (one handle of receptor + solvent, the library as guests) against
the route a caller has without it: per candidate one `MdState(complex)` - receptor, solvent and the candidate as residents - plus one
`score_poses`, then the handle is dropped.  System: complex50k without its ligand; library: 50-atom guests (lig50 of --kinds seeds,
each parameterised on its own) with 16 poses each about the ligand's site.  The arms are interleaved over --rounds; every wall time
ends in the call's own device wait.  Appends one JSON line per round to profiles/guest_screen_rates.jsonl.

--resident: instead, the time of `score_poses` with 256 poses of the RESIDENT ligand of complex50k (the pose pass both ligand sources
compile from), --reps calls after a warm-up; run it alternately with MDX_LIB pointing at two builds to compare them."""
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
    with MdState(s, MdConfig()) as md:
        md.set_energy_groups(three_groups(s), 3)
        poses = rigid_poses(whole(s, md.positions()[lo:hi]), 256, 2)
        md.score_poses(lo, poses)
        md.score_poses(lo, poses)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rows = md.score_poses(lo, poses)
            ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e3
    rec = {"what": "score_poses, 256 resident poses, complex50k", "lib": LIB_PATH, "reps": a.reps, "ms_median": float(np.median(ts)),
           "ms_min": float(ts.min()), "ms_p90": float(np.percentile(ts, 90)), "row0": [float(v) for v in rows[0]]}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ligands", type=int, default=256, help="guests in the library")
    ap.add_argument("--kinds", type=int, default=8, help="distinct lig50 seeds the library cycles through")
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--per-candidate", type=int, default=4, help="candidates the create-per-candidate arm runs per round")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guest_screen_rates.jsonl"))
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
        poses = rigid_poses(start, a.poses, 1000 + m)
        lib_.append(GuestLigand.from_system(g, 0, g.n_atoms, poses=poses))
    for m in range(a.per_candidate):
        g = kinds[m % a.kinds]
        g.pos = lib_[m].poses[0]
        residents.append(gc.concat_systems([R, g], R))
    g3 = np.concatenate([gR, np.full(50, 2, np.uint8)])
    cfg = MdConfig()
    t0 = time.perf_counter()
    md = MdState(R, cfg)
    md.set_energy_groups(gR, 2)
    md.screen_ligands(lib_[:2], best=True)      # warm-up: code objects, the first rebuild
    t_create = time.perf_counter() - t0
    with MdState(residents[0], cfg) as w:      # warm-up of the other arm
        w.set_energy_groups(g3, 3)
        w.score_poses(R.n_atoms, lib_[0].poses)
    n_poses = sum(l.n_poses for l in lib_)
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        rows, (bp, bs) = md.screen_ligands(lib_, best=True)
        t_screen = time.perf_counter() - t0
        t0 = time.perf_counter()
        for m in range(a.per_candidate):
            with MdState(residents[m], cfg) as one:
                one.set_energy_groups(g3, 3)
                res = one.score_poses(R.n_atoms, lib_[m].poses)
        t_each = (time.perf_counter() - t0) / a.per_candidate
        # the two routes answer the same question: environment columns and the ligand's own element of the last candidate
        d = np.abs(rows[a.per_candidate - 1].astype(np.float64) - res[:, [0, 1, 2]].astype(np.float64)).max()
        rec = {"system": "complex50k without its ligand", "n_resident_atoms": R.n_atoms, "ligands": a.ligands, "poses_per_ligand": a.poses,
               "round": rnd, "handle_create_and_warm_up_s": t_create, "screen_wall_s": t_screen, "screen_ligands_per_s": a.ligands / t_screen,
               "screen_poses_per_s": n_poses / t_screen, "create_per_candidate_s": t_each, "create_per_candidate_ligands_per_s": 1.0 / t_each,
               "create_per_candidate_poses_per_s": a.poses / t_each, "ligands_per_s_ratio": t_each * a.ligands / t_screen,
               "largest_row_difference_between_the_routes": float(d), "best_pose_of_ligand_0": int(bp[0]), "best_score_of_ligand_0": float(bs[0])}
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fo:
            fo.write(json.dumps(rec) + "\n")
    md.close()


if __name__ == "__main__":
    main()
