#!/usr/bin/env python
"""Ligands per second and evaluations per second of `mdx_refine_guests_flex` (one handle of receptor + solvent, the library as guests
with all their rotatable bonds) against the route a caller has without it: per candidate one `MdState(complex)` - receptor, solvent
and the candidate as residents - plus `set_energy_groups`, one `refine_poses_flex`, then the handle is dropped.  The workload is that of
tools/guest_refine_rates.py: complex50k without its ligand; 50-atom guests (lig50 of --kinds seeds) with 16 poses each about the
ligand's site; a fixed --max-evals with tolerances of 0.  The arms are interleaved over --rounds; every wall time ends in the call's own
device wait.  Appends one JSON line per round to profiles/guest_flex_rates.jsonl.

--ab: instead, the times of the calls this work must leave as they were - `score_poses` (256 poses), `refine_poses`,
`refine_poses_flex`, `search_poses` on the resident ligand of complex50k, `screen_ligands` and `refine_guests` on the library - --reps
calls each after a warm-up, one JSON line to --out.  It uses nothing a build before `mdx_refine_guests_flex` lacks: run it from two
trees alternately and compare (profiles/guest_flex_resident_ab.jsonl)."""
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
from tests import pose_flex_ref as F          # noqa: E402
from tests.test_gpu_pose_batch import ligand_range, rigid_poses, three_groups, whole          # noqa: E402


def timed(call, reps):
    call()
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e3
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_p90": float(np.percentile(ts, 90))}


def library(a, site):
    kinds = [systems.lig50(seed=100 + k) for k in range(a.kinds)]
    lib_ = []
    for m in range(a.ligands):
        g = kinds[m % a.kinds]
        start = np.asarray(g.pos, np.float64) - np.asarray(g.pos, np.float64).mean(0) + site
        lib_.append(GuestLigand.from_system(g, 0, g.n_atoms, poses=rigid_poses(start, a.poses, 1000 + m)))
    return kinds, lib_


def ab(a):
    s = systems.complex50k()
    lo, hi = ligand_range(s)
    rec = {"what": "calls that must stay as they were, complex50k", "label": a.label, "lib": LIB_PATH, "reps": a.reps, "max_evals": a.max_evals}
    tb = F.rotatable_bonds(hi - lo, F.local_bonds(s, lo, hi), 0)[:32]
    with MdState(s, MdConfig()) as md:
        md.set_energy_groups(three_groups(s), 3)
        poses = rigid_poses(whole(s, md.positions()[lo:hi]), 256, 2)
        rec["score_poses"] = timed(lambda: md.score_poses(lo, poses), a.reps)
        rec["refine_poses"] = timed(lambda: md.refine_poses(lo, poses, a.max_evals, 0.0, 0.0), a.reps)
        rec["refine_poses_flex"] = timed(lambda: md.refine_poses_flex(lo, poses, 0, tb, a.max_evals, 0.0, 0.0, 0.0), a.reps)
        rec["search_poses"] = timed(lambda: md.search_poses(lo, poses, 0, tb, 4, 0.5, 0.2, 0.3, 0.6, 7, 8, 0.0, 0.0, 0.0), a.reps)
    R = gc.without_molecules(s, [1])
    gR = np.ones(R.n_atoms, np.uint8)
    gR[:lo] = 0
    _, lib_ = library(a, np.asarray(s.pos, np.float64)[lo:hi].mean(0))
    with MdState(R, MdConfig()) as md:
        md.set_energy_groups(gR, 2)
        rec["screen_ligands"] = timed(lambda: md.screen_ligands(lib_, best=True), a.reps)
        rec["refine_guests"] = timed(lambda: md.refine_guests(lib_, a.max_evals, 0.0, 0.0, best=True), a.reps)
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
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guest_flex_rates.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.ab:
        rec = ab(a)
        with open(a.out, "a") as fo:
            fo.write(json.dumps(rec) + "\n")
        return
    from molchanica_amd import GuestFlex
    S = systems.complex50k()
    lo, hi = ligand_range(S)
    R = gc.without_molecules(S, [1])
    gR = np.ones(R.n_atoms, np.uint8)
    gR[:lo] = 0
    kinds, lib_ = library(a, np.asarray(S.pos, np.float64)[lo:hi].mean(0))
    kflex = [GuestFlex.from_system(g, 0, g.n_atoms) for g in kinds]      # all rotatable bonds (at most 32)
    flex = [kflex[m % a.kinds] for m in range(a.ligands)]
    residents = []
    for m in range(a.per_candidate):
        g = kinds[m % a.kinds]
        g.pos = lib_[m].poses[0]
        residents.append(gc.concat_systems([R, g], R))
    g3 = np.concatenate([gR, np.full(50, 2, np.uint8)])
    cfg = MdConfig()
    args = (a.max_evals, 0.0, 0.0, 0.0)
    t0 = time.perf_counter()
    md = MdState(R, cfg)
    md.set_energy_groups(gR, 2)
    md.refine_guests_flex(lib_[:2], flex[:2], *args, best=True)      # warm-up: code objects, the first rebuild
    t_create = time.perf_counter() - t0
    with MdState(residents[0], cfg) as w:      # warm-up of the other arm
        w.set_energy_groups(g3, 3)
        w.refine_poses_flex(R.n_atoms, lib_[0].poses, 0, flex[0].torsion_bonds, *args)
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        *out, (bp, bs) = md.refine_guests_flex(lib_, flex, *args, best=True)
        t_guest = time.perf_counter() - t0
        evals_guest = int(sum(int(e.sum()) for e in out[7]))
        t0 = time.perf_counter()
        evals_each = 0
        for m in range(a.per_candidate):
            with MdState(residents[m], cfg) as one:
                one.set_energy_groups(g3, 3)
                res = one.refine_poses_flex(R.n_atoms, lib_[m].poses, 0, flex[m].torsion_bonds, *args)
                evals_each += int(res[7].sum())
        t_each = (time.perf_counter() - t0) / a.per_candidate
        # the two routes answer the same question: the accepted rows and E_dih of the last candidate (resident columns: receptor,
        # solvent, ligand)
        m = a.per_candidate - 1
        d = np.abs(out[1][m].astype(np.float64) - res[1][:, [0, 1, 2]].astype(np.float64)).max()
        dd = np.abs(out[4][m].astype(np.float64) - res[4].astype(np.float64)).max()
        rec = {"system": "complex50k without its ligand", "n_resident_atoms": R.n_atoms, "ligands": a.ligands, "poses_per_ligand": a.poses,
               "torsions_per_ligand": [f.n_torsions for f in kflex], "dihedral_terms_per_ligand": [int(len(f.dihedral_idx)) for f in kflex],
               "max_evals": a.max_evals, "round": rnd, "handle_create_and_warm_up_s": t_create, "refine_guests_flex_wall_s": t_guest,
               "refine_guests_flex_ligands_per_s": a.ligands / t_guest, "refine_guests_flex_evaluations_per_s": evals_guest / t_guest,
               "create_per_candidate_s": t_each, "create_per_candidate_ligands_per_s": 1.0 / t_each,
               "create_per_candidate_evaluations_per_s": evals_each / a.per_candidate / t_each, "ligands_per_s_ratio": t_each * a.ligands / t_guest,
               "evaluations_guests": evals_guest, "status_counts_guests": np.bincount(np.concatenate(out[6]), minlength=4).tolist(),
               "largest_accepted_row_difference_between_the_routes": float(d), "largest_dihedral_energy_difference_between_the_routes": float(dd),
               "evaluations_equal_for_that_candidate": bool(np.array_equal(out[7][m], res[7])),
               "best_pose_of_ligand_0": int(bp[0]), "best_score_of_ligand_0": float(bs[0])}
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fo:
            fo.write(json.dumps(rec) + "\n")
    md.close()


if __name__ == "__main__":
    main()
