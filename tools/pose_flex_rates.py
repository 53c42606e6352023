#!/usr/bin/env python
"""Cost per pose-evaluation of `mdx_refine_poses_flex` (the flexible device loop) against `mdx_refine_poses` (the rigid device loop) on
the same poses and against the host loop it replaces - one `MdState.pose_forces` call per evaluation plus the numpy stepper of
tests/pose_flex_ref.py -, in the same process, the arms interleaved over three rounds.  Appends one JSON line per (system, batch size,
round) to profiles/pose_flex_rates.jsonl.

Systems and rigid placements are those of tools/pose_batch_rates.py.  On complex50k the range is the 50-atom ligand: all its rotatable
bonds are declared (root 0), the ligand's dihedral terms are on, and the placements have their torsions turned by 0.3 u w^2 rad as in
the tests.  On dhfr23k the range of that tool is sixteen waters: no torsion exists there, so the flexible arm runs with none and shows
what the larger step kernel costs by itself.  Tolerances are 0 and max_evals is fixed; the evaluations actually taken are what the
times are divided by.  The host arm runs over at most --loop-cap poses and is timed twice over: the whole loop, and the part spent inside
`pose_forces`.  Device time: the handle's own event bracket around the launches of a chunk (mdx_profile), in a call of its own so that the
wall figures carry no events."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from molchanica_amd import MdConfig          # noqa: E402
from molchanica_amd.md_state import MdState          # noqa: E402
from pose_batch_rates import poses_of, setup          # noqa: E402
from tests import pose_flex_ref as F          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="complex50k,dhfr23k")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--max-evals", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_flex_rates.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name in a.systems.split(","):
        s, g, lo, hi = setup(name)
        n = hi - lo
        bonds = F.local_bonds(s, lo, hi)
        try:
            tb = F.rotatable_bonds(n, bonds, 0)[:F.MAX_TORSIONS]
            tors = F.moving_sides(n, bonds, 0, tb)
        except F.GraphError:      # (the range is not one bonded molecule)
            tb, tors = np.zeros((0, 2), np.uint32), []
        terms = F.dihedral_terms(s, lo, hi)
        box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
        with MdState(s, MdConfig()) as md:
            md.set_energy_groups(g, 3)
            md.energy()
            start = md.positions()[lo:hi].astype(np.float64)
            start = start - np.round((start - start[0]) / box) * box

            def placements(p, seed):
                out = poses_of(start, p, seed).astype(np.float64)
                rng = np.random.default_rng(seed + 1000)
                for k in range(1, p):
                    out[k] = F.turn(out[k], tors, 0.3 * rng.uniform(-1.0, 1.0, len(tors)) * rng.random(len(tors)) ** 2)
                return out.astype(np.float32)

            warm = placements(4, 1)
            md.pose_forces(lo, warm, rigid=True)      # warm-up: tables, buffers, code objects
            md.refine_poses(lo, warm, 2, 0.0, 0.0)
            md.refine_poses_flex(lo, warm, 0, tb, 2, 0.0, 0.0, 0.0)
            in_call = [0.0]
            inner = F.host_evaluate(md, lo, 3)

            def evaluate(Y):
                t0 = time.perf_counter()
                out = inner(Y)
                in_call[0] += time.perf_counter() - t0
                return out

            def timed(call):
                t0 = time.perf_counter()
                out = call()
                wall = time.perf_counter() - t0
                md.profile(1)
                call()
                dev_ms = md.stats()["nb_ms_sum"]
                md.profile(0)
                return out, wall, dev_ms

            for p in (int(v) for v in a.batches.split(",")):
                poses = placements(p, 100 + p)
                n_host = min(p, a.loop_cap)
                for rnd in range(a.rounds):
                    flex, t_flex, ms_flex = timed(lambda: md.refine_poses_flex(lo, poses, 0, tb, a.max_evals, 0.0, 0.0, 0.0))
                    rigid, t_rigid, ms_rigid = timed(lambda: md.refine_poses(lo, poses, a.max_evals, 0.0, 0.0))
                    in_call[0] = 0.0
                    t0 = time.perf_counter()
                    host = F.refine_batch(poses[:n_host], evaluate, tors, terms, a.max_evals, 0.0, 0.0, 0.0, box=box)
                    t_host = time.perf_counter() - t0
                    ev_flex, ev_rigid, ev_host = int(flex[7].sum()), int(rigid[5].sum()), int(host[7].sum())
                    S0 = md.score_poses(lo, poses).astype(np.float64).sum(1)
                    E0 = np.array([float(np.float32(F.dihedral(q, terms, box)[0])) for q in poses[:n_host]])
                    rec = {"system": name, "n_atoms": s.n_atoms, "ligand_atoms": n, "n_torsions": len(tors), "dihedral_terms": len(terms[0]),
                           "n_poses": p, "round": rnd, "max_evals": a.max_evals, "evals_flex_loop": ev_flex, "evals_rigid_loop": ev_rigid,
                           "host_poses_timed": n_host, "evals_host_loop": ev_host,
                           "flex_loop_wall_us_per_pose_eval": 1e6 * t_flex / ev_flex,
                           "flex_loop_device_us_per_pose_eval": 1e3 * ms_flex / ev_flex,
                           "rigid_loop_wall_us_per_pose_eval": 1e6 * t_rigid / ev_rigid,
                           "rigid_loop_device_us_per_pose_eval": 1e3 * ms_rigid / ev_rigid,
                           "host_loop_wall_us_per_pose_eval": 1e6 * t_host / ev_host,
                           "host_loop_in_pose_forces_us_per_pose_eval": 1e6 * in_call[0] / ev_host,
                           "flex_over_rigid_device": (ms_flex / ev_flex) / (ms_rigid / ev_rigid),
                           "flex_over_rigid_wall": (t_flex / ev_flex) / (t_rigid / ev_rigid),
                           "host_calls_over_flex_loop": (in_call[0] / ev_host) / (t_flex / ev_flex),
                           "host_loop_over_flex_loop": (t_host / ev_host) / (t_flex / ev_flex),
                           "same_status_and_evals": bool(np.array_equal(flex[6][:n_host], host[6]) and np.array_equal(flex[7][:n_host], host[7])),
                           "coordinates_not_bit_equal": int((flex[0][:n_host].view(np.uint32) != host[0].view(np.uint32)).sum()),
                           "median_decrease_flex_kcal_mol": float(np.median(S0[:n_host] + E0 - flex[1][:n_host].astype(np.float64).sum(1)
                                                                            - flex[4][:n_host].astype(np.float64))),
                           "median_decrease_rigid_kcal_mol": float(np.median(S0[:n_host] - rigid[1][:n_host].astype(np.float64).sum(1)))}      # (both medians over the host arm's poses)
                    print(json.dumps(rec), flush=True)
                    with open(a.out, "a") as fo:
                        fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
