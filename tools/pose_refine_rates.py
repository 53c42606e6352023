#!/usr/bin/env python
"""Cost per pose-evaluation of `mdx_refine_poses` (the device loop) against the host loop it replaces - one `MdState.pose_forces` call per
evaluation plus the numpy stepper of tests/pose_refine_ref.py - on the same poses, in the same process, the arms interleaved over
three rounds.  Appends one JSON line per (batch size, round) to profiles/pose_refine_rates.jsonl.

System and poses are those of tools/pose_batch_rates.py (complex50k).  Tolerances are 0 and max_evals is fixed, so every pose runs all
its evaluations unless its step length runs out; the evaluations actually taken are what the times are divided by.  The host arm runs
over at most --loop-cap poses of the batch (its cost per pose does not depend on the batch) and is timed twice over: the whole loop,
and the part spent inside `pose_forces` - upload, three launches, read-back, wait - which is what the device loop saves; the numpy
stepper around it is this tool's, not the caller's.  Device time: the handle's own event bracket around the launches of a chunk
(mdx_profile), in a call of its own so that the wall figures carry no events."""
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
from tests import pose_refine_ref as P          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="complex50k")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--max-evals", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine_rates.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    s, g, lo, hi = setup(a.system)
    with MdState(s, MdConfig()) as md:
        md.set_energy_groups(g, 3)
        md.energy()
        start = md.positions()[lo:hi].astype(np.float64)
        box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
        start = start - np.round((start - start[0]) / box) * box
        warm = poses_of(start, 4, 1)
        md.pose_forces(lo, warm, rigid=True)      # warm-up: tables, buffers, code objects
        md.refine_poses(lo, warm, 2, 0.0, 0.0)
        in_call = [0.0]
        inner = P.host_evaluate(md, lo, 3)

        def evaluate(Y):
            t0 = time.perf_counter()
            out = inner(Y)
            in_call[0] += time.perf_counter() - t0
            return out

        for p in (int(v) for v in a.batches.split(",")):
            poses = poses_of(start, p, 100 + p)
            n_host = min(p, a.loop_cap)
            for rnd in range(a.rounds):
                t0 = time.perf_counter()
                dev = md.refine_poses(lo, poses, a.max_evals, 0.0, 0.0)
                t_dev = time.perf_counter() - t0
                md.profile(1)
                md.refine_poses(lo, poses, a.max_evals, 0.0, 0.0)
                dev_ms = md.stats()["nb_ms_sum"]
                md.profile(0)
                in_call[0] = 0.0
                t0 = time.perf_counter()
                host = P.refine_batch(poses[:n_host], evaluate, a.max_evals, 0.0, 0.0)
                t_host = time.perf_counter() - t0
                ev_dev, ev_host = int(dev[5].sum()), int(host[5].sum())
                rec = {"system": a.system, "n_atoms": s.n_atoms, "ligand_atoms": hi - lo, "n_poses": p, "round": rnd,
                       "max_evals": a.max_evals, "evals_device_loop": ev_dev, "host_poses_timed": n_host, "evals_host_loop": ev_host,
                       "device_loop_wall_us_per_pose_eval": 1e6 * t_dev / ev_dev,
                       "device_loop_device_us_per_pose_eval": 1e3 * dev_ms / ev_dev,
                       "host_loop_wall_us_per_pose_eval": 1e6 * t_host / ev_host,
                       "host_loop_in_pose_forces_us_per_pose_eval": 1e6 * in_call[0] / ev_host,
                       "host_calls_over_device_loop": (in_call[0] / ev_host) / (t_dev / ev_dev),
                       "same_status_and_evals": bool(np.array_equal(dev[4][:n_host], host[4]) and np.array_equal(dev[5][:n_host], host[5])),
                       "coordinates_not_bit_equal": int((dev[0][:n_host].view(np.uint32) != host[0].view(np.uint32)).sum()),
                       "median_decrease_kcal_mol": float(np.median(md.score_poses(lo, poses).astype(np.float64).sum(1)
                                                        - dev[1].astype(np.float64).sum(1)))}
                print(json.dumps(rec), flush=True)
                with open(a.out, "a") as fo:
                    fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
