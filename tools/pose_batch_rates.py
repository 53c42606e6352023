#!/usr/bin/env python
"""Cost per pose of `mdx_score_poses` against the loop it replaces (`mdx_upload_range` + `mdx_energy_between_mols`), same poses, same
process, the two arms interleaved over three rounds.  Appends one JSON line per (system, batch size, round) to
profiles/pose_batch_rates.jsonl.

Systems: complex50k (receptor / 50-atom ligand / solvent) and dhfr23k (the chain / its first 16 waters standing in for a ligand: the box
holds no other small molecule / the rest of the water).  Poses: rigid moves within 3 A / 0.3 rad of the start.  The loop arm is timed
over at most --loop-cap poses of the batch (its cost per pose does not depend on the batch).  Device time of the batch: the handle's
own event brackets around the two kernels (mdx_profile), in a run of its own so that the wall figures carry no events."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from molchanica_amd import MdConfig, systems          # noqa: E402
from molchanica_amd.md_state import MdState          # noqa: E402


def poses_of(lig, n, seed):
    rng = np.random.default_rng(seed)
    c = lig.mean(0)
    out = np.empty((n,) + lig.shape, np.float32)
    for k in range(n):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = 0.3 * rng.random()
        kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        rot = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        out[k] = (lig - c) @ rot.T + c + d * 3.0 * rng.random()
    return out


def setup(name):
    if name == "complex50k":
        s = systems.complex50k()
        lo, hi = int(s.mol_start[1]), int(s.mol_start[2])
    else:
        s = systems.dhfr23k()
        lo = int(s.mol_start[1])
        hi = int(s.mol_start[17])
    g = np.full(s.n_atoms, 2, np.uint8)
    g[:lo] = 0
    g[lo:hi] = 1
    return s, g, lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="complex50k,dhfr23k")
    ap.add_argument("--batches", default="1,64,1024,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_batch_rates.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name in a.systems.split(","):
        s, g, lo, hi = setup(name)
        with MdState(s, MdConfig()) as md:
            md.set_energy_groups(g, 3)
            md.energy()
            start = md.positions()[lo:hi].astype(np.float64)
            box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
            start = start - np.round((start - start[0]) / box) * box
            md.score_poses(lo, poses_of(start, 4, 1))      # warm-up: tables, buffers
            for p in (int(v) for v in a.batches.split(",")):
                poses = poses_of(start, p, 100 + p)
                n_loop = min(p, a.loop_cap)
                for rnd in range(a.rounds):
                    t0 = time.perf_counter()
                    rows = md.score_poses(lo, poses)
                    t_batch = time.perf_counter() - t0
                    md.profile(1)
                    md.score_poses(lo, poses)
                    dev_ms = md.stats()["nb_ms_sum"]
                    md.profile(0)
                    t0 = time.perf_counter()
                    for k in range(n_loop):
                        md.set_positions_range(lo, poses[k])
                        m = md.energy_between_mols()
                    t_loop = time.perf_counter() - t0
                    md.set_positions_range(lo, start.astype(np.float32))
                    md.energy_between_mols()
                    rec = {"system": name, "n_atoms": s.n_atoms, "ligand_atoms": hi - lo, "n_poses": p, "round": rnd,
                           "batch_wall_us_per_pose": 1e6 * t_batch / p, "batch_device_us_per_pose": 1e3 * dev_ms / p,
                           "loop_poses_timed": n_loop, "loop_wall_us_per_pose": 1e6 * t_loop / n_loop,
                           "loop_over_batch": (t_loop / n_loop) / (t_batch / p),
                           "last_row_batch": [float(v) for v in rows[n_loop - 1]], "last_row_loop": [float(v) for v in m[1]]}
                    print(json.dumps(rec), flush=True)
                    with open(a.out, "a") as f:
                        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
