#!/usr/bin/env python
"""Cost per pose of `mdx_pose_forces` against the loop it replaces (`mdx_upload_range` + `mdx_energy`, the force call, +
`mdx_download(MDX_FORCE)`), same poses, same process, the arms interleaved over three rounds; beside it the energy-only
`mdx_score_poses` over the same batch.  Appends one JSON line per (system, batch size, round) to profiles/pose_force_rates.jsonl.

Systems and poses are those of tools/pose_batch_rates.py.  The loop arm is timed over at most --loop-cap poses of the batch (its cost
per pose does not depend on the batch).  Device times: the handle's own event brackets around the kernels of a call (mdx_profile), in
calls of their own so that the wall figures carry no events.  `last_atom_force_loop` is the whole force of the step loop (bonded terms
included), `last_atom_force_batch` the non-bonded pose force: they show that both arms ran, they are not meant to agree."""
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def device_ms(md, fn):
    md.profile(1)
    fn()
    ms = md.stats()["nb_ms_sum"]
    md.profile(0)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="complex50k,dhfr23k")
    ap.add_argument("--batches", default="1,64,1024,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_force_rates.jsonl"))
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
            warm = poses_of(start, 4, 1)
            md.score_poses(lo, warm)      # warm-up: tables, buffers
            md.pose_forces(lo, warm, rigid=True)
            for p in (int(v) for v in a.batches.split(",")):
                poses = poses_of(start, p, 100 + p)
                n_loop = min(p, a.loop_cap)
                for rnd in range(a.rounds):
                    t_force, (f, rows, rigid) = timed(lambda: md.pose_forces(lo, poses, rigid=True))
                    t_score, _ = timed(lambda: md.score_poses(lo, poses))
                    dev_force = device_ms(md, lambda: md.pose_forces(lo, poses, rigid=True))
                    dev_score = device_ms(md, lambda: md.score_poses(lo, poses))
                    t0 = time.perf_counter()
                    for k in range(n_loop):
                        md.set_positions_range(lo, poses[k])
                        md.energy()
                        fl = md.forces()
                    t_loop = time.perf_counter() - t0
                    md.set_positions_range(lo, start.astype(np.float32))
                    md.energy()
                    rec = {"system": name, "n_atoms": s.n_atoms, "ligand_atoms": hi - lo, "n_poses": p, "round": rnd,
                           "forces_wall_us_per_pose": 1e6 * t_force / p, "forces_device_us_per_pose": 1e3 * dev_force / p,
                           "score_wall_us_per_pose": 1e6 * t_score / p, "score_device_us_per_pose": 1e3 * dev_score / p,
                           "forces_over_score_device": dev_force / dev_score,
                           "loop_poses_timed": n_loop, "loop_wall_us_per_pose": 1e6 * t_loop / n_loop,
                           "loop_over_forces": (t_loop / n_loop) / (t_force / p),
                           "last_atom_force_batch": [float(v) for v in f[n_loop - 1, -1]],
                           "last_atom_force_loop": [float(v) for v in fl[hi - 1]]}
                    print(json.dumps(rec), flush=True)
                    with open(a.out, "a") as fo:
                        fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
