#!/usr/bin/env python
"""Wall time of `mdx_search_poses` (the device search: one call, one wait per chunk of 256 walkers) against the host loop it replaces -
one `MdState.refine_poses_flex` call per round for the whole batch plus the move and the decision of tests/pose_search_ref.py in numpy -,
in the same process, the two arms interleaved over three rounds.  Appends one JSON line per (batch size, round) to
profiles/pose_search_rates.jsonl.

complex50k of tools/pose_batch_rates.py: the range is the 50-atom ligand with all its rotatable bonds (root 0) and its dihedral terms; the
walkers start from the placements of tools/pose_flex_rates.py.  Tolerances are 0 and max_evals is fixed; times are divided by the
evaluations actually taken.  The host arm is timed twice over: the whole loop, and the part spent inside `refine_poses_flex` - the parent's
code and the fair baseline, since the numpy move around it is the tool's own.  Device time: the handle's own event bracket around the
launches of a chunk (mdx_profile), in a call of its own so that the wall figures carry no events."""
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
from tests import pose_search_ref as S          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="complex50k")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--n-rounds", type=int, default=8)
    ap.add_argument("--max-evals", type=int, default=16)
    ap.add_argument("--moves", default="0.5,0.15,0.4")
    ap.add_argument("--kT", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_search_rates.jsonl"))
    a = ap.parse_args()
    moves = tuple(float(v) for v in a.moves.split(","))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    s, g, lo, hi = setup(a.system)
    n = hi - lo
    bonds = F.local_bonds(s, lo, hi)
    tb = F.rotatable_bonds(n, bonds, 0)[:F.MAX_TORSIONS]
    tors = F.moving_sides(n, bonds, 0, tb)
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
        md.refine_poses_flex(lo, warm, 0, tb, 2, 0.0, 0.0, 0.0)      # warm-up: tables, buffers, code objects
        md.search_poses(lo, warm, 0, tb, 2, *moves, a.kT, a.seed, 2, 0.0, 0.0, 0.0)
        in_call = [0.0]

        def refine_all(X):
            t0 = time.perf_counter()
            y, rows, rigid, xform, dih, tgrad, status, evals = md.refine_poses_flex(lo, np.ascontiguousarray(X), 0, tb, a.max_evals, 0.0, 0.0, 0.0)
            in_call[0] += time.perf_counter() - t0
            return y, rows, dih, status, evals

        def search():
            return md.search_poses(lo, starts, 0, tb, a.n_rounds, *moves, a.kT, a.seed, a.max_evals, 0.0, 0.0, 0.0)

        for w in (int(v) for v in a.batches.split(",")):
            starts = placements(w, 100 + w)
            for rnd in range(a.rounds):
                t0 = time.perf_counter()
                dev = search()
                t_dev = time.perf_counter() - t0
                md.profile(1)
                search()
                ms_dev = md.stats()["nb_ms_sum"]
                md.profile(0)
                in_call[0] = 0.0
                t0 = time.perf_counter()
                host = S.search_batch(starts, refine_all, tors, a.n_rounds, *moves, a.kT, a.seed)
                t_host = time.perf_counter() - t0
                ev_dev, ev_host = int(dev[5][:, 3].sum()), int(host[5][:, 3].sum())
                one = md.search_poses(lo, starts, 0, tb, 1, *moves, a.kT, a.seed, a.max_evals, 0.0, 0.0, 0.0)
                rec = {"system": a.system, "n_atoms": s.n_atoms, "ligand_atoms": n, "n_torsions": len(tors), "n_walkers": w, "round": rnd,
                       "n_rounds": a.n_rounds, "max_evals": a.max_evals, "moves": moves, "kT": a.kT, "evals_device_search": ev_dev, "evals_host_loop": ev_host,
                       "device_search_wall_s": t_dev, "device_search_device_s": 1e-3 * ms_dev, "host_loop_wall_s": t_host,
                       "host_loop_in_refine_poses_flex_s": in_call[0],
                       "device_search_wall_us_per_walker_eval": 1e6 * t_dev / ev_dev,
                       "device_search_device_us_per_walker_eval": 1e3 * ms_dev / ev_dev,
                       "host_loop_wall_us_per_walker_eval": 1e6 * t_host / ev_host,
                       "host_loop_in_refine_poses_flex_us_per_walker_eval": 1e6 * in_call[0] / ev_host,
                       "host_calls_over_device_search": in_call[0] / t_dev, "host_loop_over_device_search": t_host / t_dev,
                       "device_search_wall_exceeds_host_loop": bool(t_dev > t_host),
                       "same_best_round_and_counters": bool(np.array_equal(dev[4], host[4]) and np.array_equal(dev[5], host[5])),
                       "best_coordinates_not_bit_equal": int((dev[0].view(np.uint32) != host[0].view(np.uint32)).sum()),
                       "smallest_metropolis_margin": host[6],
                       "rounds_accepted": int(dev[5][:, 0].sum()), "accepted_uphill": int(dev[5][:, 1].sum()), "non_finite_rounds": int(dev[5][:, 2].sum()),
                       "median_best_score": float(np.median(dev[2])), "median_score_after_round_0": float(np.median(one[2]))}
                print(json.dumps(rec), flush=True)
                with open(a.out, "a") as fo:
                    fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
