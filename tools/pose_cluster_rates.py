#!/usr/bin/env python
"""Wall and device time of `mdx_cluster_poses` (one call, one wait) against what a caller has without it: the stand-alone host build of
the same rule header (tests/cpp/pose_cluster_driver.cpp at -O2, single thread - a different program, not the code under test) on the
same inputs; and of `mdx_pose_rmsd` on the same poses, all pairs.  The arms are interleaved over three rounds.  Appends one JSON line per
(size, round) to profiles/pose_cluster_rates.jsonl.

Inputs: seven families of lig50 (or of a 256-atom molecule) jittered by 0.3 A inside small_complex's box, 1.9 A from the first, cut 2 A
(tests/pose_cluster_cases.py); the 2 perms are the identity and a swap, the 12 perms the images of a ring on atoms 0..5.  Device time:
the handle's own event brackets (mdx_profile(1)), one per kernel - pair tiles in nb_ms_sum, gather in bonded_ms_sum, leader scan in
integ_ms_sum, assignment in fused_ms_sum -, in a call of its own so that the wall figures carry no events.  The host baseline computes
only the pose-leader distances the greedy rule needs (N x clusters, not N x N): it is the cheapest host program, not a strawman - with
the standard inputs' seven clusters it is at its best; `--cut 0.5` makes every pose a leader, its worst."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from molchanica_amd import systems          # noqa: E402
from molchanica_amd.md_state import MdState          # noqa: E402
from tests import pose_cluster_cases as K          # noqa: E402
from tests.test_gpu_pose_batch import small_configs          # noqa: E402
from tests.test_pose_cluster_host import driver_input          # noqa: E402

SIZES = [(256, 50, 1), (256, 50, 2), (1024, 50, 1), (1024, 50, 2), (4096, 50, 1), (4096, 50, 2), (16384, 50, 1), (16384, 50, 2), (4096, 256, 12)]
KERNELS = (("tiles", "nb_ms_sum"), ("gather", "bonded_ms_sum"), ("scan", "integ_ms_sum"), ("assign", "fused_ms_sum"))


def perms_of(count, n_perms):
    if n_perms == 12:
        return K.ring_perms(count)
    p = np.tile(np.arange(count, dtype=np.uint32), (n_perms, 1))
    if n_perms == 2:
        p[1, [1, 4]] = [4, 1]
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-n", type=int, default=16384)
    ap.add_argument("--sizes", default="", help="n:count:n_perms,... instead of the standard list")
    ap.add_argument("--cut", type=float, default=K.CUT, help="RMSD cutoff in A; below the jitter every pose leads a cluster of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cluster_rates.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "pose_cluster_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pose_cluster_driver.cpp"), "-o", exe])
    L = K.periodic_edges()
    with MdState(systems.small_complex(), small_configs()[0]) as md:
        warm, ws, _ = K.families(12, 64, 1)
        md.cluster_poses(warm, ws, K.CUT)      # warm-up: code objects
        md.pose_rmsd(warm)

        def device_ms(call):
            md.profile(1)
            s0 = md.stats()
            call()
            s1 = md.stats()
            md.profile(0)
            return {k: s1[f] - s0[f] for k, f in KERNELS}

        sizes = [tuple(int(v) for v in w.split(":")) for w in a.sizes.split(",")] if a.sizes else SIZES
        for n, count, n_perms in sizes:
            if n > a.max_n:
                continue
            poses, scores, _ = K.families(count, n, 1000 + n + count, spacing=1.9)
            perms = perms_of(count, n_perms)
            path = driver_input(os.path.join(tmp, "in.bin"), 2, poses, scores, a.cut, None, perms, L)
            md.cluster_poses(poses, scores, a.cut, None, perms)      # buffers of this size
            md.pose_rmsd(poses[:min(n, 4096)], None, None, perms)
            for rnd in range(a.rounds):
                t0 = time.perf_counter()
                dev = md.cluster_poses(poses, scores, a.cut, None, perms)
                t_dev = time.perf_counter() - t0
                ms = device_ms(lambda: md.cluster_poses(poses, scores, a.cut, None, perms))
                out = subprocess.check_output([exe, path], text=True).split()
                t_host, k_host = float(out[1]), int(out[2])
                m = min(n, 4096)      # all pairs: 4096 x 4096 fp32 = 64 MiB back to the host
                t0 = time.perf_counter()
                md.pose_rmsd(poses[:m], None, None, perms)
                t_rmsd = time.perf_counter() - t0
                ms_rmsd = device_ms(lambda: md.pose_rmsd(poses[:m], None, None, perms))
                total = sum(ms.values())
                rec = {"n_poses": n, "count": count, "rmsd_cut": a.cut, "n_perms": n_perms, "round": rnd, "n_clusters": int(len(dev[0])), "same_cluster_count_on_host": bool(k_host == len(dev[0])),
                       "cluster_wall_s": t_dev, "cluster_device_ms": total, "cluster_kernel_ms": ms,
                       "dominant_kernel": max(ms, key=ms.get), "scan_share_of_device": ms["scan"] / total if total else None,
                       "host_rule_single_thread_s": t_host, "host_over_device_wall": t_host / t_dev,
                       "pair_atom_images_lower_triangle": n * (n - 1) // 2 * count * n_perms,
                       "pose_rmsd_n": m, "pose_rmsd_wall_s": t_rmsd, "pose_rmsd_tiles_ms": ms_rmsd["tiles"], "pose_rmsd_gather_ms": ms_rmsd["gather"]}
                print(json.dumps(rec), flush=True)
                with open(a.out, "a") as fo:
                    fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
