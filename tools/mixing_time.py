#!/usr/bin/env python
"""Time of one `mdx_solubility_mixing` call against the path a caller has without it - `mdx_download` plus the same fp32 pair loop in
C++ at -O3 on one thread (tools/mixing_host.cpp: the rule header, a different program from the code under test) - on the same box.
Appends one JSON line per size to profiles/mixing_time.jsonl.

Sizes.  "workflow": what setup_for of the reference's shrinking-box workflow (src/properties/sol_shrinking_box.rs:348-418) gives a
30-atom solute of 300 A^3 with 20 non-hydrogens: 40 copies (SOLUTE_COPY_COUNT; 40 x 300 / 0.14 A^3 is above the 34 A floor), a 44.1 A
target cube, round(0.84 x 1.2 x side^3 / 29.97) = 2883 waters.  "large": 200 x 30 atoms (all selected) in 30,000 waters, a 98 A cube.
The atoms sit on a jittered lattice, a copy on consecutive sites: the pair work does not depend on the geometry, and nothing is stepped.

Wall time: the mean of --calls calls after a warm-up.  Device time: the handle's own hipEvent brackets (mdx_profile(1)), in calls of their
own - pair kernel in nb_ms_sum, gather in bonded_ms_sum, slab sum in integ_ms_sum.  Pair rate = rows x (rows + waters) / pair kernel time."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from molchanica_amd import MdConfig, MdSystem, systems          # noqa: E402
from molchanica_amd import topology as topo          # noqa: E402
from molchanica_amd.md_state import MdState          # noqa: E402

SIZES = {"workflow": dict(n_copies=40, apc=30, n_sel=20, n_waters=2883, side=44.1),
         "large": dict(n_copies=200, apc=30, n_sel=30, n_waters=30000, side=98.0)}


def build(n_copies, apc, n_waters, side, seed=0) -> MdSystem:
    rng = np.random.default_rng(seed)
    n_sol = n_copies * apc
    m = int(np.ceil((n_sol + n_waters) ** (1 / 3)))
    g = (np.arange(m) + 0.5) * side / m
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    sol = sites[:n_sol] + rng.normal(scale=0.1, size=(n_sol, 3))
    wsites = sites[n_sol:][np.sort(rng.choice(len(sites) - n_sol, size=n_waters, replace=False))]
    wpos = systems._water_atoms(wsites, rng, 0.0)
    tp = systems._water_topology(n_sol, n_waters, 1, 2)
    off, idx = topo.csr_from_pairs(n_sol + 3 * n_waters, tp["excl_pairs"])
    return MdSystem(
        pos=np.concatenate([sol, wpos]), mass=np.concatenate([np.full(n_sol, 12.011), tp["mass"]]).astype(np.float32),
        charge=np.concatenate([np.zeros(n_sol), tp["charge"]]), lj_type=np.concatenate([np.zeros(n_sol, np.int64), tp["lj_type"]]),
        lj_sigma=[3.4, systems.TIP3P["o_sigma"], 0.0], lj_eps=[0.1, systems.TIP3P["o_eps"], 0.0], bond_idx=tp["bonds"], bond_k=tp["bond_k"],
        bond_r0=tp["bond_r0"], angle_idx=tp["angles"], angle_k=tp["angle_k"], angle_theta0=tp["angle_t0"], excl_offsets=off, excl_idx=idx,
        mol_start=np.concatenate([apc * np.arange(n_copies), n_sol + 3 * np.arange(n_waters)]), periodic=True, box_lo=(0, 0, 0),
        box_hi=(side, side, side), name=f"mixtime{n_copies}x{apc}w{n_waters}").normalise()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="workflow,large")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixing_time.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    so = os.path.join(tempfile.mkdtemp(), "mixing_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-shared", "-fPIC", "-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                           os.path.join(ROOT, "tools", "mixing_host.cpp"), "-o", so])
    host = C.CDLL(so).mixing_host
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    host.argtypes = [fp, C.c_uint32, C.c_uint32, C.c_uint32, up, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, fp, fp, fp]
    for name in a.sizes.split(","):
        z = SIZES[name]
        s = build(z["n_copies"], z["apc"], z["n_waters"], z["side"])
        sel = np.arange(z["n_sel"], dtype=np.uint32)
        n_sol = z["n_copies"] * z["apc"]
        rows, partners = z["n_copies"] * z["n_sel"], z["n_copies"] * z["n_sel"] + z["n_waters"]
        with MdState(s, MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.0)) as md:
            md.set_water_layout(n_sol, z["n_waters"], 3)
            md.set_solute_copies(0, z["n_copies"], z["apc"], sel)
            for _ in range(3):
                dev = md.solubility()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                md.solubility()
            wall_ms = (time.perf_counter() - t0) * 1e3 / a.calls
            md.profile(1)
            for _ in range(a.calls):
                md.solubility()
            st = md.stats()
            md.profile(0)
            pair_ms, gather_ms, sum_ms = (st[k] / a.calls for k in ("nb_ms_sum", "bonded_ms_sum", "integ_ms_sum"))
            lo, hi = md.cell()
            out = np.zeros(10, np.float32)
            t0 = time.perf_counter()
            for _ in range(a.host_calls):
                pos = md.positions()
                host(pos.ctypes.data_as(fp), 0, z["n_copies"], z["apc"], sel.ctypes.data_as(up), z["n_sel"], n_sol, 3, z["n_waters"],
                     lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), out.ctypes.data_as(fp))
            host_ms = (time.perf_counter() - t0) * 1e3 / a.host_calls
        rec = dict(size=name, **z, rows=rows, pairs=rows * partners, call_wall_ms=round(wall_ms, 4), pair_kernel_ms=round(pair_ms, 4),
                   gather_ms=round(gather_ms, 4), slab_sum_ms=round(sum_ms, 4), pairs_per_s=round(rows * partners / (pair_ms * 1e-3), 1),
                   download_plus_host_loop_ms=round(host_ms, 2), speedup=round(host_ms / wall_ms, 1), score_device=float(dev["score"]),
                   score_host=float(out[0]), local_mixing_device=float(dev["local_mixing"]), local_mixing_host=float(out[2]))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
