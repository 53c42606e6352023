"""Summarises rocprofv3's rocpd SQLite outputs (kernel trace + PMC passes) into small text/JSON
files for profiles/.  Usage: python tools/summarize_rocprof.py gpurun_out/r01 profiles r01"""
import glob
import json
import os
import re
import sqlite3
import sys

src, dst, tag = sys.argv[1], sys.argv[2], sys.argv[3]
os.makedirs(dst, exist_ok=True)


def short(name):
    """Kernel name without return type and argument list.  The pair kernels keep their template arguments
    <ENERGY, COUL, GEOM, SAMECUT, WPT, HALF>: the energy flavour (minimiser, snapshots, barostat) and the
    force-only flavour of the step loop are different kernels with different costs."""
    m = re.match(r"(?:void )?([A-Za-z0-9_]+)(<[^>]*>)?", name)
    if not m:
        return name
    if m.group(1).startswith("nb_") and m.group(2):
        return m.group(1) + m.group(2).replace(" ", "")
    return m.group(1)


def is_step_pair_kernel(k):
    return k.startswith("nb_") and "<false," in k


lines = []
# ---- kernel trace stats -------------------------------------------------------------------------
kt = glob.glob(os.path.join(src, "kt", "*.db"))
stats = {}
if kt:
    db = sqlite3.connect(kt[0])
    rows = db.execute("select name, start, end from kernels").fetchall()
    for name, st, en in rows:
        d = stats.setdefault(short(name), [0, 0.0, 1e30, 0.0])
        dur = (en - st) / 1e3
        d[0] += 1; d[1] += dur; d[2] = min(d[2], dur); d[3] = max(d[3], dur)
    total = sum(v[1] for v in stats.values())
    lines.append(f"# rocprofv3 --kernel-trace --stats  ({tag}; python3 bench.py --full --steps 300 --warmup 30 --no-cpu-baseline)")
    lines.append("# includes the untimed preparation of the box (minimiser = energy-flavour kernels, 600 thermostatted steps)")
    lines.append(f"{'kernel':58s} {'calls':>7s} {'total_us':>12s} {'avg_us':>10s} {'min_us':>10s} {'max_us':>10s} {'pct':>6s}")
    for k, v in sorted(stats.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"{k:58s} {v[0]:7d} {v[1]:12.1f} {v[1] / v[0]:10.2f} {v[2]:10.2f} {v[3]:10.2f} {100 * v[1] / total:6.2f}")
    lines.append("")
    lines.append("note: pair-kernel launches that were gated off behind a stale neighbour list (no-ops, a few us)")
    lines.append("      are included in 'calls'; see the per-kernel avg of launches > 100 us below.")
    big = [(en - st) / 1e3 for name, st, en in rows if is_step_pair_kernel(short(name)) and (en - st) > 100e3]
    if big:
        lines.append(f"pair kernel of the step loop (force-only flavour), executed launches only: n={len(big)} "
                     f"avg_us={sum(big) / len(big):.2f} min_us={min(big):.2f} max_us={max(big):.2f}")
    # dual pair list: <...,1> walks the inner list, <...,2> is the pruning pass (walks the Verlet list); each step
    # enqueues both and the device runs one (the other returns at once and shows up as a ~4 us launch)
    per = {}
    for name, st, en in rows:
        k = short(name)
        if is_step_pair_kernel(k) and (en - st) > 100e3:
            per.setdefault(k, []).append((en - st) / 1e3)
    for k, v in sorted(per.items()):
        lines.append(f"  executed {k}: n={len(v)} avg_us={sum(v) / len(v):.2f} min_us={min(v):.2f} max_us={max(v):.2f}")

# ---- PMC passes ----------------------------------------------------------------------------------
pmc = {}
for d in sorted(glob.glob(os.path.join(src, "pmc_*"))):
    dbs = glob.glob(os.path.join(d, "*.db"))
    if not dbs or not os.path.isdir(d):
        continue
    db = sqlite3.connect(dbs[0])
    try:
        cols = [r[1] for r in db.execute("pragma table_info(counters_collection)")]
        rows = db.execute("select * from counters_collection").fetchall()
    except Exception as e:  # pragma: no cover
        lines.append(f"{d}: {e}")
        continue
    ci = {c: i for i, c in enumerate(cols)}
    kname = "kernel_name" if "kernel_name" in ci else ("name" if "name" in ci else None)
    cname = "counter_name" if "counter_name" in ci else "pmc_name"
    vname = "value" if "value" in ci else "counter_value"
    if kname is None:
        lines.append(f"{d}: unknown schema {cols}")
        continue
    dur_ok = "start" in ci and "end" in ci
    for r in rows:
        k = short(r[ci[kname]])
        if dur_ok and k.startswith("nb_") and (r[ci["end"]] - r[ci["start"]]) < 100e3:
            continue   # gated no-op launch
        e = pmc.setdefault(k, {}).setdefault(r[ci[cname]], [0, 0.0])
        e[0] += 1; e[1] += float(r[ci[vname]])
if pmc:
    lines.append("")
    lines.append(f"# rocprofv3 --pmc (separate passes; mean per executed dispatch)   ({tag})")
    for k, cs in sorted(pmc.items()):
        if not k.startswith(("nb_", "bonded", "integrate", "build_list", "prune_list", "rb_")):
            continue
        lines.append(k)
        for c, (n, tot) in sorted(cs.items()):
            lines.append(f"    {c:28s} n={n:5d} mean={tot / n:18.1f}")

open(os.path.join(dst, f"{tag}_rocprof_summary.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))

# ---- HBM traffic of the pair kernel (MI355X_MICROARCH.md §HBM: FETCH_SIZE on gfx950 reports 1/2 of the
# bytes of wide coalesced reads -> x2; units are KiB-ish 'FETCH_SIZE'=KB, WRITE_SIZE uncalibrated) ----
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from molchanica_amd._build_info import pair_kernel_rev as _pair_kernel_rev  # noqa: E402
nbk = sorted((k for k in pmc if is_step_pair_kernel(k)), key=lambda k: -max(v[0] for v in pmc[k].values()))
if nbk:
    cs = pmc[nbk[0]]
    raw = {c: v[1] / v[0] for c, v in cs.items()}
    json.dump({"kernel": nbk[0], "raw": raw}, open(os.path.join(dst, f"{tag}_nb_pmc_raw.json"), "w"), indent=1)
    if "FETCH_SIZE" in raw and "WRITE_SIZE" in raw:
        fetch, write = raw["FETCH_SIZE"] * 1024.0, raw["WRITE_SIZE"] * 1024.0
        traffic = {
            "workload": "water1M", "kernel": nbk[0], "round": tag,
            "kernel_rev": _pair_kernel_rev(),   # = bench.py's NB_KERNEL_REV (molchanica_amd/_build_info.py)
            "source": f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, {tag}",
            "FETCH_SIZE_KB_per_launch": raw["FETCH_SIZE"], "WRITE_SIZE_KB_per_launch": raw["WRITE_SIZE"],
            "correction": "MI355X_MICROARCH.md HBM section: on gfx950 FETCH_SIZE tallies 128-B read requests at 64 B -> x2 "
                          "for wide coalesced reads; WRITE_SIZE taken as reported (uncalibrated)",
            "hbm_bytes_per_launch": 2.0 * fetch + write, "hbm_bytes_per_launch_uncorrected": fetch + write,
            "algorithmic_bytes_per_launch": 32.0 * 1029000,
            "note": "memory-side (fabric) request bytes.  Reads: pair list (3.2 M entries x 8 B) + posq/lj of j-clusters that miss "
                    "the 4 MiB per-XCD L2.  Writes: the half-list kernel returns the reaction force with f32 atomics, which "
                    "gfx950 executes on the memory side - ~88 M atomic words per launch appear here as write requests "
                    "(~6 B each); the full-list kernel (nb_variant 2) writes 16.5 MB, exactly the force array, and is 40 % slower",
        }
        json.dump(traffic, open(os.path.join(dst, "nb_traffic.json"), "w"), indent=1)
