#!/usr/bin/env python3
"""How does the pair launch END?  Resident waves over time and idle SIMD-time of one inner-list walk at water1M.

Needs a library with the wave clocks compiled in (off by default, like NB_HALF_STATS):

    make -C molchanica_amd/csrc clean all EXTRA=-DNB_DRAIN_TRACE       # or build a copy and point MDX_LIB at it
    python3 tools/pair_drain.py [--steps 8] [--bins 24] [--raw FILE.npz] > profiles/pair_drain.txt

Every wave of the merged dual-list launch writes the constant-rate clock (wall_clock64, 100 MHz) at entry and at exit and the SIMD it
ran on (HW_ID, XCC_ID).  The atoms are frozen (dt = 1e-9 ps, as tools/exp_split_cost.py does), so after the first pruning pass every
launch walks the same inner list; the LAST launch is analysed:
  (a) resident waves over time;
  (b) the share of the launch's SIMD-time (1024 SIMDs x launch length) a SIMD spends with 0 and with 1 resident wave;
  (c) how the busy time (>= 1 resident wave) and the wave-time (sum of wave lifetimes) spread over the SIMDs.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

TICK_US = 0.01      # wall_clock64: 100 MHz


def analyse(rec, bins, out=sys.stdout):
    """rec: uint32 [n_waves, 8] = t0 lo, t0 hi, t1 lo, t1 hi, HW_ID, XCC_ID, pruning pass, written."""
    p = lambda *a: print(*a, file=out)
    rec = rec[rec[:, 7] == 1]
    t0 = rec[:, 0].astype(np.int64) | (rec[:, 1].astype(np.int64) << 32)
    t1 = rec[:, 2].astype(np.int64) | (rec[:, 3].astype(np.int64) << 32)
    hw, xcc = rec[:, 4], rec[:, 5] & 0xF
    # gfx9 HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13.  The key only has to tell SIMDs apart.
    key = (xcc.astype(np.int64) << 16) | (hw & 0xFF30).astype(np.int64)
    simds, sidx = np.unique(key, return_inverse=True)
    S = len(simds)
    start, end = int(t0.min()), int(t1.max())
    L = end - start
    life = (t1 - t0) * TICK_US
    p(f"waves {len(rec)}  pruning pass {int(rec[:, 6].max())}  SIMDs seen {S}  XCDs seen {len(np.unique(xcc))}")
    p(f"launch length (first entry to last exit) {L * TICK_US:.1f} us; wave lifetime us: mean {life.mean():.1f}  p5 {np.percentile(life, 5):.1f}  "
      f"median {np.median(life):.1f}  p95 {np.percentile(life, 95):.1f}  max {life.max():.1f}")
    p(f"wave-time / (SIMDs x launch length) = mean resident waves per SIMD {life.sum() / (S * L * TICK_US):.3f}")
    # (a) resident waves over time
    p("\n(a) resident waves over time (mean over the bin; slots = SIMDs x 4)")
    p(f"{'from_us':>9s} {'to_us':>9s} {'resident':>9s} {'per_SIMD':>9s} {'entries':>8s} {'exits':>8s}")
    edges = np.linspace(start, end, bins + 1)
    for b in range(bins):
        lo, hi = edges[b], edges[b + 1]
        ov = np.clip(np.minimum(t1, hi) - np.maximum(t0, lo), 0, None).sum() / (hi - lo)
        p(f"{(lo - start) * TICK_US:9.1f} {(hi - start) * TICK_US:9.1f} {ov:9.0f} {ov / S:9.2f} {int(((t0 >= lo) & (t0 < hi)).sum()):8d} "
          f"{int(((t1 > lo) & (t1 <= hi)).sum()):8d}")
    # (b) per SIMD: time with k resident waves, by an event sweep
    occ = np.zeros((S, 8))          # [simd, k] ticks with k resident waves (k capped at 7)
    busy_end = np.zeros(S, np.int64)
    first_in = np.zeros(S, np.int64)
    order = np.argsort(sidx, kind="stable")
    bounds = np.searchsorted(sidx[order], np.arange(S + 1))
    for s in range(S):
        w = order[bounds[s]:bounds[s + 1]]
        ev = np.concatenate([np.stack([t0[w], np.ones(len(w), np.int64)], 1), np.stack([t1[w], -np.ones(len(w), np.int64)], 1)])
        ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
        k, t = 0, start
        for tt, d in ev:
            occ[s, min(k, 7)] += tt - t
            t, k = tt, k + d
        occ[s, 0] += end - t
        busy_end[s], first_in[s] = t1[w].max(), t0[w].min()
    tot = float(S) * L
    p("\n(b) share of the launch's SIMD-time with k resident waves")
    p("   " + "  ".join(f"k={k}: {100 * occ[:, k].sum() / tot:5.2f} %" for k in range(6)))
    head0 = (first_in - start).sum() / tot
    tail0 = (end - busy_end).sum() / tot
    p(f"   of k=0: before the SIMD's first wave {100 * head0:.2f} %, after its last wave {100 * tail0:.2f} %, between {100 * (occ[:, 0].sum() / tot - head0 - tail0):.2f} %")
    # the closing stretch on its own: from the moment the first SIMD runs dry of queued work (first exit not followed by an entry
    # on that SIMD) - approximated by the last entry of the launch - to the end
    last_entry = int(t0.max())
    p(f"   last wave enters at {(last_entry - start) * TICK_US:.1f} us = {100 * (last_entry - start) / L:.1f} % of the launch; the stretch after it is "
      f"{(end - last_entry) * TICK_US:.1f} us")
    tail_w = np.clip(t1 - np.maximum(t0, last_entry), 0, None).sum()
    p(f"   mean resident waves per SIMD after the last entry: {tail_w / (S * max(end - last_entry, 1)):.2f}")
    # (c) spread over the SIMDs
    busy = (L - occ[:, 0]) * TICK_US
    wt = np.array([life[order[bounds[s]:bounds[s + 1]]].sum() for s in range(S)])
    nw = np.diff(bounds)
    p("\n(c) spread over the SIMDs")
    for name, v in (("busy time us (>= 1 wave)", busy), ("wave-time us (sum of lifetimes)", wt), ("waves per SIMD", nw.astype(float)),
                    ("last exit us after launch start", (busy_end - start) * TICK_US)):
        p(f"   {name:34s} min {v.min():8.1f}  p5 {np.percentile(v, 5):8.1f}  median {np.median(v):8.1f}  p95 {np.percentile(v, 95):8.1f}  max {v.max():8.1f}  "
          f"std {v.std():7.1f}")
    # the drain figure the decision rule uses: SIMD-time with no resident wave, plus half of the SIMD-time with one resident wave (a lone wave
    # issues its dependent VALU stream at half the rate two or more reach together)
    drain = (occ[:, 0].sum() + 0.5 * occ[:, 1].sum()) / tot
    p(f"\ndrain = k=0 share + half of the k=1 share = {100 * drain:.2f} % of the launch's SIMD-time")
    return drain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--bins", type=int, default=24)
    ap.add_argument("--raw", default=None, help="also save the records (npz)")
    ap.add_argument("--from-raw", default=None, help="analyse saved records, no GPU")
    ap.add_argument("--system", default="water1M")
    args = ap.parse_args()
    if args.from_raw:
        analyse(np.load(args.from_raw)["rec"], args.bins)
        return
    from molchanica_amd import MdConfig, systems
    from molchanica_amd.md_state import MdState, load_library
    lib = load_library()
    if not hasattr(lib, "mdx_debug_drain_trace"):
        sys.exit("this libmdx.so has no wave clocks: build with EXTRA=-DNB_DRAIN_TRACE")
    lib.mdx_debug_drain_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    lib.mdx_debug_drain_trace.restype = C.c_int
    cfg = MdConfig(skin=2.0, chunk_steps=16)
    system = systems.BY_NAME[args.system]()
    with MdState(system, cfg) as eq:      # the box bench.py times: minimised, 300 K, 600 thermostatted steps
        eq.minimize_energy(100)
        eq.initialize_velocities(300.0, True, seed=105)
        eq.set_thermostat(1, 300.0, 0.02, 1)
        eq.step(0.0005, None, 600)
        pos = eq.positions()
    system.pos = np.ascontiguousarray(pos, np.float32)
    system.vel = np.zeros_like(system.pos)
    with MdState(system, cfg) as md:
        md.step(1e-9, None, 20)
        lib.mdx_debug_drain_trace(md._h, 1, None, 0)
        md.step(1e-9, None, args.steps)
        info = md.pair_launch_info()["step"]
        cap = 1 << 18
        buf = np.zeros((cap, 8), np.uint32)
        n = lib.mdx_debug_drain_trace(md._h, 0, buf.ctypes.data_as(C.c_void_p), cap)
        if n <= 0:
            sys.exit(f"no trace came back ({n})")
        rec = buf[:n]
        print(f"# tools/pair_drain.py: {args.system}, {system.n_atoms} atoms frozen, last of {args.steps} inner-list walks; launch {info}")
        if args.raw:
            np.savez_compressed(args.raw, rec=rec)
        analyse(rec, args.bins)


if __name__ == "__main__":
    main()
