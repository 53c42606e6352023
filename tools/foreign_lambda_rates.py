"""Cost of the foreign-lambda energies (mdx_set_foreign_lambdas) on small_solvated, the reference's hydration-window setup:
  window      steps/s of a TI window (lambda 0.5, SPME, CSVR, snapshot every 10 steps) without and with the 13 foreign lambdas of
              the reference's grid, arms interleaved in one process (fresh handle, untimed settle steps)
  pass        wall time of one mdx_foreign_energies call at K = 13 (cutoff Coulomb: the pair pass, its sum and the read-back only)
One JSON line per measurement:  python tools/foreign_lambda_rates.py [rounds=3] [pass]   ("pass": the pass timing only)
(Run under `rocprofv3 --kernel-trace --stats` for the device time of nb_foreign_kernel itself.)"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())

GRID = [0.0, 0.05, 0.10, 0.20, 0.30, 0.40, 0.50, 0.60, 0.70, 0.80, 0.90, 0.95, 1.0]


def window_rate(s, cfg, foreign, n):
    import torch
    from molchanica_amd.md_state import MdState
    with MdState(s, cfg) as md:
        md.configure_alchemical_window(0, 0.5)
        if foreign:
            md.set_foreign_lambdas(GRID)
        md.set_thermostat(2, 300.0, 0.1, 10, seed=3)
        md.set_snapshot_cadence(10)
        md.step(0.002, None, 500)
        md.flush_snapshot_queues()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); md.step(0.002, None, n); torch.cuda.synchronize(); el = time.perf_counter() - t0
        snaps = len(md.snapshots)
        st = md.stats()
    return {"steps_per_s": n / el, "ms_per_step": 1e3 * el / n, "snapshots": snaps, "energy_evaluations": int(st["energy_evaluations"])}


def pass_time(s, cfg, calls):
    from molchanica_amd.md_state import MdState
    with MdState(s, cfg) as md:
        md.configure_alchemical_window(0, 0.5)
        md.set_foreign_lambdas(GRID)
        for _ in range(20):
            md.foreign_energies()
        t0 = time.perf_counter()
        for _ in range(calls):
            md.foreign_energies()
        el = time.perf_counter() - t0
    return {"us_per_call": 1e6 * el / calls, "calls": calls}


def main():
    from molchanica_amd import MdConfig, systems, _abi
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    s = systems.small_solvated()
    spme = MdConfig(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=_abi.COULOMB_EWALD, ewald_alpha=0.4, overrides=0)
    rf = MdConfig(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, coulomb_mode=_abi.COULOMB_REACTION)
    only_pass = len(sys.argv) > 2 and sys.argv[2] == "pass"
    for r in range(rounds):
        for arm in () if only_pass else ("window", "window+foreign13"):
            out = window_rate(s, spme, arm != "window", 4000)
            print(json.dumps(dict(kind="window", system="small_solvated", n_atoms=s.n_atoms, arm=arm, round=r, **out)), flush=True)
        print(json.dumps(dict(kind="pass", system="small_solvated", n_atoms=s.n_atoms, K=13, round=r, **pass_time(s, rf, 500))), flush=True)


if __name__ == "__main__":
    main()
