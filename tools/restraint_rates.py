"""Steps/s with and without position restraints (mdx_set_position_restraints), arms interleaved in one process, measured like
bench.class_rate (relaxed 300 K start, fresh handle, untimed settle steps, NVE, no event brackets):
  dhfr23k      the chain's heavy atoms restrained (k 5 kcal/mol/A^2)
  complex50k   the solutes' heavy atoms restrained
  water64      64^3 flexible waters (786 k atoms, > 2048 tiles: the fused bonded + kick + drift pass), every 12th atom restrained
One JSON line per (system, arm, round):  python tools/restraint_rates.py [rounds=2]"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np


def _relaxed(s, dt):
    from molchanica_amd import MdConfig
    from molchanica_amd.md_state import MdState
    with MdState(s, MdConfig()) as eq:
        eq.minimize_energy(100); eq.initialize_velocities(300.0, True, seed=105)
        eq.set_thermostat(1, 300.0, 0.02, 1); eq.step(dt, None, 600); eq.set_thermostat(0, 300.0, 0.02, 1)
        s.pos, s.vel = np.ascontiguousarray(eq.positions(), np.float32), np.ascontiguousarray(eq.velocities(), np.float32)
    return s


def rate(s, idx, dt, n):
    import torch
    from molchanica_amd import MdConfig
    from molchanica_amd.md_state import MdState
    with MdState(s, MdConfig()) as md:
        if idx is not None:
            md.set_position_restraints(idx, None, 5.0)
        md.step(dt, None, 1000)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); md.step(dt, None, n); torch.cuda.synchronize(); el = time.perf_counter() - t0
        st = md.stats(); info = md.pair_launch_info()
    return {"steps_per_s": n / el, "ms_per_step": 1e3 * el / n, "rebuilds": int(st["rebuild_count"]), "n_tiles": int(st["n_tiles"]),
            "one_launch_steps": info["one_launch_steps"]}


def main():
    from molchanica_amd import systems
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    dt = 0.0005
    cases = []
    for name in ("dhfr23k", "complex50k"):
        s = _relaxed(systems.BY_NAME[name](), dt)
        n_sol = int(s.mol_start[2 if name == "complex50k" else 1])      # the chain (and the ligand) come before the water
        idx = np.nonzero(np.asarray(s.mass)[:n_sol] > 2.0)[0]
        cases.append((name, s, idx, 3000))
    w = _relaxed(systems.water_box(64), dt)
    cases.append(("water64", w, np.arange(0, w.n_atoms, 12), 500))
    for r in range(rounds):
        for name, s, idx, n in cases:
            for arm in ("plain", "restrained"):
                out = rate(s, idx if arm == "restrained" else None, dt, n)
                print(json.dumps(dict(system=name, arm=arm, round=r, n_atoms=s.n_atoms, n_restrained=int(len(idx)) if arm == "restrained" else 0, **out)), flush=True)


if __name__ == "__main__":
    main()
