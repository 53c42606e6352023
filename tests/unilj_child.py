"""Child of tests/test_gpu_unilj.py: one process per MDX_UNI_LJ value (the library reads its knobs once per process).

usage: python tests/unilj_child.py bits <water|solvated> <out.npz> | timed <water|opc> <out.npz> | refusals
  bits      nb_variant 2, the deterministic full-list cluster kernel: steps across a list rebuild; positions, velocities, forces and what
            mdx_pair_body_info says, saved for the parent to compare bit for bit between MDX_UNI_LJ=0 and the default;
  timed     the bodies the bench line times (MDX_WPT=1: the one-wave class, merged dual-list launch) at fixed positions: forces of a plain
            force call, of a pruning pass and of an inner-list walk (atoms frozen: dt = 1e-9 ps, zero velocities), saved;
  refusals  the handles that must not, and those that must, be eligible (default environment)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402

OFF = os.environ.get("MDX_UNI_LJ") == "0"


def f32_pair_constant(sigma):
    h = np.float32(0.5) * np.float32(sigma)
    s = np.float32(h + h)
    return np.float32(s * s)


def bits(which, path):
    if which == "water":
        s, cfg, steps = systems.water_box(n_side=16), MdConfig(nb_variant=2), 20
    else:
        s, cfg, steps = systems.small_solvated(), MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2), 10
    with md_state.MdState(s, cfg) as md:
        b0 = md.pair_body_info()
        md.step(0.0005, None, steps // 2)
        if which == "water":
            md.rebuild_spatial_caches()      # at least one rebuild inside the run, whatever the skin allows
        md.step(0.0005, None, steps - steps // 2)
        b1, st, info = md.pair_body_info(), md.stats(), md.pair_launch_info()
        assert st["rebuild_count"] >= (2 if which == "water" else 1), st["rebuild_count"]
        assert info["any"]["half"] == 0 and info["any"]["energy"] == 0 and info["any"]["waves_per_tile"] in (4, 8), info
        np.savez(path, pos=md.positions(), vel=md.velocities(), force=md.forces(),
                 body=np.array([b0["eligible"], b1["eligible"], b1["step"], b1["any"], b1["c_bits"]], np.uint32))
        print(f"{which}: body {b1}, launch {info['any']}, rebuilds {st['rebuild_count']}")


def timed(which, path):
    assert os.environ.get("MDX_WPT") == "1" and os.environ.get("MDX_REBUILD_INNER") == "0"
    if which == "water":
        s, cfg, coul = systems.water_box(n_side=16), MdConfig(), 0
    else:
        s, cfg, coul = systems.opc_water_box(n_side=12), MdConfig(coulomb_mode=2, ewald_alpha=0.3), 4
    s.vel = np.zeros_like(s.pos)
    out = {}
    with md_state.MdState(s, cfg) as md:
        out["plain"] = md.forces()                       # (a) a plain force call: the plain list
        info, body = md.pair_launch_info(), md.pair_body_info()
        assert (info["any"]["waves_per_tile"], info["any"]["dual"], info["any"]["half"], info["any"]["coulomb"]) == (1, 0, 1, coul), info
        assert body["any"] == (not OFF), body
        used = {"plain": body["any"]}
        prunes = md.stats()["prune_passes"]
        for k in range(6):                               # (b), (c): single steps; a step's force call is a pruning pass or an inner-list walk
            if k == 0 or k == 3:
                md.rebuild_spatial_caches()              # the force call behind a rebuild is the pruning pass (MDX_REBUILD_INNER=0)
            md.step(1e-9, None, 1)
            p = md.stats()["prune_passes"]
            kind = "prune" if p > prunes else "walk"
            prunes = p
            info, body = md.pair_launch_info(), md.pair_body_info()
            assert (info["step"]["waves_per_tile"], info["step"]["dual"], info["step"]["half"], info["step"]["coulomb"], info["step"]["energy"]) == (1, 3, 1, coul, 0), info
            assert body["step"] == (not OFF), (kind, body)
            if kind not in out:
                out[kind] = md.forces()                  # what the step's pair launch left behind, not re-evaluated
                used[kind] = body["step"]
        assert "prune" in out and "walk" in out, sorted(out)      # both bodies of the merged launch ran
        body = md.pair_body_info()
        assert body["eligible"] == (not OFF), body
        if not OFF:
            assert body["c_bits"] == int(f32_pair_constant(s.lj_sigma[0]).view(np.uint32)), body
        np.savez(path, **out)
        print(f"{which}: {s.n_atoms} atoms, {info['step']['tiles']} tiles, body {body}, used {used}, pruning passes {prunes}")


def refusals():
    t = systems.TIP3P
    # (648-atom boxes: of the kernels such a box launches, the full-list ones of nb_variant 2 have the constant-sigma^2 body)
    cfgw = dict(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0, nb_variant=2)
    # several LJ types
    with md_state.MdState(systems.small_solvated(), MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)) as md:
        md.forces(); md.step(0.0005, None, 3)
        b = md.pair_body_info()
        assert not b["eligible"] and not b["step"] and not b["any"] and b["c_bits"] == 0, b
    # a second oxygen type, sigma one ulp up, on ONE molecule
    s = systems.water_box(n_side=6)
    s.lj_sigma = np.array([t["o_sigma"], 0.0, np.nextafter(np.float32(t["o_sigma"]), np.float32(10.0))], np.float32)
    s.lj_eps = np.array([t["o_eps"], 0.0, t["o_eps"]], np.float32)
    s.lj_type = s.lj_type.copy(); s.lj_type[3 * 100] = 2
    assert s.lj_sigma[2] != s.lj_sigma[0] and np.float32(0.5) * s.lj_sigma[2] != np.float32(0.5) * s.lj_sigma[0]
    with md_state.MdState(s, MdConfig(**cfgw)) as md:
        md.forces(); md.step(0.0005, None, 3)
        b = md.pair_body_info()
        assert not b["eligible"] and not b["step"] and not b["any"], b
    # hydrogens with a sigma of their own and no well: eligible, and the body goes out
    s = systems.water_box(n_side=6)
    s.lj_sigma = np.array([t["o_sigma"], 1.0], np.float32)
    with md_state.MdState(s, MdConfig(**cfgw)) as md:
        md.forces(); md.step(0.0005, None, 3)
        b = md.pair_body_info()
        assert b["eligible"] and b["step"] and b["any"], b
        assert b["c_bits"] == int(f32_pair_constant(t["o_sigma"]).view(np.uint32)), b
    # the geometric rule: never
    with md_state.MdState(systems.water_box(n_side=6), MdConfig(combining_rule=1, **cfgw)) as md:
        md.forces()
        b = md.pair_body_info()
        assert not b["eligible"] and not b["any"], b
    # an alchemical window on a water box: off while the window is on, back when it is switched off
    with md_state.MdState(systems.water_box(n_side=6), MdConfig(**cfgw)) as md:
        md.forces()
        assert md.pair_body_info()["eligible"] and md.pair_body_info()["any"]
        md.configure_alchemical_window(5, 0.5)
        md.forces(); md.step(0.0005, None, 3)
        b = md.pair_body_info()
        assert not b["eligible"] and not b["step"] and not b["any"] and b["c_bits"] == 0, b
        md.configure_alchemical_window(5, -1.0)
        md.forces(); md.step(0.0005, None, 3)
        b = md.pair_body_info()
        assert b["eligible"] and b["step"] and b["any"], b
    print("refusals: several types, one ulp, geometric, alchemical refused; well-free sigmas accepted")


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    mode = sys.argv[1]
    if mode == "bits":
        bits(sys.argv[2], sys.argv[3])
    elif mode == "timed":
        timed(sys.argv[2], sys.argv[3])
    else:
        refusals()
    print("UNILJ-OK")
