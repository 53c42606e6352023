"""Child of tests/test_gpu_walk_chunks.py: one process per case (the library reads its knobs once per process).

usage: python tests/walk_chunks_child.py <water1|tail4|water8|solvated1|solvated8|opc> <out.npz>

As tests/jtail_child.py: forces of the half-list pair kernels at FIXED positions (zero velocities, dt = 1e-9 ps) - a plain force call (the
plain list), a pruning pass and an inner-list walk (what a step's pair launch left behind) - and, on the same positions, the forces of the
deterministic full-list kernel (nb_variant 2): the yardstick.  Saved for the parent: plain, prune, walk, full, and `two_sets` - whether
each of the three launches ran the chunk loop with two sets of pipeline registers (mdx_pair_body_info).

  water1     water_box(16), 12,288 atoms, MDX_WPT=1: the one-wave class, constant-sigma^2 body - the two-set loop.  About 25 chunks per
             tile, shares of either parity; the ~50 A cell is four list radii wide, so the Verlet list's pairs cross it in all 27 image
             directions (asserted here from the neighbour list): every image code a list can name is decoded
  tail4      the same with MDX_WPT_TAIL=4/1: every tile is four units, chunk stride 4
  water8     the same box with MDX_WPT=8: three or four chunks per wave, the one-set loop of a multi-wave class
  solvated1  small_solvated(), MDX_WPT=1: several LJ types - the general body - and exclusions, so masked chunks
  solvated8  small_solvated(), MDX_WPT=8: 22 tiles, waves with no chunk and with one, the masked run ending at odd positions
  opc        opc_water_box(12), coulomb_mode 2: the Ewald force table sharing LDS with the strips"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402
from jtail_child import image_directions  # noqa: E402

KNOBS = {
    "water1": dict(MDX_WPT="1"),
    "tail4": dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL="4/1"),
    "water8": dict(MDX_WPT="8"),
    "solvated1": dict(MDX_WPT="1"),
    "solvated8": dict(MDX_WPT="8"),
    "opc": dict(MDX_WPT="1"),
}


def case(which, path):
    knobs = dict(KNOBS[which], MDX_REBUILD_INNER="0")
    assert all(os.environ.get(k) == v for k, v in knobs.items()), "the parent sets the knobs"
    wpt = int(knobs["MDX_WPT"])
    if which in ("water1", "tail4", "water8"):
        s, kw, coul, uni = systems.water_box(n_side=16), {}, 0, True
    elif which in ("solvated1", "solvated8"):
        s, kw, coul, uni = systems.small_solvated(), dict(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5), 0, False
    else:
        s, kw, coul, uni = systems.opc_water_box(n_side=12), dict(coulomb_mode=2, ewald_alpha=0.3), 4, True
    s.vel = np.zeros_like(s.pos)
    out = {}
    with md_state.MdState(s, MdConfig(**kw)) as md:
        pos0 = md.positions()
        out["plain"] = md.forces()
        info = md.pair_launch_info()["any"]
        assert (info["waves_per_tile"], info["dual"], info["half"], info["coulomb"]) == (wpt, 0, 1, coul), info
        body = md.pair_body_info()
        assert body["eligible"] == uni, body
        two = {"plain": bool(body.get("any_two_sets", False))}
        # the two-set loop belongs to the one-wave kernels with the constant-sigma^2 body and to nothing else
        assert not two["plain"] or (wpt == 1 and body["any"]), (body, info)
        if which == "water1":
            assert body["any"]
            codes = image_directions(md, s)
            assert codes == set(range(27)), sorted(set(range(27)) - codes)
        prunes = md.stats()["prune_passes"]
        for k in range(6):
            if k == 0 or k == 3:
                md.rebuild_spatial_caches()              # the force call behind a rebuild is the pruning pass (MDX_REBUILD_INNER=0)
            md.step(1e-9, None, 1)
            p = md.stats()["prune_passes"]
            kind = "prune" if p > prunes else "walk"
            prunes = p
            linfo = md.pair_launch_info()
            info = linfo["step"]
            assert (info["waves_per_tile"], info["half"], info["coulomb"], info["energy"]) == (wpt, 1, coul, 0) and info["dual"] != 0, info
            if kind not in out:
                out[kind] = md.forces()                  # what the step's pair launch left behind, not re-evaluated
                body = md.pair_body_info()
                two[kind] = bool(body.get("step_two_sets", False))
                assert not two[kind] or (wpt == 1 and body["step"]), (body, info)
        assert "prune" in out and "walk" in out, sorted(out)
        if which == "tail4":
            assert linfo["tail"]["waves_per_tile"] == 4 and linfo["tail"]["tiles"] == info["tiles"], linfo      # every tile is four units
        st = md.stats()
        if which in ("solvated1", "solvated8"):
            assert st["n_masked_entries"] > 0, st        # the masked chunk loop runs
        moved = float(np.abs(md.positions() - pos0).max())
        assert moved <= 1e-5, moved                      # frozen: every sample and the yardstick see the same positions
        tiles = info["tiles"]
    with md_state.MdState(s, MdConfig(nb_variant=2, **kw)) as md:
        out["full"] = md.forces()
        info = md.pair_launch_info()["any"]
        assert info["half"] == 0 and info["energy"] == 0, info
    out["two_sets"] = np.array([two["plain"], two["prune"], two["walk"]])      # (in the order plain, prune, walk)
    np.savez(path, **out)
    d = {k: float(np.abs(out[k].astype(np.float64) - out["full"].astype(np.float64)).max()) for k in ("plain", "prune", "walk")}
    print(f"{which}: {s.n_atoms} atoms, {tiles} tiles, chunk loop with two sets: {two}, max |F_half - F_full| "
          + ", ".join(f"{k} {v:.4e}" for k, v in d.items()))


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    case(sys.argv[1], sys.argv[2])
    print("WALK-CHUNKS-OK")
