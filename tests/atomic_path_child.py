"""Child of tests/test_gpu_atomic_path.py: one process per case (the library reads its knobs once per process).

usage: python tests/atomic_path_child.py <tail0|tail4|wpt8|solvated> <out.npz>

Forces of the step loop's pair launch at FIXED positions (zero velocities, dt = 1e-9 ps), as tests/jtail_child.py takes them: the pruning
pass (the force call behind a rebuild, MDX_REBUILD_INNER=0) and the inner-list walk that follows it, and on the same positions the
forces of the deterministic full-list kernel (nb_variant 2): the yardstick.  Saved for the parent: prune, walk, full.

  tail0     water_box(16), 12,288 atoms, forced into the one-wave class and the order by length (MDX_WPT=1 MDX_TILE_LPT=2
            MDX_WPT8_BELOW=32), MDX_WPT_TAIL=0: every tile is one unit, which alone adds the tile's i-forces to its rows
  tail4     the same with MDX_WPT_TAIL=4/1: every tile is four units, each adds partial i-forces into rows three others add into
  wpt8      the same box, MDX_WPT=8 MDX_ONEPASS=0: a multi-wave class, the tile's first wave adds the fixed-order sum of the eight
            (the one-launch-per-step body, which this class would run by default, keeps the strided write-back and is not the subject)
  solvated  small_solvated(), MDX_WPT=1: several LJ types, exclusions: the masked chunk loop, entries that stay in place

Every case asserts from stats() that the pruning pass kept fewer cluster pairs than the Verlet list holds: entries were dropped (the
library reports cluster pairs, not entries; a tile's entry words are not reachable through the C ABI)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402

KNOBS = {
    "tail0": dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL="0"),
    "tail4": dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL="4/1"),
    "wpt8": dict(MDX_WPT="8", MDX_ONEPASS="0"),
    "solvated": dict(MDX_WPT="1"),
}


def case(which, path):
    knobs = dict(KNOBS[which], MDX_REBUILD_INNER="0")
    assert all(os.environ.get(k) == v for k, v in knobs.items()), "the parent sets the knobs"
    wpt = int(knobs["MDX_WPT"])
    if which == "solvated":
        s, kw = systems.small_solvated(), dict(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)
    else:
        s, kw = systems.water_box(n_side=16), {}
    s.vel = np.zeros_like(s.pos)
    out = {}
    with md_state.MdState(s, MdConfig(**kw)) as md:
        pos0 = md.positions()
        prunes = md.stats()["prune_passes"]
        for k in range(6):
            if k == 0 or k == 3:
                md.rebuild_spatial_caches()              # the force call behind a rebuild is the pruning pass (MDX_REBUILD_INNER=0)
            md.step(1e-9, None, 1)
            p = md.stats()["prune_passes"]
            kind = "prune" if p > prunes else "walk"
            prunes = p
            info = md.pair_launch_info()
            step = info["step"]
            assert (step["waves_per_tile"], step["half"], step["coulomb"], step["energy"]) == (wpt, 1, 0, 0) and step["dual"] != 0, info
            if kind not in out:
                out[kind] = md.forces()                  # what the step's pair launch left behind, not re-evaluated
        assert "prune" in out and "walk" in out, sorted(out)
        if which in ("tail0", "tail4"):
            tail = info["tail"]
            if which == "tail4":
                assert tail["waves_per_tile"] == 4 and tail["tiles"] == step["tiles"], info      # every tile is four units
            else:
                assert tail["waves_per_tile"] == 0 and tail["tiles"] == 0, info
        assert info["one_launch_steps"] == 0, info      # the bodies with the row-shaped write-back ran, not the one-launch-per-step one
        st = md.stats()
        assert 0 < st["n_inner_cluster_pairs"] < st["n_cluster_pairs"], (st["n_inner_cluster_pairs"], st["n_cluster_pairs"])
        if which == "solvated":
            assert st["n_masked_entries"] > 0, st        # the masked chunk loop runs
            assert not md.pair_body_info()["eligible"]   # the general body
        moved = float(np.abs(md.positions() - pos0).max())
        assert moved <= 1e-5, moved                      # frozen: every sample and the yardstick see the same positions
        tiles = step["tiles"]
    with md_state.MdState(s, MdConfig(nb_variant=2, **kw)) as md:
        out["full"] = md.forces()
        info = md.pair_launch_info()["any"]
        assert info["half"] == 0 and info["energy"] == 0, info
    np.savez(path, **out)
    full = out["full"].astype(np.float64)
    d = {k: float(np.abs(out[k].astype(np.float64) - full).max()) for k in ("prune", "walk")}
    pw = float(np.abs(out["prune"].astype(np.float64) - out["walk"].astype(np.float64)).max())
    print(f"{which}: {s.n_atoms} atoms, {tiles} tiles, cluster pairs {st['n_cluster_pairs']} -> inner {st['n_inner_cluster_pairs']}, "
          "max |F_half - F_full| " + ", ".join(f"{k} {v:.4e}" for k, v in d.items()) + f", max |F_prune - F_walk| {pw:.4e}")


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    case(sys.argv[1], sys.argv[2])
    print("ATOMIC-PATH-OK")
