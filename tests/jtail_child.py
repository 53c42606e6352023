"""Child of tests/test_gpu_jtail.py: one process per case (the library reads its knobs once per process).

usage: python tests/jtail_child.py <water1|water8|solvated|opc> <out.npz>

Forces of the half-list pair kernels at FIXED positions (zero velocities, dt = 1e-9 ps) - a plain force call (the plain list), a
pruning pass and an inner-list walk (what a step's pair launch left behind) - and, on the same positions, the forces of the
deterministic full-list kernel (nb_variant 2): the yardstick.  Saved for the parent: plain, prune, walk, full.

  water1    water_box(16), 12,288 atoms, MDX_WPT=1 MDX_REBUILD_INNER=0: the one-wave class, constant-sigma^2 body.  The ~50 A cell is four
            list radii wide: pairs of the Verlet list cross it in all 27 image directions (asserted here from the neighbour list)
  water8    the same box with MDX_WPT=8: a multi-wave class
  solvated  small_solvated(): several LJ types - the general body - and exclusions, so masked chunks
  opc       opc_water_box(12), coulomb_mode 2: Ewald real space from the force table"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402


def image_directions(md, s):
    """The image shifts k in {-1, 0, 1}^3 between the two atoms of the Verlet list's pairs, as codes (kx+1) + 3 (ky+1) + 9 (kz+1); a
    pair seen from its other end has the opposite shift, so both are counted."""
    off, idx = md.neighbor_list()
    pos = md.positions().astype(np.float64)
    L = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    i = np.repeat(np.arange(s.n_atoms), np.diff(off.astype(np.int64)))
    k = np.rint((pos[i] - pos[idx]) / L).astype(np.int64)
    assert np.abs(k).max() <= 1
    codes = set(np.unique((k[:, 0] + 1) + 3 * (k[:, 1] + 1) + 9 * (k[:, 2] + 1)).tolist())
    codes |= set(np.unique((1 - k[:, 0]) + 3 * (1 - k[:, 1]) + 9 * (1 - k[:, 2])).tolist())
    return codes


def case(which, path):
    wpt = {"water1": "1", "water8": "8", "solvated": "1", "opc": "1"}[which]
    assert os.environ.get("MDX_WPT") == wpt and os.environ.get("MDX_REBUILD_INNER") == "0", "the parent sets the knobs"
    if which in ("water1", "water8"):
        s, kw, coul, uni = systems.water_box(n_side=16), {}, 0, True
    elif which == "solvated":
        s, kw, coul, uni = systems.small_solvated(), dict(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5), 0, False
    else:
        s, kw, coul, uni = systems.opc_water_box(n_side=12), dict(coulomb_mode=2, ewald_alpha=0.3), 4, True
    s.vel = np.zeros_like(s.pos)
    out = {}
    with md_state.MdState(s, MdConfig(**kw)) as md:
        pos0 = md.positions()
        out["plain"] = md.forces()
        info = md.pair_launch_info()["any"]
        assert (info["waves_per_tile"], info["dual"], info["half"], info["coulomb"]) == (int(wpt), 0, 1, coul), info
        if which == "water1":
            assert md.pair_body_info()["any"] == uni
            codes = image_directions(md, s)
            assert codes == set(range(27)), sorted(set(range(27)) - codes)
        if which == "solvated":
            assert not md.pair_body_info()["eligible"]
        prunes = md.stats()["prune_passes"]
        for k in range(6):
            if k == 0 or k == 3:
                md.rebuild_spatial_caches()              # the force call behind a rebuild is the pruning pass (MDX_REBUILD_INNER=0)
            md.step(1e-9, None, 1)
            p = md.stats()["prune_passes"]
            kind = "prune" if p > prunes else "walk"
            prunes = p
            info = md.pair_launch_info()["step"]
            assert (info["waves_per_tile"], info["half"], info["coulomb"], info["energy"]) == (int(wpt), 1, coul, 0) and info["dual"] != 0, info
            if kind not in out:
                out[kind] = md.forces()                  # what the step's pair launch left behind, not re-evaluated
        assert "prune" in out and "walk" in out, sorted(out)
        moved = float(np.abs(md.positions() - pos0).max())
        assert moved <= 1e-5, moved                      # frozen: every sample and the yardstick see the same positions
        tiles = info["tiles"]
    with md_state.MdState(s, MdConfig(nb_variant=2, **kw)) as md:
        out["full"] = md.forces()
        info = md.pair_launch_info()["any"]
        assert info["half"] == 0 and info["energy"] == 0, info
    np.savez(path, **out)
    d = {k: float(np.abs(out[k].astype(np.float64) - out["full"].astype(np.float64)).max()) for k in ("plain", "prune", "walk")}
    print(f"{which}: {s.n_atoms} atoms, {tiles} tiles, max |F_half - F_full| " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    case(sys.argv[1], sys.argv[2])
    print("JTAIL-OK")
