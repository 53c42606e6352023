"""Child of tests/test_gpu_prune_hitbits.py: one process per (case, arm) - the library reads its knobs once per process.

usage: python tests/prune_hitbits_child.py <water|tail4|inner0|solvated|short|opc> <out.npz>

Two handles per case, one rebuild_spatial_caches() each - the fused chain, whose one-wave pruning pass (prune_list_kernel, forced on these
small boxes by MDX_PRUNE_MW_BELOW=0) is what the arms differ in - and the read-out of the lists as the device holds them
(MdState.debug_pair_lists) BEFORE any force call touches them:
  full   nb_variant 2, the deterministic full-list kernel: no dual list, so the pass runs without the inner list; its forces are bitwise
         reproducible for a given slot order and list
  half   the default half-list kernel: on a flexible system the pass also writes the inner list of the dual pair list
`water` does it twice: at the lattice start, and at the positions 20 steps later.  The 20 steps are taken by the FULL handle - the half-list
kernel adds its j-forces with atomics, so two processes would not arrive at the same positions bit for bit - and handed to the half handle."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402

INNER_SKIN = 0.5
SHORT = dict(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)      # the boxes of 26 A and less
STATS = ("n_tiles", "n_cluster_pairs", "n_inner_cluster_pairs", "rebuild_fallbacks")


def system_of(which):
    """-> system, cutoffs, whether the half handle's rebuild writes the inner list"""
    if which in ("water", "tail4"):
        return systems.water_box(16, seed=41), {}, True
    if which == "inner0":
        assert os.environ.get("MDX_REBUILD_INNER") == "0", "the parent sets the knob"
        return systems.water_box(16, seed=41), {}, False
    if which == "solvated":
        return systems.small_solvated(), SHORT, True
    if which == "short":             # (the dual list wants its inner skin of 0.5 A below the skin)
        return systems.water_box(16, seed=41), dict(lj_cutoff=3.0, coulomb_cutoff=3.0, skin=1.0), True
    if which == "opc":               # rigid four-site water, clusters by interaction kind: the kind filter, no inner list from the rebuild
        assert os.environ.get("MDX_KIND_CLUSTERS") == "1", "the parent sets the knob"
        return systems.opc_water_box(8), SHORT, False
    raise SystemExit(f"unknown case {which}")


def rebuild_and_record(md, out, tag, forces=False):
    before = md.stats()["rebuild_count"]
    md.rebuild_spatial_caches()
    for k, v in md.debug_pair_lists().items():
        out[f"{tag}_{k}"] = v
    st = md.stats()
    assert st["rebuild_count"] > before and st["rebuild_fallbacks"] == 0, (before, st["rebuild_count"], st["rebuild_fallbacks"])
    out[tag + "_stats"] = np.array([int(st[k]) for k in STATS], np.int64)
    out[tag + "_wrote_inner"] = np.array(bool(md.pair_launch_info()["last_rebuild_wrote_the_inner_list"]))
    out[tag + "_nl_off"], out[tag + "_nl_idx"] = md.neighbor_list()
    out[tag + "_pos"] = md.positions()
    if forces:
        out[tag + "_forces"] = md.forces()
    print(f"{tag}: " + ", ".join(f"{k} {st[k]}" for k in STATS) + f", inner list from the rebuild: {bool(out[tag + '_wrote_inner'])}")


def case(which, path):
    assert os.environ.get("MDX_PRUNE_MW_BELOW") == "0" and os.environ.get("MDX_WPT") == "1", "the parent sets the knobs"
    s, cut, inner = system_of(which)
    out = {}
    moved = None
    with md_state.MdState(s, MdConfig(nb_variant=2, inner_skin=INNER_SKIN, **cut)) as md:
        rebuild_and_record(md, out, "full_start", forces=True)
        assert not out["full_start_wrote_inner"]
        if which == "water":
            md.step(0.0005, None, 20)
            moved = md.positions()
            rebuild_and_record(md, out, "full_moved", forces=True)
    with md_state.MdState(s, MdConfig(inner_skin=INNER_SKIN, **cut)) as md:
        rebuild_and_record(md, out, "half_start")
        assert bool(out["half_start_wrote_inner"]) == inner, "which flavour of the pass ran"
        if moved is not None:
            md.set_positions(moved)
            rebuild_and_record(md, out, "half_moved")
            assert bool(out["half_moved_wrote_inner"]) == inner, "which flavour of the pass ran"
    np.savez(path, **out)


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    case(sys.argv[1], sys.argv[2])
    print("PRUNE-HITBITS-OK")
