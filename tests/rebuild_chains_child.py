"""Child of tests/test_gpu_rebuild_chains.py: one process per (case, arm) - the library latches its knobs once per process.

usage: python tests/rebuild_chains_child.py <water|opc_kinds|solvated|lig50> <out.npz>

A frozen system (zero velocities, no stepping) is built twice per handle - at creation, which always takes the unfused chain, and by
rebuild_spatial_caches(), which takes the fused chain unless the arm or the system forbids it - once with the default (half-list) pair
kernel and once with the full-list kernel (nb_variant 2), whose forces are bitwise reproducible for a given slot order and list.  After
either build the child records forces, energies, the neighbour list and the statistics of the build; the parent compares them across the
two builds and across the arms."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402

STATS = ("n_tiles", "n_slots", "n_clusters", "n_cluster_pairs", "n_list_entries", "n_masked_entries", "rebuild_fallbacks")
ENERGIES = ("potential", "lj", "coulomb")
CUT = dict(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5)


def system_of(which):
    if which == "water":
        return systems.water_box(8), CUT
    if which == "opc_kinds":          # clusters by interaction kind: the order the unfused chain once did not apply
        assert os.environ.get("MDX_KIND_CLUSTERS") == "1", "the parent sets the knob"
        return systems.opc_water_box(8), CUT
    if which == "solvated":           # bonded roles, exclusions, masked entries
        return systems.small_solvated(), CUT
    if which == "lig50":              # vacuum: the grid follows the atoms, every build takes the unfused chain
        return systems.lig50(), dict(lj_cutoff=0.0, coulomb_cutoff=0.0)
    raise SystemExit(f"unknown case {which}")


def record(md, out, tag):
    out[tag + "_forces"] = md.forces()
    e = md.energy()
    out[tag + "_energy"] = np.array([e[k] for k in ENERGIES], np.float64)
    off, idx = md.neighbor_list()
    out[tag + "_nl_off"], out[tag + "_nl_idx"] = off, idx
    st = md.stats()
    out[tag + "_stats"] = np.array([int(st[k]) for k in STATS], np.int64)
    return st


def case(which, path):
    s, kw = system_of(which)
    s.vel = np.zeros_like(s.pos)
    out = {}
    for kernel, variant in (("half", 0), ("full", 2)):
        with md_state.MdState(s, MdConfig(nb_variant=variant, **kw)) as md:
            pos0 = md.positions()
            st1 = record(md, out, f"{kernel}_first")
            md.rebuild_spatial_caches()
            st2 = record(md, out, f"{kernel}_second")
            assert st2["rebuild_count"] > st1["rebuild_count"], (st1["rebuild_count"], st2["rebuild_count"])
            assert st2["rebuild_fallbacks"] == 0, st2["rebuild_fallbacks"]
            if which == "solvated":
                assert st2["n_masked_entries"] > 0, st2
            assert float(np.abs(md.positions() - pos0).max()) <= 1e-5      # frozen: every build sees the same positions
            print(f"{which} {kernel}: {s.n_atoms} atoms, " + ", ".join(f"{k} {st1[k]} -> {st2[k]}" for k in STATS))
    np.savez(path, **out)


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    case(sys.argv[1], sys.argv[2])
    print("REBUILD-CHAINS-OK")
