"""The neighbour list is rebuilt through two chains (mdx_grid.hip): the unfused one - a handle's first build, vacuum systems, every
fallback, MDX_REBUILD_FUSED=0 - and the fused one (rebuild_fast, one host wait).  Slot assignment and the list are functions of the
positions, not of the chain that ran: this test holds the chains against each other.

Arms, a fresh child process each (tests/rebuild_chains_child.py; the library latches its knobs once per process):
  default              creation builds unfused + count/fill, rebuild_spatial_caches() takes the fused chain (lig50: unfused, single pass)
  MDX_REBUILD_FUSED=0  the second build takes the unfused chain with the single-pass list build
  MDX_LIST_TWO_PASS=1  both builds unfused, count + scan + fill
Cases: water_box(8); opc_water_box(8) with clusters by interaction kind; small_solvated() (roles, exclusions, masked entries); lig50()
(vacuum: always the unfused chain).  All frozen: zero velocities, no stepping.

Across the two builds of a handle and the three arms (six builds per pair kernel):
  - the neighbour list (offsets and indices), n_tiles, n_slots, n_clusters and n_cluster_pairs are identical;
  - the forces of the full-list kernel (nb_variant 2) are identical bit patterns;
  - the half-list forces pass _force_err < 1.0 (tests/test_gpu_dual_list.py) against the default arm's first build;
  - energies agree to rel 1e-5, abs 1e-3 (tests/test_gpu_constraints.py between list arms).
  - n_list_entries and n_masked_entries are identical as well: count + fill and the single pass pad every tile's run to the same whole
    chunks.  (Measured on the build before the chains shared their stages - DESIGN.md, "one copy of each rebuild stage": no quantity
    differed between the chains there, so nothing is compared more loosely than listed here.)
What the test cannot show: that the default arm's second build went through rebuild_fast.  stats() has no count per chain; the child
asserts that rebuild_count rose and rebuild_fallbacks stayed 0, and a library that sent every rebuild down the unfused chain would still
pass here."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "rebuild_chains_child.py")

ARMS = {"default": {}, "unfused": dict(MDX_REBUILD_FUSED="0"), "two_pass": dict(MDX_LIST_TWO_PASS="1")}
CASE_KNOBS = {"water": {}, "opc_kinds": dict(MDX_KIND_CLUSTERS="1"), "solvated": {}, "lig50": {}}
STATS = ("n_tiles", "n_slots", "n_clusters", "n_cluster_pairs", "n_list_entries", "n_masked_entries", "rebuild_fallbacks")
SAME = ("n_tiles", "n_slots", "n_clusters", "n_cluster_pairs", "n_list_entries", "n_masked_entries")
ENERGIES = ("potential", "lj", "coulomb")


def _force_err(f_a, f_b):      # tests/test_gpu_dual_list.py
    d = np.linalg.norm(f_a - f_b, axis=1)
    scale = np.maximum(np.linalg.norm(f_b, axis=1), 1.0)
    rmsf = math.sqrt((f_b ** 2).sum(1).mean())
    return float((d / (1e-4 * scale + 1e-5 * rmsf)).max())


def run_child(which, arm, path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_") or k == "MDX_LIB"}      # (MDX_LIB: which build, not a knob)
    env.update(CASE_KNOBS[which], **ARMS[arm])
    p = subprocess.run([sys.executable, CHILD, which, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "REBUILD-CHAINS-OK" in p.stdout, tail
    print(f"[{arm}]\n{tail}")
    return np.load(path)


@pytest.mark.parametrize("which", ["water", "opc_kinds", "solvated", "lig50"])
def test_chains_build_the_same_list(tmp_path, which):
    runs = {arm: run_child(which, arm, str(tmp_path / f"{which}_{arm}.npz")) for arm in ARMS}
    builds = [(arm, b) for arm in ARMS for b in ("first", "second")]
    bad = []
    for kernel in ("half", "full"):
        get = lambda arm, b, what: runs[arm][f"{kernel}_{b}_{what}"]      # noqa: E731
        ref = {what: get("default", "first", what) for what in ("forces", "energy", "nl_off", "nl_idx", "stats")}
        f_ref = ref["forces"].astype(np.float64)
        assert np.isfinite(f_ref).all() and float(np.abs(f_ref).max()) > 1.0
        assert ref["nl_idx"].size > 0 and ref["stats"][STATS.index("n_cluster_pairs")] > 0
        for arm, b in builds:
            tag = f"{which} {kernel} {arm}/{b}"
            st = dict(zip(STATS, get(arm, b, "stats").tolist()))
            st_ref = dict(zip(STATS, ref["stats"].tolist()))
            f = get(arm, b, "forces")
            bits = bool(np.array_equal(f.view(np.uint32), ref["forces"].view(np.uint32)))
            err = _force_err(f.astype(np.float64), f_ref)
            nl = bool(np.array_equal(get(arm, b, "nl_off"), ref["nl_off"]) and np.array_equal(get(arm, b, "nl_idx"), ref["nl_idx"]))
            print(f"{tag}: list identical {nl}, forces bitwise {bits}, force err {err:.3e}, "
                  + ", ".join(f"{k} {st[k]}" for k in STATS) + ", energies " + " ".join(f"{v:.6f}" for v in get(arm, b, "energy")))
            if not nl: bad.append((tag, "neighbour list"))
            for k in SAME:
                if st[k] != st_ref[k]: bad.append((tag, k, st[k], st_ref[k]))
            if st["rebuild_fallbacks"] != 0: bad.append((tag, "rebuild_fallbacks", st["rebuild_fallbacks"]))
            if kernel == "full" and not bits: bad.append((tag, "full-list forces differ as bit patterns", err))
            if not err < 1.0: bad.append((tag, "force err", err))
            for k, v, v_ref in zip(ENERGIES, get(arm, b, "energy"), ref["energy"]):
                if v != pytest.approx(v_ref, rel=1e-5, abs=1e-3): bad.append((tag, k, v, v_ref))
    assert not bad, bad
