"""The one-wave exact pruning pass of the list rebuild (prune_list_kernel / prune_list_hb_kernel, mdx_grid.hip) keeps each lane's answers in
vector registers and combines the 64 lanes once per two entries (the default), where it took a ballot per cluster pair
(MDX_PRUNE_HITBITS=0).  The kept set is "any lane: d2 < r2" per cluster pair either way, so the lists must come out bit for bit the same.

Arms, a fresh child process each (tests/prune_hitbits_child.py; the knobs are read once per process): `ballots` MDX_PRUNE_HITBITS=0,
`hitbits` the default, and on `water` `tries0` / `tries3`, the hit-bit pass with no and with three quick-accept tries per cluster pair
in either flavour.  Every arm runs with MDX_PRUNE_MW_BELOW=0 (the one-wave pass on boxes this small) and MDX_WPT=1 (the one-wave class of
the pair kernel, which the inner list out of the rebuild is written for).  Cases:
  water     water_box(16), 12,288 atoms, periodic (image codes occur): the pass that also writes the inner list, at the lattice start and
            at the positions 20 steps later
  tail4     the same box with MDX_WPT_TAIL=4/1 MDX_TILE_LPT=2 MDX_WPT8_BELOW=32: tail units share a tile's plain run
  inner0    the same box with MDX_REBUILD_INNER=0: the pass without the inner list on the half-list handle as well
  solvated  small_solvated(): several atom kinds, exclusions - masked chunks, whose entries stay in place
  short     water_box(16) with rc 3 + skin 1: lists of two or three chunks, the masked run among them
  opc       opc_water_box(8) with MDX_KIND_CLUSTERS=1: the kind filter
Compared bit for bit against `ballots`, per handle (full-list kernel without the inner list, half-list kernel) and rebuild: the per-tile
counts; the entries over every tile's run, padding included; the inner list's entries over the masked run and up to each tile's
inner_nch bound; all eight inner_nch words per tile; n_cluster_pairs and n_inner_cluster_pairs; neighbor_list(); the forces of the
full-list kernel as uint32.  (Entry offsets are not compared: the single-pass build hands out a tile's place in the array by an atomic
cursor.)

Independent of the other arm, on `water` in fp64 with the minimum image (the cell is four list radii wide): every atom pair within
cutoff + skin - 1e-3 A is in neighbor_list() (at the positions 20 steps off the lattice); every kept cluster pair has an atom pair
within cutoff + skin + 1e-3 A, every cluster pair of the inner list one within cutoff + inner_skin + 1e-3 A.  The margin: the device
tests fp32 distances of fp32 coordinates of up to 50 A, image shift applied - a few ulp of 3e-6 A each in dx, dy, dz, and a relative
2e-7 of d2 = 144 A^2 is 1e-6 A in d; the list radius of the build is r (1 + 1e-5) + 1e-4 = 12.00022 A.  All far inside the margin."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "prune_hitbits_child.py")

COMMON = dict(MDX_PRUNE_MW_BELOW="0", MDX_WPT="1")
ARMS = {"ballots": dict(MDX_PRUNE_HITBITS="0"), "hitbits": {},
        "tries0": dict(MDX_PRUNE_TRIES="0", MDX_PRUNE_TRIES_INNER="0"), "tries3": dict(MDX_PRUNE_TRIES="3", MDX_PRUNE_TRIES_INNER="3")}
CASES = {
    "water": (dict(), ("ballots", "hitbits", "tries0", "tries3")),
    "tail4": (dict(MDX_WPT_TAIL="4/1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32"), ("ballots", "hitbits")),
    "inner0": (dict(MDX_REBUILD_INNER="0"), ("ballots", "hitbits")),
    "solvated": (dict(), ("ballots", "hitbits")),
    "short": (dict(), ("ballots", "hitbits")),
    "opc": (dict(MDX_KIND_CLUSTERS="1"), ("ballots", "hitbits")),
}
STATS = ("n_tiles", "n_cluster_pairs", "n_inner_cluster_pairs", "rebuild_fallbacks")
CUTOFF, SKIN, INNER_SKIN, MARGIN = 10.0, 2.0, 0.5, 1e-3      # MdConfig() defaults, the child's inner skin


def run_child(which, arm, path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_") or k == "MDX_LIB"}      # (MDX_LIB: which build, not a knob)
    env.update(COMMON, **CASES[which][0], **ARMS[arm])
    p = subprocess.run([sys.executable, CHILD, which, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "PRUNE-HITBITS-OK" in p.stdout, tail
    print(f"[{which} / {arm}]\n{tail}")
    return dict(np.load(path))


def tile_runs(run, tag):
    """-> per tile: the entries of its run as pruned (padding included); the inner list's entries up to the tile's loop bound, or None"""
    counts, off, ent, ent_in, nch = (run[f"{tag}_{k}"] for k in ("counts", "entry_off", "entries", "entries_in", "inner_nch"))
    inner = bool(run[f"{tag}_wrote_inner"])
    lists, inners = [], []
    for t in range(counts.shape[0]):
        e0, nm, npl = int(off[t]), int(counts[t, 0]), int(counts[t, 1])
        assert nm % 8 == 0 and npl % 8 == 0
        lists.append(ent[e0:e0 + nm + npl])
        if inner:
            assert (nch[t] == nch[t, 0]).all() and nm // 8 <= int(nch[t, 0]) <= (nm + npl) // 8, (t, nch[t], nm, npl)
            inners.append(ent_in[e0:e0 + int(nch[t, 0]) * 8])
    return lists, (inners if inner else None)


def compare(which, arm, ref, run):
    bad = []
    tags = sorted(k[:-len("_counts")] for k in ref if k.endswith("_counts"))
    assert tags and tags == sorted(k[:-len("_counts")] for k in run if k.endswith("_counts"))
    for tag in tags:
        name = f"{which} {arm} {tag}"
        same = lambda k: np.array_equal(ref[f"{tag}_{k}"], run[f"{tag}_{k}"])      # noqa: E731
        if not same("pos"): bad.append((name, "the two arms rebuilt at different positions"))
        if bool(ref[f"{tag}_wrote_inner"]) != bool(run[f"{tag}_wrote_inner"]): bad.append((name, "inner list from the rebuild in one arm only"))
        for k in ("counts", "orig_of", "nl_off", "nl_idx", "inner_nch"):
            if not same(k): bad.append((name, k))
        for k, a, b in zip(STATS, ref[f"{tag}_stats"].tolist(), run[f"{tag}_stats"].tolist()):
            if a != b: bad.append((name, k, a, b))
        if bad:
            continue
        (l_ref, in_ref), (l_run, in_run) = tile_runs(ref, tag), tile_runs(run, tag)
        n_diff = sum(not np.array_equal(a, b) for a, b in zip(l_ref, l_run))
        if n_diff: bad.append((name, "entries differ in tiles", n_diff))
        n_in = 0
        if in_ref is not None:
            n_in = sum(len(a) for a in in_ref)
            n_diff = sum(not np.array_equal(a, b) for a, b in zip(in_ref, in_run))
            if n_diff: bad.append((name, "inner entries differ in tiles", n_diff))
        bits = None
        if f"{tag}_forces" in ref:
            f = ref[f"{tag}_forces"]
            assert np.isfinite(f).all() and float(np.abs(f).max()) > 1.0
            bits = bool(np.array_equal(f.view(np.uint32), run[f"{tag}_forces"].view(np.uint32)))
            if not bits: bad.append((name, "full-list forces differ as bit patterns"))
        st = dict(zip(STATS, run[f"{tag}_stats"].tolist()))
        print(f"{name}: {st['n_tiles']} tiles, {sum(len(a) for a in l_ref)} entries, {n_in} inner entries, cluster pairs "
              f"{st['n_cluster_pairs']}, inner {st['n_inner_cluster_pairs']}, forces bitwise {bits}")
    return bad


_runs = {}


def runs_of(which, tmp_path_factory):
    if which not in _runs:
        d = tmp_path_factory.mktemp(f"prune_hitbits_{which}")
        _runs[which] = {arm: run_child(which, arm, str(d / f"{arm}.npz")) for arm in CASES[which][1]}
    return _runs[which]


@pytest.mark.parametrize("which", list(CASES))
def test_hit_bits_leave_the_lists_bit_for_bit(tmp_path_factory, which):
    runs = runs_of(which, tmp_path_factory)
    ref = runs["ballots"]
    st = dict(zip(STATS, ref["half_start_stats"].tolist()))
    assert st["n_cluster_pairs"] > 0 and st["rebuild_fallbacks"] == 0
    if which == "solvated":
        c = ref["half_start_counts"]
        assert (c[:, 0] > 0).any(), "no masked entries"
    if which in ("solvated", "short"):
        c = ref["half_start_counts"]
        print(f"{which}: tiles with masked entries {(c[:, 0] > 0).sum()}, without a plain chunk {(c[:, 1] == 0).sum()}, "
              f"with a single chunk {((c[:, 0] + c[:, 1]) <= 8).sum()} of {c.shape[0]}")
    bad = []
    for arm in CASES[which][1][1:]:
        bad += compare(which, arm, ref, runs[arm])
    assert not bad, bad


def min_image(d, box):
    return d - np.round(d / box) * box


def cluster_pair_min_distances(run, tag, ent_lists, box):
    """fp64 minimum atom distance of every cluster pair whose mask bit is set in `ent_lists` (per tile) -> one array"""
    pos = run[f"{tag}_pos"].astype(np.float64)
    orig = run[f"{tag}_orig_of"].astype(np.int64)                  # [T, 64] slot -> atom
    far = np.full((1, 3), np.nan)
    slot_pos = np.concatenate([pos, far])[np.where(orig == 0xFFFFFFFF, len(pos), orig)]      # [T, 64, 3]; dummies: NaN
    cl = np.concatenate([slot_pos.reshape(-1, 8, 3), np.full((8, 8, 3), np.nan)])            # [T * 8 + null tile, 8, 3]
    out = []
    for t, ent in enumerate(ent_lists):
        if not len(ent):
            continue
        jc, mask = ent[:, 0].astype(np.int64), (ent[:, 1] >> 8) & 0xFF
        e_idx, ci = np.nonzero((mask[:, None] >> np.arange(8)[None, :]) & 1)
        if not len(e_idx):
            continue
        assert (jc[e_idx] < orig.shape[0] * 8).all(), "a kept cluster pair names the null cluster"
        xi, xj = cl[t * 8 + ci], cl[jc[e_idx]]                     # [P, 8, 3]
        d = min_image(xi[:, :, None, :] - xj[:, None, :, :], box)
        d2 = (d * d).sum(-1).reshape(len(e_idx), 64)
        d2 = np.where(np.isnan(d2), np.inf, d2)
        out.append(np.sqrt(d2.min(1)))
    return np.concatenate(out)


@pytest.mark.parametrize("tag", ["half_start", "half_moved", "full_start"])
def test_kept_set_against_fp64_distances(tmp_path_factory, tag):
    from molchanica_amd import systems
    run = runs_of("water", tmp_path_factory)["hitbits"]
    s = systems.water_box(16, seed=41)
    box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    assert (box > 4 * (CUTOFF + SKIN)).all()
    pos = run[f"{tag}_pos"].astype(np.float64)
    n = len(pos)
    # every atom pair within the list radius less the margin is in the neighbour list
    off, idx = run[f"{tag}_nl_off"].astype(np.int64), run[f"{tag}_nl_idx"].astype(np.int64)
    have = np.repeat(np.arange(n, dtype=np.int64), np.diff(off)) * n + idx
    r_in = CUTOFF + SKIN - MARGIN
    assert (np.diff(have) > 0).all()
    n_close, missing = 0, 0
    if tag == "half_moved":      # (all pairs j > i once, off the lattice and across the cell's faces: 75 M distances; both orders looked up)
        for a in range(0, n, 512):
            d2 = np.zeros((min(512, n - a), n - a))
            for k in range(3):
                d = pos[a:a + 512, None, k] - pos[None, a:, k]
                d -= np.round(d / box[k]) * box[k]
                d2 += d * d
            i, j = np.nonzero(d2 < r_in * r_in)
            i, j = i[j > i] + a, j[j > i] + a
            for want in (i * n + j, j * n + i):
                n_close += len(want)
                at = np.minimum(np.searchsorted(have, want), len(have) - 1)
                missing += int((have[at] != want).sum())
        assert n_close > 0
    print(f"{tag}: {n_close} ordered atom pairs within {r_in} A, {len(have)} in the neighbour list, missing {missing}")
    assert missing == 0
    # every kept cluster pair has an atom pair within the radius plus the margin
    lists, inners = tile_runs(run, tag)
    dmin = cluster_pair_min_distances(run, tag, lists, box)
    print(f"{tag}: {len(dmin)} kept cluster pairs, largest minimum distance {dmin.max():.6f} A")
    assert len(dmin) == int(run[f"{tag}_stats"][STATS.index("n_cluster_pairs")])
    assert dmin.max() < CUTOFF + SKIN + MARGIN
    assert (tag != "full_start") == (inners is not None)
    if inners is not None:
        dmin_in = cluster_pair_min_distances(run, tag, inners, box)
        print(f"{tag}: {len(dmin_in)} cluster pairs in the inner list, largest minimum distance {dmin_in.max():.6f} A")
        assert 0 < len(dmin_in) < len(dmin) and dmin_in.max() < CUTOFF + INNER_SKIN + MARGIN
        # ... and the inner list misses none: cluster pairs of the list with an atom pair inside the inner radius less the margin
        assert len(dmin_in) >= int((dmin < CUTOFF + INNER_SKIN - MARGIN).sum())
