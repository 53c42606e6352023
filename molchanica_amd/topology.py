"""Bonded-term and exclusion lists from a bond graph.

Host-side system build (the part of `MdState::new` that "build[s] bonded term lists from
bonds/adjacency"; input shape at /root/reference src/md/mod.rs:1110-1120
`bonds`, `adjacency_list`).  Setup-time only; not on the accelerated path.
"""
from __future__ import annotations

import numpy as np

from ._abi import CLUSTER_MAX_PERMS


def adjacency(n_atoms: int, bonds: np.ndarray) -> list[list[int]]:
    adj: list[list[int]] = [[] for _ in range(n_atoms)]
    for a, b in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        adj[a].append(int(b))
        adj[b].append(int(a))
    return [sorted(set(x)) for x in adj]


def angles_from_bonds(adj: list[list[int]]) -> np.ndarray:
    out = []
    for j, nb in enumerate(adj):
        for x in range(len(nb)):
            for y in range(x + 1, len(nb)):
                out.append((nb[x], j, nb[y]))
    return np.asarray(out, dtype=np.uint32).reshape(-1, 3)


def dihedrals_from_bonds(adj: list[list[int]]) -> np.ndarray:
    out = []
    for j, nbj in enumerate(adj):
        for k in nbj:
            if k <= j:
                continue
            for i in nbj:
                if i == k:
                    continue
                for l in adj[k]:
                    if l == j or l == i:
                        continue
                    out.append((i, j, k, l))
    return np.asarray(out, dtype=np.uint32).reshape(-1, 4)


def exclusions_and_pairs14(n_atoms: int, adj: list[list[int]]):
    """1-2 and 1-3 partners -> exclusion CSR (symmetric); 1-4 partners that are not also
    1-2/1-3 -> unique (i<j) pair list."""
    excl: list[set[int]] = [set() for _ in range(n_atoms)]
    for i, nb in enumerate(adj):
        for j in nb:
            excl[i].add(j)
            for k in adj[j]:
                if k != i:
                    excl[i].add(k)
    p14 = set()
    for i, nb in enumerate(adj):
        for j in nb:
            for k in adj[j]:
                if k == i:
                    continue
                for l in adj[k]:
                    if l == j or l == i or l in excl[i]:
                        continue
                    p14.add((min(i, l), max(i, l)))
    offsets = np.zeros(n_atoms + 1, dtype=np.uint32)
    for i in range(n_atoms):
        offsets[i + 1] = offsets[i] + len(excl[i])
    idx = np.zeros(int(offsets[-1]), dtype=np.uint32)
    for i in range(n_atoms):
        idx[offsets[i]:offsets[i + 1]] = sorted(excl[i])
    pairs = np.asarray(sorted(p14), dtype=np.uint32).reshape(-1, 2)
    return offsets, idx, pairs


def csr_from_pairs(n_atoms: int, pairs: np.ndarray):
    """Symmetric exclusion CSR from an (i,j) pair array — vectorised, for large systems."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    both = np.concatenate([pairs, pairs[:, ::-1]], axis=0)
    order = np.lexsort((both[:, 1], both[:, 0]))
    both = both[order]
    counts = np.bincount(both[:, 0], minlength=n_atoms)
    offsets = np.zeros(n_atoms + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(counts)
    return offsets, both[:, 1].astype(np.uint32)


def pairs_from_csr(offsets: np.ndarray, idx: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """The inverse of csr_from_pairs for the atoms [lo, hi): every (i, j) of their rows with i != j as a sorted pair, each once, in
    GLOBAL indices -> int64 [P, 2].  A partner outside [lo, hi) stays in the list: the caller decides what that means."""
    off = np.asarray(offsets, dtype=np.int64)
    ii = np.repeat(np.arange(lo, hi, dtype=np.int64), np.diff(off[lo:hi + 1]))
    jj = np.asarray(idx, dtype=np.int64)[off[lo]:off[hi]]
    keep = ii != jj
    pairs = np.sort(np.stack([ii[keep], jj[keep]], 1), axis=1)
    return np.unique(pairs, axis=0).reshape(-1, 2)


def _side_of(count: int, adj: list[list[int]], start: int, skip) -> np.ndarray:
    """The atoms reachable from `start` without crossing the bond `skip` -> bool [count]."""
    seen = np.zeros(count, bool)
    seen[start] = True
    stack = [start]
    while stack:
        i = stack.pop()
        for j in adj[i]:
            if seen[j] or (skip is not None and {i, j} == skip):
                continue
            seen[j] = True
            stack.append(j)
    return seen


def rotatable_bonds(count: int, bonds, root: int = 0) -> np.ndarray:
    """The bonds of a ligand that `MdState.refine_poses_flex` / `refine_guests_flex` accept as a torsion, in bond order: removing the bond
    splits the ligand in two parts of at least two atoms each (no ring bond, no leaf bond), in a bond graph that is connected.
    bonds: integer [B, 2], ligand-local.  -> uint32 [T, 2], each pair as it is listed.  A listed pair with an index outside
    0 .. count-1 and a pair of an atom with itself are left out; with root outside the ligand there is none."""
    count, root = int(count), int(root)
    b = np.asarray(bonds, np.int64).reshape(-1, 2)
    if not 0 <= root < count:
        return np.zeros((0, 2), np.uint32)
    ok = ((b >= 0) & (b < count)).all(1)
    adj: list[list[int]] = [[] for _ in range(count)]
    for p, q in b[ok]:
        adj[int(p)].append(int(q))
        adj[int(q)].append(int(p))
    out = []
    if b.shape[0] and _side_of(count, adj, root, None).all():
        for k, (p, q) in enumerate(b):
            p, q = int(p), int(q)
            if not ok[k] or p == q:
                continue
            fixed = _side_of(count, adj, root, {p, q})
            n_fixed = int(fixed.sum())
            if (fixed[p] and fixed[q]) or n_fixed == 1 or count - n_fixed == 1:
                continue
            out.append((p, q))
    return np.array(out, np.uint32).reshape(-1, 2)


def ligand_automorphisms(n: int, bonds, keys, mask=None, cap: int = CLUSTER_MAX_PERMS) -> np.ndarray:
    """The symmetry images `MdState.pose_rmsd` / `cluster_poses` take: the automorphisms of the bond graph on n atoms that preserve the
    per-atom `keys` (e.g. the LJ type index), the identity first, de-duplicated by their action on the atoms of `mask` ([n] booleans,
    None: all) - with a heavy-atom mask the permutations of methyl hydrogens collapse; of the perms that act alike the first found
    stands for all (its unmasked atoms map in one consistent way).  -> uint32 [P, n].  Raises ParamError when more than `cap` distinct
    ones exist: a truncated set is not a group, and the distance would stop being symmetric.  Plain backtracking in atom order over
    key- and degree-compatible candidates."""
    from .md_state import ParamError
    n = int(n)
    keys = np.asarray(keys).reshape(-1)
    if keys.shape[0] != n:
        raise ParamError("ligand_automorphisms: keys must hold one entry per atom")
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    if b.size and (b.min() < 0 or b.max() >= n):
        raise ParamError("ligand_automorphisms: a bond names an atom outside 0..n-1")
    m = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if m.shape[0] != n or not m.any():
        raise ParamError("ligand_automorphisms: mask must select at least one of the n atoms")
    adj = [set(x) for x in adjacency(n, b)]
    sig = [(keys[i].item(), len(adj[i])) for i in range(n)]
    # visit the atoms so that each one after the first of its component has an earlier neighbour: candidates come from that
    # neighbour's image, not from all atoms
    order, parent, seen = [], {}, [False] * n
    for root in range(n):
        if seen[root]:
            continue
        seen[root] = True
        queue = [root]
        parent[root] = -1
        while queue:
            i = queue.pop(0)
            order.append(i)
            for j in sorted(adj[i]):
                if not seen[j]:
                    seen[j] = True
                    parent[j] = i
                    queue.append(j)
    masked = np.flatnonzero(m)
    found, actions = [], set()
    image, used = [-1] * n, [False] * n

    def place(pos):
        if pos == n:
            act = tuple(image[i] for i in masked)
            if act not in actions:
                if len(found) >= cap:
                    raise ParamError(f"ligand_automorphisms: more than cap = {cap} distinct symmetry images on the masked atoms")
                actions.add(act)
                found.append(list(image))
            return
        i = order[pos]
        cands = range(n) if parent[i] < 0 else sorted(adj[image[parent[i]]])
        for c in cands:
            if used[c] or sig[c] != sig[i]:
                continue
            # every bond of i to an atom placed before it must be a bond of the images (equal degrees make the converse hold at the end)
            if any(image[j] >= 0 and image[j] not in adj[c] for j in adj[i]):
                continue
            image[i], used[c] = c, True
            place(pos + 1)
            image[i], used[c] = -1, False

    import sys
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, n + 200))
    try:
        place(0)
    finally:
        sys.setrecursionlimit(limit)
    found.sort(key=lambda p: (p != list(range(n)),))      # (stable: the identity first, the others in the order found)
    return np.asarray(found, dtype=np.uint32).reshape(-1, n)
