"""numpy restatement of the rule of `mdx_pose_rmsd` / `mdx_cluster_poses` (include/mdx.h): the symmetry-aware distance of two poses in the
receptor's frame and the greedy leader clustering by it.  Sequential in the atoms - every sum in the rule's order, one fp64 operation per
numpy operation, so nothing is contracted or reordered - and vectorised over the pose pairs.  Written from the rule's statement, not from
molchanica_amd/csrc/mdx_cluster_rule.h; the tests hold the header (on the host) and the kernels (on the device) against it."""
import numpy as np

MAX_POSES, MAX_PERMS = 16384, 64
MARGIN = 1e-9      # cluster(): no pair of the inputs may lie this near the cutoff, relative to T


def masked_atoms(count, mask=None):
    """M: the masked atoms in atom order"""
    return np.arange(count) if mask is None else np.flatnonzero(np.asarray(mask).reshape(count) != 0)


def box_edges(box_lo, box_hi, periodic=True):
    """L of the rule: (double) box_hi - (double) box_lo of the handle's fp32 box; 0 where not periodic"""
    lo, hi = np.asarray(box_lo, np.float32).astype(np.float64), np.asarray(box_hi, np.float32).astype(np.float64)
    return (hi - lo) if periodic else np.zeros(3)


def centroid(poses, M):
    """c(p) of every pose: the fp64 mean over M in atom order -> [n, 3]"""
    x = np.asarray(poses, np.float32).astype(np.float64)
    c = np.zeros((x.shape[0], 3))
    for k in M:
        c = c + x[:, k, :]
    return c / float(len(M))


def shift(ca, cb, L):
    """s of every pair (a row, b column): L rint((c(b) - c(a)) / L) on a periodic axis, 0 elsewhere -> [A, B, 3]"""
    L = np.asarray(L, np.float64)
    s = np.zeros((ca.shape[0], cb.shape[0], 3))
    for ax in range(3):
        if L[ax] > 0.0:
            s[:, :, ax] = L[ax] * np.rint((cb[None, :, ax] - ca[:, None, ax]) / L[ax])
    return s


def distance(a, b=None, mask=None, perms=None, L=(0.0, 0.0, 0.0)):
    """D(a_i, b_j) for every pair, fp64 [A, B]: the minimum over the perms, in their order, of the sum over M in atom order, then x, y,
    z, of d d with d = (a_k - b_pi(k)) + s"""
    a = np.asarray(a, np.float32)
    b = a if b is None else np.asarray(b, np.float32)
    count = a.shape[1]
    M = masked_atoms(count, mask)
    P = np.arange(count)[None, :] if perms is None or len(perms) == 0 else np.asarray(perms, np.int64)
    s = shift(centroid(a, M), centroid(b, M), L)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    D = None
    for pi in P:
        acc = np.zeros((a.shape[0], b.shape[0]))
        for k in M:
            for ax in range(3):
                d = (a64[:, k, ax][:, None] - b64[:, pi[k], ax][None, :]) + s[:, :, ax]
                acc = acc + d * d
        D = acc if D is None else np.where(acc < D, acc, D)
    return D


def threshold(cut, n_m):
    """T = (cut cut) n_m, cut an fp32 number"""
    c = float(np.float32(cut))
    return (c * c) * float(n_m)


def rmsd_of(D, n_m):
    return np.sqrt(D / float(n_m)).astype(np.float32)


def rmsd(a, b=None, mask=None, perms=None, L=(0.0, 0.0, 0.0)):
    """what `pose_rmsd` returns: float32 [A, B]"""
    count = np.asarray(a).shape[1]
    return rmsd_of(distance(a, b, mask, perms, L), len(masked_atoms(count, mask)))


def rank(scores):
    """(score ascending, index ascending); +inf last"""
    s = np.asarray(scores, np.float64)
    assert not np.isnan(s).any()
    return np.argsort(s, kind="stable")


def smallest_margin(D, T):
    """min over the pairs i != j of |D - T| / T (inf where T == 0: then D <= T is D == 0, decided exactly)"""
    if T == 0.0:
        return np.inf
    off = ~np.eye(D.shape[0], dtype=bool)
    return float((np.abs(D[off] - T) / T).min()) if off.any() else np.inf


def cluster(poses, scores, cut, mask=None, perms=None, L=(0.0, 0.0, 0.0), info=None):
    """Greedy leader clustering -> (leaders [K], cluster_of [N], rmsd_to_leader [N] f32, sizes [K]).  Asserts that no pair of the inputs
    lies within MARGIN, relative, of the cutoff: a result that hangs on the last bits of a sum is no test of anything."""
    poses = np.asarray(poses, np.float32)
    n, count = poses.shape[0], poses.shape[1]
    n_m = len(masked_atoms(count, mask))
    order = rank(scores)
    T = threshold(cut, n_m)
    D = distance(poses[order], None, mask, perms, L)      # [leader side a, member side b], rank order
    margin = smallest_margin(D, T)
    assert margin > MARGIN, f"a pair of the inputs lies within {margin:.2e} of the cutoff"
    if info is not None:
        info["margin"], info["T"] = margin, T
    leaders, cluster_of, rm, sizes = [], np.zeros(n, np.uint32), np.zeros(n, np.float32), []
    for r in range(n):
        c = next((k for k, lr in enumerate(leaders) if D[lr, r] <= T), None)
        if c is None:
            c = len(leaders)
            leaders.append(r)
            sizes.append(0)
        else:
            rm[order[r]] = rmsd_of(D[leaders[c], r], n_m)
        cluster_of[order[r]] = c
        sizes[c] += 1
    return order[np.asarray(leaders, np.int64)].astype(np.uint32), cluster_of, rm, np.asarray(sizes, np.uint32)
