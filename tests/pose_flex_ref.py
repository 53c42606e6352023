"""The stepper of `mdx_refine_poses_flex` (include/mdx.h states it) in numpy fp64, shared by tests/test_pose_flex_host.py (no GPU),
tests/test_gpu_pose_flex.py and tools/pose_flex_rates.py: the rigid stepper of tests/pose_refine_ref.py with the ligand's torsion angles
as further coordinates.  It is parameterised by `evaluate(Y) -> (row, rigid, forces)`: with `MdState.pose_forces` behind it, it is
the host loop the device loop replaces; with the oracle behind it, it is independent of the library.

Statement by statement it follows molchanica_amd/csrc/mdx_flex_step.h: sums over atoms and terms run in order (np.cumsum adds
sequentially), products are rounded before they are added, so the two differ by the last bit of sin / cos / sqrt / atan2 at most."""
import math

import numpy as np

from tests import pose_refine_ref as P

MAX_TORSIONS = 32
E_ROOT, E_INDEX, E_SELF, E_NOT_BONDED, E_TWICE, E_RING, E_LEAF, E_DISCONNECTED = 1, 2, 3, 4, 5, 6, 7, 8


class GraphError(ValueError):
    def __init__(self, code, torsion):
        super().__init__(f"rule {code} broken by torsion {torsion}")
        self.code, self.torsion = code, torsion


def seq_sum(a):
    """sum of a[0], a[1], ... in that order (along axis 0), starting from 0"""
    a = np.asarray(a, np.float64)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a, axis=0)[-1]


# ---- the bond graph -----------------------------------------------------------------------------------------------------------------------
def local_bonds(s, lo, hi):
    """bonds and constraints of the system inside [lo, hi), ligand-local"""
    pairs = [np.asarray(s.bond_idx, np.int64).reshape(-1, 2)]
    if getattr(s, "constraint_idx", None) is not None and len(s.constraint_idx):
        pairs.append(np.asarray(s.constraint_idx, np.int64).reshape(-1, 2))
    b = np.concatenate(pairs)
    keep = ((b >= lo) & (b < hi)).all(1)
    return b[keep] - lo


def _reach(count, adj, start, skip):
    seen = np.zeros(count, bool)
    seen[start] = True
    stack = [start]
    while stack:
        i = stack.pop()
        for j in adj[i]:
            if (i, j) == skip or (j, i) == skip or seen[j]:
                continue
            seen[j] = True
            stack.append(j)
    return seen


def moving_sides(count, bonds, root, torsions):
    """-> [(a_k, b_k, mask_k bool [count])]: the side of bond k without `root` moves, b_k its end of the bond.  GraphError otherwise."""
    bonds = [(int(p), int(q)) for p, q in np.asarray(bonds, np.int64).reshape(-1, 2)]
    tors = [(int(p), int(q)) for p, q in np.asarray(torsions, np.int64).reshape(-1, 2)]
    if not 0 <= root < count:
        raise GraphError(E_ROOT, 0)
    adj = [[] for _ in range(count)]
    for p, q in bonds:
        adj[p].append(q)
        adj[q].append(p)
    for k, (a, b) in enumerate(tors):
        if not (0 <= a < count and 0 <= b < count):
            raise GraphError(E_INDEX, k)
        if a == b:
            raise GraphError(E_SELF, k)
        if (a, b) not in bonds and (b, a) not in bonds:
            raise GraphError(E_NOT_BONDED, k)
        if (a, b) in tors[:k] or (b, a) in tors[:k]:
            raise GraphError(E_TWICE, k)
    if tors and not _reach(count, adj, root, None).all():
        raise GraphError(E_DISCONNECTED, 0)
    out = []
    for k, (a, b) in enumerate(tors):
        fixed = _reach(count, adj, root, (a, b))
        if fixed[a] and fixed[b]:
            raise GraphError(E_RING, k)
        if fixed.sum() == 1 or count - fixed.sum() == 1:
            raise GraphError(E_LEAF, k)
        out.append((a, b, ~fixed) if fixed[a] else (b, a, ~fixed))
    return out


def rotatable_bonds(count, bonds, root=0):
    """Every bond of a ligand that can be declared a torsion, in bond order."""
    out = []
    for p, q in np.asarray(bonds, np.int64).reshape(-1, 2):
        try:
            moving_sides(count, bonds, root, [(p, q)])
        except GraphError:
            continue
        out.append((int(p), int(q)))
    return np.array(out, np.uint32).reshape(-1, 2)


# ---- the ligand's dihedral terms ----------------------------------------------------------------------------------------------------------
def dihedral_terms(s, lo, hi):
    """-> (atoms [Nt, 4] ligand-local, v, phase, n) of the system's dihedral terms inside [lo, hi), in list order"""
    idx = np.asarray(s.dihedral_idx, np.int64).reshape(-1, 4)
    keep = ((idx >= lo) & (idx < hi)).all(1)
    return (idx[keep] - lo, np.asarray(s.dihedral_v, np.float32)[keep].astype(np.float64),
            np.asarray(s.dihedral_phase, np.float32)[keep].astype(np.float64), np.asarray(s.dihedral_n)[keep].astype(np.float64))


NO_TERMS = (np.zeros((0, 4), np.int64), np.zeros(0), np.zeros(0), np.zeros(0))


def _mimg(d, box):
    if box is None:
        return d
    box = np.asarray(box, np.float64)
    on = box > 0
    out = d.copy()
    out[:, on] = d[:, on] - np.rint(d[:, on] / box[on]) * box[on]
    return out


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def dihedral(Y, terms, box=None):
    """-> (E fp64: the terms' energies added in list order, f [n, 3] fp64: per atom, the terms that name it in list order) at fp32 Y"""
    at, v, phase, n = terms
    y = np.asarray(Y, np.float32).astype(np.float64)
    f = np.zeros_like(y)
    if len(at) == 0:
        return 0.0, f
    xi, xj, xk, xl = (y[at[:, r]] for r in range(4))
    F, G, H = _mimg(xi - xj, box), _mimg(xj - xk, box), _mimg(xl - xk, box)
    A, B = _cross(F, G), _cross(H, G)
    A2, B2, Gn = _dot(A, A), _dot(B, B), np.sqrt(_dot(G, G))
    ok = ~((A2 < 1e-24) | (B2 < 1e-24) | (Gn < 1e-12))
    with np.errstate(all="ignore"):
        cosphi = _dot(A, B)
        sinphi = _dot(_cross(B, A), G) / Gn
        phi = np.arctan2(sinphi, cosphi)
        arg = n * phi - phase
        E = v * (1.0 + np.cos(arg))
        dE = -(v * n) * np.sin(arg)
        FG, HG = _dot(F, G), _dot(H, G)
        ca, cb, ta, tb = Gn / A2, Gn / B2, FG / (A2 * Gn), HG / (B2 * Gn)
        wa = np.stack([-ca, ca + ta, -ta, np.zeros_like(ca)], axis=1)
        wb = np.stack([np.zeros_like(cb), -tb, tb - cb, cb], axis=1)
        Ft = -(dE[:, None, None] * (wa[:, :, None] * A[:, None, :] + wb[:, :, None] * B[:, None, :]))
    E = np.where(ok, E, 0.0)
    Ft = np.where(ok[:, None, None], Ft, 0.0)
    np.add.at(f, at.reshape(-1), Ft.reshape(-1, 3))      # (unbuffered, in order: term by term)
    return float(seq_sum(E)), f


# ---- torsion gradient, atom field, trial ---------------------------------------------------------------------------------------------------
def axis(y, a, b):
    d = y[b] - y[a]
    ln = P.norm3(d)
    if not ln > 0.0:
        return None
    return d / ln


def gradient(y, f, v, tors):
    """-> (g [T], J [T], A [T, 3], axes [T, 3]) of fp64 y, f [n, 3]"""
    T = len(tors)
    g, J, A, U = np.zeros(T), np.zeros(T), np.zeros((T, 3)), np.zeros((T, 3))
    for k, (a, b, mask) in enumerate(tors):
        u = axis(y, a, b)
        if u is None:
            continue
        U[k] = u
        arm = np.cross(u, y[mask] - y[b])      # (np.cross: a1 b2 - a2 b1, products rounded first)
        fm = f[mask] - v
        g[k] = seq_sum((arm[:, 0] * fm[:, 0] + arm[:, 1] * fm[:, 1]) + arm[:, 2] * fm[:, 2])
        J[k] = seq_sum((arm[:, 0] * arm[:, 0] + arm[:, 1] * arm[:, 1]) + arm[:, 2] * arm[:, 2])
        A[k] = seq_sum(arm)
    return g, J, A, U


def omega(g, J):
    return g / ((J + P.LAMBDA_REL * J) + P.LAMBDA_ABS)


def speeds(v, w, c, y, tors, U, wk, A):
    """|u_i| of the atom field"""
    r = y - c
    n = float(len(y))
    u = np.stack([v[0] + (w[1] * r[:, 2] - w[2] * r[:, 1]), v[1] + (w[2] * r[:, 0] - w[0] * r[:, 2]),
                  v[2] + (w[0] * r[:, 1] - w[1] * r[:, 0])], axis=1)
    for k, (a, b, mask) in enumerate(tors):
        shift = (wk[k] * A[k]) / n
        arm = np.cross(U[k], y[mask] - y[b])
        u[mask] = u[mask] + (wk[k] * arm - shift)
        u[~mask] = u[~mask] - shift
    return np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def build(x0, tors, theta):
    """B(theta): fp64 [n, 3], the torsions in caller order, each about its axis as the coordinates then stand"""
    x = np.asarray(x0, np.float32).astype(np.float64)
    for k, (a, b, mask) in enumerate(tors):
        th = float(theta[k])
        if th == 0.0:
            continue
        u = axis(x, a, b)
        if u is None:
            continue
        cs, sn = math.cos(th), math.sin(th)
        m = mask.copy()
        m[b] = False
        r = x[m] - x[b]
        cr = np.cross(u, r)
        dt = (u[0] * r[:, 0] + u[1] * r[:, 1]) + u[2] * r[:, 2]
        oc = 1.0 - cs
        x[m] = x[b] + ((r * cs + cr * sn) + (u[None, :] * dt[:, None]) * oc)
    return x


def coords(c0, t, q, x0, tors, theta):
    """fp32(c0 + t + R(q) b), b = B(theta) - mean(B(theta))"""
    R = P.rotation(q)
    B = build(x0, tors, theta)
    b = B - P.mean(B)
    out = np.empty(b.shape, np.float32)
    for d in range(3):
        out[:, d] = ((c0[d] + t[d]) + ((R[d, 0] * b[:, 0] + R[d, 1] * b[:, 1]) + R[d, 2] * b[:, 2])).astype(np.float32)
    return out


def state_of(Y, forces, rigid, tors, terms, box=None):
    """What the stepper derives from one evaluation: -> (E_dih fp32, f [n, 3] fp64 = (double) f_nb + f_dih, g [T], J, A, axes)"""
    y = np.asarray(Y, np.float32).astype(np.float64)
    E, fd = dihedral(Y, terms, box)
    f = np.asarray(forces, np.float32).astype(np.float64) + fd
    v = np.asarray(rigid, np.float32).astype(np.float64)[:3] / float(len(y))
    return (np.float32(E), f) + gradient(y, f, v, tors)


def refine(x0, evaluate, tors, terms, max_evals, f_tol, tau_tol, tors_tol, h_start=0.0, h_max=0.0, box=None, trace=None):
    """One pose.  evaluate(Y float32 [n, 3]) -> (row float32 [G], rigid float32 [6], forces float32 [n, 3]); tors from moving_sides();
    terms from dihedral_terms() or NO_TERMS.  trace, if a list, receives (flags, h, next trial or None) per evaluation.
    -> dict(pose, row, rigid, q, t, theta, edih, g, status, evals, S)"""
    x0 = np.ascontiguousarray(x0, np.float32)
    n, T = len(x0), len(tors)
    f_tol, tau_tol, tors_tol = (float(np.float32(v)) for v in (f_tol, tau_tol, tors_tol))
    h = float(np.float32(h_start)) if h_start > 0 else P.H_START
    h_max = float(np.float32(h_max)) if h_max > 0 else P.H_MAX
    c0 = P.mean(x0.astype(np.float64))
    q = qt = np.array([1.0, 0.0, 0.0, 0.0])
    t = tt = np.zeros(3)
    th = tht = np.zeros(T)
    acc = dict(status=P.MAX_EVALS, evals=0, edih=np.float32(0.0), g=np.zeros(T))
    v = w = wk = A = U = None
    m = 0.0
    Y = x0.copy()
    for k in range(max_evals):
        row, rigid, forces = evaluate(Y)
        row, rigid, forces = np.asarray(row, np.float32), np.asarray(rigid, np.float32), np.asarray(forces, np.float32)
        acc["evals"] = k + 1
        with np.errstate(all="ignore"):
            edih, f, g, J, A_new, U_new = state_of(Y, forces, rigid, tors, terms, box)
        finite = bool(np.isfinite(row).all() and np.isfinite(rigid).all() and np.isfinite(forces).all() and np.isfinite(edih)
                      and np.isfinite(f).all() and np.isfinite(g).all())
        S = 0.0
        for r in row:
            S += float(r)
        S += float(edih)
        gmax = float(np.abs(g).max()) if T else 0.0
        flags = 0
        if not finite and k == 0:
            acc.update(pose=Y.copy(), row=row, rigid=rigid, S=S, status=P.NONFINITE, edih=edih, g=g)
            flags = P.STORE | P.FROZEN
        elif finite and (k == 0 or S < acc["S"]):
            q, t, th = qt, tt, tht
            acc.update(pose=Y.copy(), row=row, rigid=rigid, S=S, edih=edih, g=g)
            if k > 0:
                h = min(1.2 * h, h_max)
            flags = P.STORE
            gr = rigid.astype(np.float64)
            if P.norm3(gr[:3]) <= f_tol and P.norm3(gr[3:]) <= tau_tol and gmax <= tors_tol:
                acc["status"] = P.CONVERGED
                flags |= P.FROZEN
            else:
                x = Y.astype(np.float64)
                c = P.mean(x)
                v = gr[:3] / float(n)
                w = P.solve(P.inertia(x, c), gr[3:])
                wk, A, U = omega(g, J), A_new, U_new
                m = float(speeds(v, w, c, x, tors, U, wk, A).max())
                if m == 0.0:
                    acc["status"] = P.CONVERGED
                    flags |= P.FROZEN
        else:
            h = 0.5 * h
            if h < P.H_MIN:
                acc["status"] = P.STALLED
                flags = P.FROZEN
        if flags & P.FROZEN:
            if trace is not None:
                trace.append((flags, h, None))
            break
        qt, tt = P.trial(q, t, v, w, h, m)
        tht = th + (h / m) * wk
        Y = coords(c0, tt, qt, x0, tors, tht)
        if trace is not None:
            trace.append((flags, h, Y.copy()))
    acc.update(q=q, t=t, theta=th)
    return acc


def refine_batch(poses, evaluate, tors, terms, max_evals, f_tol, tau_tol, tors_tol, h_start=0.0, h_max=0.0, box=None):
    """Every pose by itself.  -> (poses_out, rows, rigid, xform float32 [P, 7 + T], dih, tgrad, status, evals)"""
    res = [refine(p, evaluate, tors, terms, max_evals, f_tol, tau_tol, tors_tol, h_start, h_max, box) for p in poses]
    return (np.stack([r["pose"] for r in res]), np.stack([r["row"] for r in res]), np.stack([r["rigid"] for r in res]),
            np.stack([np.concatenate([r["q"], r["t"], r["theta"]]).astype(np.float32) for r in res]),
            np.array([r["edih"] for r in res], np.float32), np.stack([r["g"].astype(np.float32) for r in res]),
            np.array([r["status"] for r in res], np.uint32), np.array([r["evals"] for r in res], np.uint32))


def host_evaluate(md, first, n_groups):
    """`evaluate` of the host loop the device loop replaces: one `MdState.pose_forces` call per evaluation (MDX_ENAN: all NaN)."""
    from molchanica_amd.md_state import BlowUpError

    def evaluate(Y):
        try:
            f, row, rigid = md.pose_forces(first, np.ascontiguousarray(Y[None]), rows=True, rigid=True)
        except BlowUpError:
            return np.full(n_groups, np.nan, np.float32), np.full(6, np.nan, np.float32), np.full(Y.shape, np.nan, np.float32)
        return row[0], rigid[0], f[0]
    return evaluate


def synthetic_evaluate(targets, k):
    """The quadratic field of tests/pose_refine_ref.py with its per-atom forces: f_i = fp32(-k (Y_i - T_i))"""
    T = np.asarray(targets, np.float64)
    rigid_field = P.synthetic_evaluate(targets, k)

    def evaluate(Y):
        row, rigid = rigid_field(Y)
        y = np.asarray(Y, np.float32).astype(np.float64)
        return row, rigid, (-(k * (y - T))).astype(np.float32)
    return evaluate


def turn(lig, tors, theta):
    """`lig` [n, 3] with the torsions turned by theta (fp64; B(theta) of fp64 input)"""
    x = np.asarray(lig, np.float64).copy()
    for k, (a, b, mask) in enumerate(tors):
        if theta[k] == 0.0:
            continue
        u = (x[b] - x[a]) / np.linalg.norm(x[b] - x[a])
        r = x[mask] - x[b]
        x[mask] = x[b] + r * math.cos(theta[k]) + np.cross(u, r) * math.sin(theta[k]) + np.outer(r @ u, u) * (1.0 - math.cos(theta[k]))
    return x


def flex_poses(start, tors, n, seed, amp, **rigid_kw):
    """Start poses of the GPU tests: rigid_poses(...) of tests/test_gpu_pose_batch.py with the torsions then turned by amp u w^2
    (u uniform in [-1, 1], w uniform in [0, 1]); pose 0 stays the start."""
    from tests.test_gpu_pose_batch import rigid_poses
    poses = rigid_poses(start, n, seed, **rigid_kw).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    for k in range(1, n):
        theta = amp * rng.uniform(-1.0, 1.0, len(tors)) * rng.random(len(tors)) ** 2
        poses[k] = turn(poses[k], tors, theta)
    return poses.astype(np.float32)
