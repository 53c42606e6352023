"""The rule of mdx_solubility_mixing (include/mdx.h) restated in numpy fp64, from its text: the solubility mixing diagnostics of
n_copies solute copies in water, with the per-atom sums, and the bound on what the device's fp32 pair arithmetic may add to a sum."""
import numpy as np

SIGMAS = (4.0, 7.0, 10.0)
CONTACT = 4.2
PENALTY_STRENGTH = 3.5
LOG_GAIN = 80.0
FIELDS = ("score", "raw_score", "local_mixing", "solute_dispersion", "mixture_score", "aggregation_factor", "aggregation_penalty",
          "largest_cluster_fraction", "contacted_fraction", "contact_pair_fraction")
FLT_EPSILON = float(np.finfo(np.float32).eps)


def cell_edges(lo, hi):
    """L = box_hi - box_lo in fp32 -> float64 [3]"""
    return (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)).astype(np.float64)


def sigmas(L):
    """min(sigma, 0.9 half) then max(., 1), half = 0.5 max(min L, 1), in fp32 -> float64 [3]"""
    f = np.float32
    half = f(0.5) * max(f(np.min(L)), f(1.0))
    return np.array([max(min(f(s), f(0.9) * half), f(1.0)) for s in SIGMAS], np.float32).astype(np.float64)


def image(d, L):
    return d - L * np.rint(d / L)


def wrap(x, lo, L):
    return x - L * np.floor((x - lo) / L)


def pair_geometry(sol, wat, lo, hi):
    """sol float32 [n_copies, n_sel, 3], wat float32 [n_w, 3] -> (rows [n_rows, 3], partners [n_rows + n_w, 3], copy of every partner
    (-1: water), raw differences and minimum-image differences [n_rows, n_partners, 3]), all float64"""
    n_copies, n_sel, _ = sol.shape
    rows = sol.reshape(-1, 3).astype(np.float64)
    part = np.concatenate([rows, np.asarray(wat, np.float32).astype(np.float64)])
    copy = np.concatenate([np.repeat(np.arange(n_copies), n_sel), np.full(len(wat), -1)])
    raw = part[None, :, :] - rows[:, None, :]
    return rows, part, copy, raw, image(raw, cell_edges(lo, hi))


def atom_sums(sol, wat, lo, hi):
    """-> (sums float64 [n_rows, 3 sigmas, 2]: S over the selected atoms of the other copies and W over the oxygens, before
    normalisation; d2 [n_rows, n_partners]; other [n_rows, n_partners] bool: a solute partner of another copy; water [n_partners] bool)"""
    n_copies, n_sel, _ = sol.shape
    _, _, copy, _, d = pair_geometry(sol, wat, lo, hi)
    d2 = (d * d).sum(-1)
    own = np.repeat(np.arange(n_copies), n_sel)
    water = copy < 0
    other = (~water)[None, :] & (copy[None, :] != own[:, None])
    sg = sigmas(cell_edges(lo, hi))
    sums = np.zeros((n_copies * n_sel, 3, 2))
    for k in range(3):
        e = np.exp(-d2 / (2.0 * sg[k] ** 2))
        sums[:, k, 0] = (e * other).sum(1)
        sums[:, k, 1] = e[:, water].sum(1)
    return sums, d2, other, water


def atom_scores(sums, n_copies, n_sel, n_w):
    """-> float64 [n_rows, 3]: clamp(2 W' / (S' + W'), 0, 1), 0 where S' + W' <= FLT_EPSILON; and S', W'"""
    S = sums[:, :, 0] / max(1, n_copies * n_sel - n_sel)
    W = sums[:, :, 1] / n_w
    dens = S + W
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = np.where(dens > FLT_EPSILON, np.clip(2.0 * W / np.where(dens > 0, dens, 1.0), 0.0, 1.0), 0.0)
    return sc, S, W


def contact_graph(d2, other, n_copies, n_sel):
    """-> bool [n_copies, n_copies]: some pair of selected atoms has d2 <= 4.2f * 4.2f"""
    cut2 = float(np.float32(CONTACT) * np.float32(CONTACT))
    hit = other & (d2 <= cut2)
    n_rows = n_copies * n_sel
    return hit[:, :n_rows].reshape(n_copies, n_sel, n_copies, n_sel).any(axis=(1, 3))


def aggregation(touch):
    """-> (factor, penalty: float64; p, c, f: float32 ratios of integers)"""
    n = touch.shape[0]
    f32 = np.float32
    if n < 2:
        return 1.0, 0.0, f32(0), f32(0), f32(0)
    t = touch | touch.T
    np.fill_diagonal(t, False)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i in range(n):
        for j in range(i + 1, n):
            if t[i, j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[b] = a
    sizes = np.bincount([find(i) for i in range(n)], minlength=n)
    pairs = int(np.triu(t, 1).sum())
    p = f32(int(sizes.max()) - 1) / f32(n - 1)
    c = f32(int(t.any(1).sum())) / f32(n)
    f = f32(pairs) / f32(n * (n - 1) // 2)
    pen = float(np.clip(0.55 * float(p) ** 1.25 + 0.30 * float(c) ** 2 + 0.15 * float(f) ** 0.5, 0.0, 1.0))
    return float(np.clip(np.exp(-PENALTY_STRENGTH * pen), 0.0, 1.0)), pen, p, c, f


def dispersion(sol, lo, hi):
    n_copies = sol.shape[0]
    if n_copies < 2:
        return 1.0
    L = cell_edges(lo, hi)
    lo64 = np.asarray(lo, np.float32).astype(np.float64)
    x = sol.astype(np.float64)
    anchor = wrap(x[:, :1, :], lo64, L)
    centre = wrap((anchor + image(x - anchor, L)).mean(1), lo64, L)
    i, j = np.triu_indices(n_copies, 1)
    d = image(centre[j] - centre[i], L)
    rms = np.sqrt((d * d).sum(1).mean())
    return float(np.clip(rms / np.sqrt((L * L).sum() / 12.0), 0.0, 1.0))


def diagnostics(sol, wat, lo, hi, full=False):
    """The ten fields as float32 under the reference's names; full=True: -> (fields, extras: sums, scores, d2, other, water)"""
    sol = np.asarray(sol, np.float32)
    wat = np.asarray(wat, np.float32)
    n_copies, n_sel, _ = sol.shape
    sums, d2, other, water = atom_sums(sol, wat, lo, hi)
    sc, S, W = atom_scores(sums, n_copies, n_sel, len(wat))
    local = float(sc.mean(0).mean())
    factor, pen, p, c, f = aggregation(contact_graph(d2, other, n_copies, n_sel))
    disp = dispersion(sol, lo, hi)
    mixture = local * (0.60 + 0.40 * disp)
    raw = float(np.clip(factor * mixture, 0.0, 1.0))
    score = float(np.log(1.0 + LOG_GAIN * raw) / np.log(1.0 + LOG_GAIN))
    out = dict(zip(FIELDS, (np.float32(v) for v in (score, raw, local, disp, mixture, factor, pen, p, c, f))))
    if full:
        return out, dict(sums=sums, scores=sc, S=S, W=W, d2=d2, other=other, water=water)
    return out


# ---- what fp32 pair arithmetic may add to a sum (DESIGN §7k derives it) ---------------------------------------------------------------
U = 2.0 ** -24      # unit round-off of fp32


def sum_bounds(sol, wat, lo, hi):
    """-> float64 [n_rows, 3, 2]: a bound on |device sum - restated sum| per selected atom, sigma and kind.  Both sides add in fp64; the
    device forms each term in fp32: the difference of the coordinates (error <= U |raw| per axis), the image shift n L (n L rounded: U
    |raw|; the subtraction: U |d|; an image chosen the other way next to half a box changes |d| by no more than 4 U L), d2 (three products,
    two additions: 4 U d2), the product with k = fp32(-log2(e) / 2 sigma^2) (2 U x in x = d2 / 2 sigma^2) and the hardware exp2 (within two
    units in the last place, result rounding included: 4 U).  A term e^-x therefore moves by at most e^-x (expm1(dx) + 4 U)."""
    sol = np.asarray(sol, np.float32)
    n_copies, n_sel, _ = sol.shape
    L = cell_edges(lo, hi)
    _, _, copy, raw, d = pair_geometry(sol, wat, lo, hi)
    ar, ad = np.abs(raw), np.abs(d)
    eps = U * (2.0 * ar + ad) + np.where(ad > 0.5 * L * (1.0 - 1e-6), 4.0 * U * L, 0.0)
    d2 = (d * d).sum(-1)
    dd2 = (2.0 * ad * eps + eps * eps).sum(-1) + 4.0 * U * d2
    own = np.repeat(np.arange(n_copies), n_sel)
    water = copy < 0
    other = (~water)[None, :] & (copy[None, :] != own[:, None])
    sg = sigmas(L)
    out = np.zeros((n_copies * n_sel, 3, 2))
    for k in range(3):
        x = d2 / (2.0 * sg[k] ** 2)
        dx = dd2 / (2.0 * sg[k] ** 2) + 2.0 * U * x
        dt = np.exp(-x) * (np.expm1(dx) + 4.0 * U)
        out[:, k, 0] = (dt * other).sum(1)
        out[:, k, 1] = dt[:, water].sum(1)
    return out


def local_mixing_bound(sums, bounds, n_copies, n_sel, n_w):
    """The bound on local_mixing that follows from the bounds on the sums: s = 2 W' / (S' + W') has |ds| <= 2 (S' dW' + W' dS') / (S' + W' -
    dS' - dW')^2 (the clamp does not stretch), then the means; plus one fp32 rounding of the field."""
    S = sums[:, :, 0] / max(1, n_copies * n_sel - n_sel)
    W = sums[:, :, 1] / n_w
    dS = bounds[:, :, 0] / max(1, n_copies * n_sel - n_sel)
    dW = bounds[:, :, 1] / n_w
    den = np.maximum(S + W - dS - dW, 1e-300)
    ds = np.where(S + W > FLT_EPSILON, 2.0 * (S * dW + W * dS) / den ** 2, 0.0)
    return float(ds.mean(0).mean()) + 2.0 * U


def field_bounds(fields, b_local):
    """Bounds on the ten fields from the bound on local_mixing.  The fractions are exact; dispersion, penalty and factor are the same
    fp64 arithmetic on both sides (one fp32 rounding apart: 2 U of a value <= 1); mixture <= local's bound; raw = factor mixture;
    score = ln(1 + 80 raw) / ln 81 has slope <= 80 / ln 81."""
    r = 2.0 * U
    b_mix = b_local + r
    b_raw = b_mix + r
    return {"local_mixing": b_local, "solute_dispersion": r, "aggregation_penalty": r, "aggregation_factor": r, "mixture_score": b_mix,
            "raw_score": b_raw, "score": LOG_GAIN / np.log(1.0 + LOG_GAIN) * b_raw / (1.0 + LOG_GAIN * max(float(fields["raw_score"]) - b_raw, 0.0)) + r,
            "largest_cluster_fraction": 0.0, "contacted_fraction": 0.0, "contact_pair_fraction": 0.0}
