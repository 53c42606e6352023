"""Inputs of the pose-distance and clustering tests, shared by tests/test_pose_cluster_host.py (which checks, without a GPU, that no
clustering case holds a pair near the cutoff) and tests/test_gpu_pose_cluster.py.  Everything is generated from fixed seeds."""
import numpy as np

from molchanica_amd import systems
from tests import pose_cluster_ref as R

BOX = 30.0                                   # small_complex's cubic box, origin 0
CENTRE = np.array([15.0, 15.0, 15.0])
RING = [(i, (i + 1) % 6) for i in range(6)]
CUT = 2.0


def base(count):
    """One molecule of `count` atoms about the centre of the box, fp64 [count, 3]: one atom, crystal_case's 12-atom molecule, lig50, or
    lig50 laid out six times over (count 256: only the number of atoms matters to the distance)"""
    if count == 1:
        return CENTRE[None, :].copy()
    if count == 12:
        s = systems.molecular_crystal()
        x = np.asarray(s.pos, np.float64)[int(s.mol_start[0]):int(s.mol_start[1])]
    else:
        x = np.asarray(systems.lig50().pos, np.float64)
        if count > 50:
            x = np.concatenate([x + 0.7 * k * np.array([1.0, -0.5, 0.25]) for k in range(6)])[:count]
    assert x.shape[0] >= count
    x = x[:count]
    return x - x.mean(0) + CENTRE


def ring_perms(count):
    """The 12 images of a six-ring on atoms 0..5, the other atoms fixed: uint32 [12, count], the identity first"""
    from molchanica_amd.topology import ligand_automorphisms
    p = ligand_automorphisms(6, RING, [0] * 6)
    assert p.shape == (12, 6)
    out = np.tile(np.arange(count, dtype=np.uint32), (12, 1))
    out[:, :6] = p
    return out


def ring_mask(count):
    """the ring and every other atom behind it"""
    m = np.zeros(count, np.uint8)
    m[:6] = 1
    m[6::2] = 1
    return m


def jittered(x, n, sigma, seed):
    rng = np.random.default_rng(seed)
    return (x[None, :, :] + rng.normal(0.0, sigma, (n,) + x.shape)).astype(np.float32)


def families(count, n, seed, n_fam=7, sigma=0.3, shuffle_ring=False, spacing=6.0):
    """n poses in n_fam families `spacing` A from the first, each pose its family's placement with a jitter of sigma per coordinate -> (poses, scores,
    family of every pose).  shuffle_ring: every pose's ring atoms are relabelled by a random image of the ring, so that only the
    symmetry-aware distance finds the families."""
    rng = np.random.default_rng(seed)
    x = base(count)
    offs = spacing * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)[:n_fam]
    fam = rng.integers(0, n_fam, n)
    poses = x[None, :, :] + offs[fam][:, None, :] + rng.normal(0.0, sigma, (n, count, 3))
    if shuffle_ring:
        P = ring_perms(count)
        pick = rng.integers(0, 12, n)
        poses = np.stack([poses[i][P[pick[i]]] for i in range(n)])
    return poses.astype(np.float32), rng.normal(0.0, 5.0, n), fam


def continuum(count, n, seed, cut=CUT):
    """One pose translated along x in steps of 0.33 cut, the scores a fixed permutation: which poses lead depends on the score order.
    (Steps of exactly cut / 3 would put every pair three steps apart ON the cutoff, which cluster() of the reference refuses.)"""
    rng = np.random.default_rng(seed)
    x = base(count)
    poses = np.stack([x + np.array([0.33 * cut * (i - n // 2), 0.0, 0.0]) for i in range(n)])
    return poses.astype(np.float32), rng.permutation(n).astype(np.float64)


def clustering_cases():
    """-> [(name, poses, scores, cut, mask, perms)]: what the device is held against the reference on"""
    out = []
    for n, count in ((257, 12), (1500, 50)):
        p, s, _ = families(count, n, 100 + n)
        out.append((f"families N={n} count={count}", p, s, CUT, None, None))
        # six families 1.9 A from the first: with the jitter their members lie on both sides of the cutoff from its leader, some near it
        p, s, _ = families(count, n, 200 + n, spacing=1.9)
        out.append((f"close families N={n} count={count}", p, s, CUT, None, None))
    p, s, _ = families(12, 257, 7, shuffle_ring=True)
    out.append(("families N=257 count=12, ring relabelled, 12 perms and a mask", p, s, CUT, ring_mask(12), ring_perms(12)))
    p, s, _ = families(50, 300, 8, shuffle_ring=True)
    out.append(("families N=300 count=50, ring relabelled, 12 perms", p, s, CUT, None, ring_perms(50)))
    p, s = continuum(12, 130, 9)
    out.append(("continuum N=130 count=12", p, s, CUT, None, None))
    out.append(("continuum N=130 count=12, scores reversed", p, -s, CUT, None, None))
    p, s, _ = families(12, 200, 10)
    out.append(("tied scores N=200 count=12", p, np.round(s / 4.0), CUT, None, None))
    p, s, _ = families(12, 70, 11, sigma=0.2)
    dup = np.concatenate([p, p[::3], p[5:40:7]])
    rng = np.random.default_rng(12)
    out.append(("duplicates N=%d count=12, cut 0" % len(dup), dup, rng.normal(0.0, 1.0, len(dup)), 0.0, None, None))
    p, s, _ = families(50, 150, 13)
    s = s.copy()
    s[::7] = np.inf
    out.append(("+inf scores N=150 count=50", p, s, CUT, ring_mask(50), None))
    return out


def lattice(count, seed, side=16, spacing=1.5):
    """side^3 sites of a cubic lattice inside the box, each occupied twice, scores a fixed permutation of 0 .. 2 side^3 - 1
    -> (poses [2 side^3, count, 3], scores, site of every pose)"""
    rng = np.random.default_rng(seed)
    g = np.arange(side) * spacing + 3.0
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    mol = np.array([[0.0, 0.0, 0.0], [0.4, 0.1, 0.0], [0.0, 0.3, 0.2]])[:count]
    site = np.concatenate([np.arange(len(sites)), np.arange(len(sites))])
    poses = (sites[site][:, None, :] + mol[None, :, :]).astype(np.float32)
    mix = rng.permutation(len(site))
    return poses[mix], rng.permutation(len(site)).astype(np.float64), site[mix]


def periodic_edges():
    return R.box_edges((0.0, 0.0, 0.0), (BOX, BOX, BOX))


VACUUM = (0.0, 0.0, 0.0)


def boxes_of(case):
    """The box edges a clustering case is run with: the periodic box, and for the smaller cases vacuum as well (the continuum is wider
    than the box, so its two results differ)"""
    return [periodic_edges()] + ([np.array(VACUUM)] if len(case[1]) <= 400 else [])
