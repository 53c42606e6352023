"""`mdx_pose_rmsd` / `mdx_cluster_poses` through `MdState.pose_rmsd` / `MdState.cluster_poses` on the device, against the numpy
restatement of the rule (tests/pose_cluster_ref.py), against closed forms at size, against themselves (a pair alone and anywhere in a
batch, repeated calls, shuffled input, optional outputs left out, the handle untouched) and behind `search_poses`.

rmsd: within 1 fp32 ulp of the reference - D is the same sequence of fp64 operations on both sides, so the only admissible difference
is the last bit of the fp64 sqrt of two maths libraries tipping the one rounding to fp32; the number of values not bit-equal is printed.
Clusterings: leaders, cluster ids and sizes equal for every pose; the inputs hold no pair within 1e-9, relative, of the cutoff
(tests/test_pose_cluster_host.py checks that without a GPU, cluster() of the reference asserts it again).

Poses lie around lig50's coordinates (or crystal_case's 12-atom molecule, or one atom) inside small_complex's box.  Counts of values
not bit-equal as measured on an MI355X: DESIGN.md section 7i."""
import ctypes as C
import threading

import numpy as np
import pytest

from molchanica_amd import MdConfig, _abi, systems
from tests import pose_cluster_cases as K
from tests import pose_cluster_ref as R
from tests.test_gpu_pose_batch import small_configs, three_groups
from tests.test_pose_flex_host import ligand_case, start_poses

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mdx():
    from molchanica_amd import md_state
    assert md_state.device_count() >= 1, "no GPU: the HIP path must run here, there is no fallback"
    return md_state


@pytest.fixture(scope="module")
def box_md(mdx):
    """a periodic handle: small_complex in its 30 A box"""
    with mdx.MdState(systems.small_complex(), small_configs()[0]) as md:
        lo, hi = md.cell()
        assert np.array_equal(R.box_edges(lo, hi), K.periodic_edges())
        yield md


@pytest.fixture(scope="module")
def vac_md(mdx):
    """a vacuum handle"""
    with mdx.MdState(systems.lig50(), MdConfig(lj_cutoff=0, coulomb_cutoff=0)) as md:
        yield md


L = K.periodic_edges()
VACUUM = (0.0, 0.0, 0.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def ulps(a, b):
    return np.abs(np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64))


def against_the_reference(got, poses_a, poses_b, mask, perms, box, what):
    want = R.rmsd(poses_a, poses_b, mask, perms, box)
    assert got.shape == want.shape and got.dtype == np.float32
    u = ulps(got, want)
    print(f"{what}: {int((u != 0).sum())} of {u.size} rmsd values not bit-equal to the reference, worst {int(u.max())} ulp")
    assert u.max() <= 1, f"{what}: rmsd differs from the reference by {u.max()} fp32 ulp"
    return int((u != 0).sum())


def spread_poses(count, n, seed):
    """n poses: the molecule jittered by 0.4 A and translated by up to 0.7 L, so that many pairs are nearest through a box face"""
    rng = np.random.default_rng(seed)
    return (K.jittered(K.base(count), n, 0.4, seed) + rng.uniform(-0.7, 0.7, (n, 1, 3)) * L[None, None, :]).astype(np.float32)


@pytest.mark.parametrize("n_a,n_b,count", [(1, 1, 1), (2, 3, 12), (63, 65, 50), (130, 1, 50), (65, 64, 256)])
def test_pose_rmsd_against_the_reference(box_md, vac_md, n_a, n_b, count):
    """Tile tails in both dimensions, one atom and the largest count (eight atom chunks), with and without a mask, 0 / 1 / 2 / 12 perms
    (above 32 masked atoms the permuted side is staged anew per chunk and perm), A against B and A against A, periodic and vacuum"""
    a, b = spread_poses(count, n_a, 10 * count + n_a), spread_poses(count, n_b, 10 * count + n_b + 1000)
    ident = np.arange(count, dtype=np.uint32)[None, :]
    variants = [(None, None), (None, ident)]
    if count >= 12:
        swap = np.concatenate([ident, ident])
        swap[1, [1, 4]] = [4, 1]
        variants += [(None, swap), (None, K.ring_perms(count)), (K.ring_mask(count), None), (K.ring_mask(count), K.ring_perms(count))]
    differ = 0
    for mask, perms in variants:
        what = f"({n_a}, {n_b}, {count}) mask {mask is not None} perms {0 if perms is None else len(perms)}"
        differ += against_the_reference(box_md.pose_rmsd(a, b, mask, perms), a, b, mask, perms, L, what + " periodic")
        differ += against_the_reference(box_md.pose_rmsd(a, None, mask, perms), a, None, mask, perms, L, what + " periodic, A against A")
    mask, perms = variants[-1]
    differ += against_the_reference(vac_md.pose_rmsd(a, b, mask, perms), a, b, mask, perms, VACUUM, f"({n_a}, {n_b}, {count}) vacuum")
    print(f"({n_a}, {n_b}, {count}): {differ} values not bit-equal in all variants")


def test_the_periodic_image(box_md, vac_md):
    """A pose against its copies translated by +-L along every axis and by 0.49 L and 0.51 L: the periodic handle sees the nearest image
    of the centroid, the vacuum handle the translation - both as the reference does"""
    x = K.base(50)
    shifts = [np.zeros(3)] + [sg * L * np.eye(3)[ax] for ax in range(3) for sg in (1.0, -1.0)] + [f * L * np.eye(3)[ax] for ax in range(3) for f in (0.49, 0.51)]
    poses = np.stack([x + s for s in shifts]).astype(np.float32)
    per, vac = box_md.pose_rmsd(poses), vac_md.pose_rmsd(poses)
    against_the_reference(per, poses, None, None, None, L, "images, periodic")
    against_the_reference(vac, poses, None, None, None, VACUUM, "images, vacuum")
    assert (per[0, 1:7] < 1e-4).all(), per[0]
    assert np.allclose(per[0, 7::2], 0.49 * L, rtol=1e-5) and np.allclose(per[0, 8::2], 0.49 * L, rtol=1e-5), per[0, 7:]
    assert np.allclose(vac[0, 1:7], np.repeat(L, 2), rtol=1e-6) and np.allclose(vac[0, 8::2], 0.51 * L, rtol=1e-5), vac[0]
    # nearer than half a box: no shift at all, the periodic handle returns the vacuum handle's bits
    near = K.jittered(x, 20, 0.5, 3)
    assert np.array_equal(bits(box_md.pose_rmsd(near)), bits(vac_md.pose_rmsd(near)))


CASES = K.clustering_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_clustering_against_the_reference(box_md, vac_md, case):
    name, poses, scores, cut, mask, perms = case
    for md, box in zip((box_md, vac_md), K.boxes_of(case)):      # (the larger cases on the periodic handle only)
        want = R.cluster(poses, scores, cut, mask, perms, box)
        got = md.cluster_poses(poses, scores, cut, mask, perms)
        for a, b, what in zip(got, want, ("leaders", "cluster_of", "rmsd_to_leader", "sizes")):
            if what != "rmsd_to_leader":
                assert a.dtype == np.uint32 and np.array_equal(a, b), (name, what)
        leaders, cluster_of, rm, sizes = got
        assert int(sizes.sum()) == len(poses) and np.array_equal(np.bincount(cluster_of, minlength=len(leaders)), sizes)
        assert (cluster_of[leaders] == np.arange(len(leaders))).all() and (rm[leaders] == 0.0).all()
        # rmsd_to_leader carries the bits pose_rmsd(leader, p) returns
        full = md.pose_rmsd(poses[leaders], poses, mask, perms)
        mine = full[cluster_of, np.arange(len(poses))]
        mine[leaders] = 0.0
        assert np.array_equal(bits(rm), bits(mine)), f"{name}: rmsd_to_leader is not what pose_rmsd returns"
        u = ulps(rm, want[2])
        assert u.max() <= 1
    print(f"{name}: {len(leaders)} clusters of {sizes.min()} - {sizes.max()}, {int((u != 0).sum())} of {u.size} rmsd_to_leader values not bit-equal to the reference")


@pytest.mark.parametrize("count", [1, 3])
def test_closed_form_at_size(box_md, count):
    """8192 poses: 4096 lattice sites 1.5 A apart, each occupied twice, cut 1 A, scores a permutation: 4096 clusters of two, each led by
    its lower-scored copy, the leaders in score order.  (The lattice is wider than half the box: pairs are nearest through a face.)"""
    poses, scores, site = K.lattice(count, 21 + count)
    leaders, cluster_of, rm, sizes = box_md.cluster_poses(poses, scores, 1.0)
    assert len(leaders) == 4096 and (sizes == 2).all()
    assert (np.diff(scores[leaders]) > 0).all(), "the leaders are not in score order"
    assert np.array_equal(site[leaders][cluster_of], site), "a pose is not with its site's other copy"
    first = np.full(4096, np.inf)
    np.minimum.at(first, site, scores)
    assert np.array_equal(scores[leaders], first[site[leaders]]), "a cluster is not led by its lower-scored copy"
    assert (rm == 0.0).all()


def test_the_cap(box_md, mdx):
    with pytest.raises(mdx.ParamError):
        box_md.cluster_poses(np.zeros((_abi.CLUSTER_MAX_POSES + 1, 1, 3), np.float32), np.zeros(_abi.CLUSTER_MAX_POSES + 1), 1.0)
    lib = mdx.load_library()
    k = C.c_uint32(77)
    p = np.zeros((_abi.CLUSTER_MAX_POSES + 1, 1, 3), np.float32)
    sc = np.zeros(len(p))
    rc = lib.mdx_cluster_poses(box_md._h, 1, len(p), p.ctypes.data_as(C.POINTER(C.c_float)), sc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, None, 1.0,
                               C.byref(k), None, None, None, None)
    assert rc == _abi.MDX_EPARAM and k.value == 77 and b"MDX_CLUSTER_MAX_POSES" in lib.mdx_last_error()
    # the cap itself is taken: 16384 single atoms on a line of 8.2 A, neighbours 0.0005 A apart, scores in line order, cut 0.00125 A:
    # greedy along the line, a leader takes the next two poses (0.0005, 0.0010 <= 0.00125 < 0.0015, hundreds of fp32 ulp from the cutoff)
    n = _abi.CLUSTER_MAX_POSES
    x = np.zeros((n, 1, 3), np.float32)
    x[:, 0, 0] = 0.0005 * np.arange(n)
    leaders, cluster_of, rm, sizes = box_md.cluster_poses(x, np.arange(n, dtype=np.float64), 0.00125)
    assert np.array_equal(leaders, np.arange(0, n, 3)) and np.array_equal(cluster_of, np.arange(n) // 3) and int(sizes.sum()) == n


def test_a_pair_gives_the_same_bits_anywhere(box_md):
    """A pose pair alone and at places 0 / 63 / 64 / last of a batch; repeated calls; clustering: shuffled input with distinct scores
    gives the same partition, optional outputs may be NULL"""
    count = 50
    perms, mask = K.ring_perms(count), K.ring_mask(count)
    batch = spread_poses(count, 131, 77)
    a, b = spread_poses(count, 2, 78)
    alone = box_md.pose_rmsd(a[None], b[None], mask, perms)
    assert alone.shape == (1, 1)
    for ia in (0, 63, 64, 130):
        for ib in (0, 63, 64, 130):
            A, B = batch.copy(), batch.copy()
            A[ia], B[ib] = a, b
            got = box_md.pose_rmsd(A, B, mask, perms)
            assert bits(got[ia:ia + 1, ib])[0] == bits(alone)[0, 0], (ia, ib)
    one = box_md.pose_rmsd(batch, None, mask, perms)
    assert np.array_equal(bits(one), bits(box_md.pose_rmsd(batch, None, mask, perms)))
    assert np.array_equal(bits(one), bits(box_md.pose_rmsd(batch, batch, mask, perms)))
    # clustering
    name, poses, scores, cut, cmask, cperms = next(c for c in CASES if c[0].startswith("close families N=257"))
    first = box_md.cluster_poses(poses, scores, cut, cmask, cperms)
    again = box_md.cluster_poses(poses, scores, cut, cmask, cperms)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(first, again))
    assert len(np.unique(scores)) == len(scores)
    mix = np.random.default_rng(4).permutation(len(poses))
    shuf = box_md.cluster_poses(poses[mix], scores[mix], cut, cmask, cperms)
    assert np.array_equal(mix[shuf[0]], first[0]) and np.array_equal(shuf[1], first[1][mix]) and np.array_equal(bits(shuf[2]), bits(first[2][mix]))
    assert np.array_equal(shuf[3], first[3])
    from molchanica_amd import md_state
    lib = md_state.load_library()
    k = C.c_uint32(0)
    fp, dp, up = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    sc = np.ascontiguousarray(scores)
    assert lib.mdx_cluster_poses(box_md._h, poses.shape[1], len(poses), poses.ctypes.data_as(fp), sc.ctypes.data_as(dp), None, 0, None, cut, C.byref(k),
                                 None, None, None, None) == 0 and k.value == len(first[0])
    cl = np.full(len(poses), 77, np.uint32)
    assert lib.mdx_cluster_poses(box_md._h, poses.shape[1], len(poses), poses.ctypes.data_as(fp), sc.ctypes.data_as(dp), None, 0, None, cut, C.byref(k),
                                 None, cl.ctypes.data_as(up), None, None) == 0 and np.array_equal(cl, first[1])
    # leader_out is written for n_clusters entries only
    lead = np.full(len(poses), 77, np.uint32)
    assert lib.mdx_cluster_poses(box_md._h, poses.shape[1], len(poses), poses.ctypes.data_as(fp), sc.ctypes.data_as(dp), None, 0, None, cut, C.byref(k),
                                 lead.ctypes.data_as(up), None, None, None) == 0
    assert np.array_equal(lead[:k.value], first[0]) and (lead[k.value:] == 77).all()
    # no poses: success, nothing but the count
    k = C.c_uint32(77)
    assert lib.mdx_cluster_poses(box_md._h, 5, 0, None, None, None, 0, None, 1.0, C.byref(k), lead.ctypes.data_as(up), None, None, None) == 0 and k.value == 0
    assert (lead[len(first[0]):] == 77).all()
    assert box_md.pose_rmsd(np.zeros((0, 5, 3), np.float32)).shape == (0, 0)


def test_refusals_leave_the_outputs(box_md, mdx):
    """Every refusal, on a live handle: MDX_EPARAM with its message, and every output as it was"""
    lib = mdx.load_library()
    fp, up, bp, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    count, n = 6, 4
    good = K.jittered(K.base(12)[:count], n, 0.3, 2)
    scores = np.arange(n, dtype=np.float64)
    out = np.full((n, n), -7.0, np.float32)
    k_out = C.c_uint32(77)
    lead, cl, sz = (np.full(n, 77, np.uint32) for _ in range(3))
    rm = np.full(n, -7.0, np.float32)
    P = lambda a, t: None if a is None else a.ctypes.data_as(t)
    h = box_md._h

    def rmsd(count=count, n_a=n, a=good, n_b=n, b=good, mask=None, perms=None, n_perms=None, dst=out):
        return lib.mdx_pose_rmsd(h, count, n_a, P(a, fp), n_b, P(b, fp), P(mask, bp), (0 if perms is None else len(perms)) if n_perms is None else n_perms,
                                 P(perms, up), P(dst, fp))

    def clus(count=count, n=n, a=good, sc=scores, mask=None, perms=None, n_perms=None, cut=1.0, k=True):
        return lib.mdx_cluster_poses(h, count, n, P(a, fp), P(sc, dp), P(mask, bp), (0 if perms is None else len(perms)) if n_perms is None else n_perms,
                                     P(perms, up), cut, C.byref(k_out) if k else None, P(lead, up), P(cl, up), P(rm, fp), P(sz, up))

    def refused(rc, match):
        assert rc == _abi.MDX_EPARAM and match in lib.mdx_last_error(), (rc, match, lib.mdx_last_error())

    bad_pose, bad_score = good.copy(), scores.copy()
    bad_pose[1, 2, 0], bad_score[2] = np.inf, np.nan
    ident = np.arange(count, dtype=np.uint32)[None, :]
    mask = np.array([1, 1, 0, 0, 1, 1], np.uint8)
    for call in (rmsd, clus):
        refused(call(count=0), b"MDX_POSE_MAX_ATOMS")
        refused(call(count=257), b"MDX_POSE_MAX_ATOMS")
        refused(call(a=None), b"null")
        refused(call(mask=np.zeros(count, np.uint8)), b"mask")
        refused(call(perms=np.tile(ident, (65, 1))), b"MDX_CLUSTER_MAX_PERMS")
        refused(call(n_perms=1), b"null perms")
        refused(call(perms=np.array([[0, 1, 2, 3, 4, 5], [0, 0, 2, 3, 4, 5]], np.uint32)), b"perm 1 is not a bijection")
        refused(call(perms=np.array([[1, 0, 2, 3, 4, 5]], np.uint32)), b"identity")
        refused(call(mask=mask, perms=np.array([[0, 1, 2, 3, 4, 5], [2, 1, 0, 3, 4, 5]], np.uint32)), b"unmasked")
        refused(call(a=bad_pose), b"non-finite")
    refused(rmsd(n_a=16385), b"MDX_CLUSTER_MAX_POSES")
    refused(rmsd(n_b=16385), b"MDX_CLUSTER_MAX_POSES")
    refused(rmsd(b=bad_pose), b"non-finite")
    refused(rmsd(dst=None), b"null")
    refused(clus(n=16385), b"MDX_CLUSTER_MAX_POSES")
    refused(clus(sc=None), b"null")
    refused(clus(k=False), b"null")
    refused(clus(sc=bad_score), b"NaN")
    for cut in (-1e-3, float("nan"), float("inf")):
        refused(clus(cut=cut), b"rmsd_cut")
    assert (out == -7.0).all() and (rm == -7.0).all() and k_out.value == 77 and all((a == 77).all() for a in (lead, cl, sz))
    assert rmsd() == 0 and clus(cut=0.0) == 0 and k_out.value == n      # ... and the same arrays are written by a call that is not refused


def test_refused_on_a_decomposed_handle(mdx):
    from molchanica_amd.md_state import Fabric, MdState, ParamError
    s = systems.small_complex(box=44.0)
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, coulomb_mode=1, chunk_steps=8)
    poses = K.jittered(K.base(12), 3, 0.3, 1)
    world = 2
    fabric = Fabric(world)
    errs = []

    def run(rank):
        try:
            with MdState(s, cfg) as md:
                md.comm_init_fabric(fabric, rank)
                for call in (lambda: md.pose_rmsd(poses), lambda: md.cluster_poses(poses, np.zeros(3), 1.0)):
                    with pytest.raises(ParamError, match="decomposed"):
                        call()
        except BaseException as e:   # pragma: no cover
            errs.append(e)
            fabric.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]


def test_the_handle_is_untouched(mdx):
    """The twin test of tests/test_gpu_pose_search.py::test_the_handle_is_untouched with pose_rmsd and cluster_poses in place of
    search_poses: energies, positions, forces and velocities as before the calls, and ten further steps bit for bit those of a twin
    that made no such call"""
    s = systems.small_complex()
    cfg = MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5, nb_variant=2)
    name, poses, scores, cut, mask, perms = next(c for c in CASES if "12 perms and a mask" in c[0])
    with mdx.MdState(s, cfg) as md, mdx.MdState(s, cfg) as twin:
        for m in (md, twin):
            m.step(0.0005, None, 4)
        e0, x0, f0, v0 = md.energy(), md.positions(), md.forces(), md.velocities()
        rebuilds = md.stats()["rebuild_count"]
        md.pose_rmsd(poses, None, mask, perms)
        md.cluster_poses(poses, scores, cut, mask, perms)
        assert md.stats()["rebuild_count"] == rebuilds
        e1, x1, f1, v1 = md.energy(), md.positions(), md.forces(), md.velocities()
        atomic_sums = ("kinetic", "temperature", "pressure", "bond", "angle", "dihedral", "lj14", "coulomb14", "potential_bonded", "potential_nonbonded",
                       "potential")
        for k in e0:
            if k in atomic_sums:
                assert e1[k] == pytest.approx(e0[k], rel=1e-13), k
            else:
                assert e0[k] == e1[k], (k, e0[k], e1[k])
        assert np.array_equal(bits(v0), bits(v1)) and np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1))
        twin.energy(), twin.positions(), twin.forces(), twin.velocities()
        md.step(0.0005, None, 10)
        twin.step(0.0005, None, 10)
        assert np.array_equal(bits(md.positions()), bits(twin.positions()))
        assert np.array_equal(bits(md.velocities()), bits(twin.velocities()))
        assert md.stats()["rebuild_count"] == twin.stats()["rebuild_count"]


def test_behind_a_search(mdx):
    """End to end: search_poses with 64 walkers for a few rounds on small_complex, then cluster_poses of its best poses and scores - the
    leaders' scores ascend, every member is within the cut of its leader, every pair of leaders is further apart than the cut (by the
    reference), the sizes sum to 64"""
    s, lo, hi, bonds, tb, tors, terms = ligand_case()
    g = three_groups(s)
    cut = 2.0
    with mdx.MdState(s, small_configs()[0]) as md:
        md.set_energy_groups(g, 3)
        starts = start_poses(s, md.positions(), lo, hi, tors, n=64)
        best, rows, score, dih, best_round, stats = md.search_poses(lo, starts, 0, tb, 3, 0.5, 0.15, 0.4, 100.0, 78, 6, 0.0, 0.0, 0.0)
        mask = np.asarray(s.mass)[lo:hi] > 1.5      # the heavy atoms
        leaders, cluster_of, rm, sizes = md.cluster_poses(best, score, cut, mask)
        edges = R.box_edges(*md.cell())
    n_m = int(mask.sum())
    assert int(sizes.sum()) == 64 and len(leaders) == len(sizes) >= 1
    assert (np.diff(score[leaders]) >= 0).all()
    D = R.distance(best[leaders], best, mask, None, edges)
    T = R.threshold(cut, n_m)
    assert (D[cluster_of, np.arange(64)] <= T).all(), "a member is further than the cut from its leader"
    ll = D[:, leaders]
    assert (ll[~np.eye(len(leaders), dtype=bool)] > T).all(), "two leaders are within the cut of each other"
    assert ulps(rm, np.where(np.isin(np.arange(64), leaders), np.float32(0), R.rmsd_of(D[cluster_of, np.arange(64)], n_m))).max() <= 1
    print(f"64 walkers, 3 rounds: {len(leaders)} clusters, sizes {sizes.tolist()}")
