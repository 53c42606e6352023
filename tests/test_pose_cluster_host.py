"""`mdx_pose_rmsd` / `mdx_cluster_poses` without a GPU: the declarations, every refusal that is decided before a device is touched (with
the outputs left as they were), the Python-side validation, the rule's header (molchanica_amd/csrc/mdx_cluster_rule.h, the code the
kernels run) compiled into a stand-alone host program and held against the numpy restatement of tests/pose_cluster_ref.py, the symmetry
helper `ligand_automorphisms` on graphs with known groups, and the condition on the clustering inputs the GPU tests rely on: no pair
within 1e-9, relative, of the cutoff."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from molchanica_amd import _abi
from molchanica_amd.topology import ligand_automorphisms
from tests import pose_cluster_cases as K
from tests import pose_cluster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")
OUT = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT, "pose_cluster_driver")
SRC = os.path.join(ROOT, "tests", "cpp", "pose_cluster_driver.cpp")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    l.mdx_pose_rmsd.argtypes = _abi.POSE_RMSD_ARGTYPES
    l.mdx_cluster_poses.argtypes = _abi.CLUSTER_POSES_ARGTYPES
    return l


def _compile(exe, extra=("-O1",)):
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "molchanica_amd", "csrc"), SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver():
    return _compile(EXE)


def driver_input(path, mode, poses, scores=None, cut=0.0, mask=None, perms=None, L=(0.0, 0.0, 0.0)):
    """the binary file tests/cpp/pose_cluster_driver.cpp reads"""
    poses = np.ascontiguousarray(poses, np.float32)
    n, count = poses.shape[:2]
    perms = np.zeros((0, count), np.uint32) if perms is None else np.ascontiguousarray(perms, np.uint32)
    scores = np.zeros(n) if scores is None else np.ascontiguousarray(scores, np.float64)
    with open(path, "wb") as f:
        f.write(struct.pack("<5I", mode, count, n, perms.shape[0], 0 if mask is None else 1))
        f.write(np.asarray(L, np.float64).tobytes())
        f.write(np.float32(cut).tobytes())
        if mask is not None:
            f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
        f.write(perms.tobytes() + poses.tobytes() + scores.tobytes())
    return str(path)


def run_driver(exe, path):
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    return run.stdout.split("\n")


def driver_pairs(exe, path):
    """mode 0 -> (T, D fp64 [n, n], rmsd fp32 [n, n])"""
    out = run_driver(exe, path)
    T = float.fromhex(out[0].split()[1])
    rows = [[w.split(":") for w in line.split()] for line in out[1:] if line]
    D = np.array([[float.fromhex(d) for d, _ in row] for row in rows])
    r = np.array([[int(b, 16) for _, b in row] for row in rows], np.uint32).view(np.float32)
    return T, D, r


def driver_clusters(exe, path):
    out = run_driver(exe, path)
    k = int(out[0].split()[1])
    ints = lambda line: np.array([int(v) for v in line.split()], np.uint32)
    rm = np.array([int(v, 16) for v in out[3].split()], np.uint32).view(np.float32)
    lead, cl, sz = ints(out[1]), ints(out[2]), ints(out[4])
    assert len(lead) == len(sz) == k
    return lead, cl, rm, sz


def ulps(a, b):
    return np.abs(np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64))


def test_header_declares_the_exports():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mdx_pose_rmsd\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_pose_rmsd"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 == len(_abi.POSE_RMSD_ARGTYPES) and args[0].startswith("mdx_handle") and args[3].startswith("const float*")
    assert args[5].startswith("const float*") and args[6].startswith("const uint8_t*") and args[8].startswith("const uint32_t*") and args[9].startswith("float*")
    m = re.search(r"\bint\s+mdx_cluster_poses\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_cluster_poses"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14 == len(_abi.CLUSTER_POSES_ARGTYPES) and args[4].startswith("const double*") and args[8] == "float rmsd_cut"
    assert args[9].startswith("uint32_t* n_clusters_out") and args[12].startswith("float*") and args[13].startswith("uint32_t*")
    for name, want in (("MDX_CLUSTER_MAX_POSES", _abi.CLUSTER_MAX_POSES), ("MDX_CLUSTER_MAX_PERMS", _abi.CLUSTER_MAX_PERMS)):
        cap = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, code)
        assert cap and int(cap.group(1)) == want
    assert (R.MAX_POSES, R.MAX_PERMS) == (_abi.CLUSTER_MAX_POSES, _abi.CLUSTER_MAX_PERMS)
    comment = src[src.index("pose distances and clustering"):src.index("#define MDX_CLUSTER_MAX_POSES")]
    for must in ("rint(", "in atom order", "min over pi", "D <= T", "(score ascending, index ascending)", "+inf", "greedy leader", "bijection", "bit for bit",
                 "same bits in a batch of any size"):
        assert must in comment, must
    search = src[src.index("pose search: per walker"):src.index("#define MDX_SEARCH_MAX_ROUNDS")]
    assert "mdx_cluster_poses" in search      # (the search no longer lists clustering as missing)
    hpp = open(os.path.join(ROOT, "include", "mdx.hpp")).read()
    assert re.search(r"\bpose_rmsd\s*\(", hpp) and re.search(r"\bcluster_poses\s*\(", hpp)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    blk = blk[:blk.index("\n}\n")]
    assert "pub fn mdx_pose_rmsd" in blk and "pub fn mdx_cluster_poses" in blk
    rule = open(os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_cluster_rule.h")).read()
    assert '#include "mdx_' not in rule      # a stand-alone host program can include it
    assert int(re.search(r"#define\s+MDX_CL_MAX_POSES\s+(\d+)u", rule).group(1)) == _abi.CLUSTER_MAX_POSES
    assert int(re.search(r"#define\s+MDX_CL_MAX_PERMS\s+(\d+)u", rule).group(1)) == _abi.CLUSTER_MAX_PERMS


def test_every_refusal_is_decided_before_any_device_is_touched(lib):
    fp, up, bp, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    count, n = 6, 4
    rng = np.random.default_rng(3)
    good = rng.normal(0.0, 1.0, (n, count, 3)).astype(np.float32)
    scores = np.arange(n, dtype=np.float64)
    ident = np.arange(count, dtype=np.uint32)[None, :]
    out = np.full((n, n), -7.0, np.float32)
    k_out = C.c_uint32(77)
    lead, cl, sz = (np.full(n, 77, np.uint32) for _ in range(3))
    rm = np.full(n, -7.0, np.float32)
    fake = C.create_string_buffer(64)      # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    h = C.addressof(fake)
    P = lambda a, t: None if a is None else a.ctypes.data_as(t)

    def rmsd(h=h, count=count, n_a=n, a=good, n_b=n, b=good, mask=None, perms=None, n_perms=None, dst=out):
        return lib.mdx_pose_rmsd(h, count, n_a, P(a, fp), n_b, P(b, fp), P(mask, bp), (0 if perms is None else len(perms)) if n_perms is None else n_perms,
                                 P(perms, up), P(dst, fp))

    def clus(h=h, count=count, n=n, a=good, sc=scores, mask=None, perms=None, n_perms=None, cut=1.0, k=True):
        return lib.mdx_cluster_poses(h, count, n, P(a, fp), P(sc, dp), P(mask, bp), (0 if perms is None else len(perms)) if n_perms is None else n_perms,
                                     P(perms, up), cut, C.byref(k_out) if k else None, P(lead, up), P(cl, up), P(rm, fp), P(sz, up))

    def refused(rc, match):
        assert rc == _abi.MDX_EPARAM, (rc, match)
        assert match in lib.mdx_last_error(), (match, lib.mdx_last_error())

    nan_pose, inf_pose = good.copy(), good.copy()
    nan_pose[2, 3, 1] = np.nan
    inf_pose[0, 0, 0] = np.inf
    nan_score = scores.copy()
    nan_score[1] = np.nan
    swap = np.array([[0, 1, 2, 3, 4, 5], [1, 0, 2, 3, 4, 5]], np.uint32)
    mask = np.array([1, 1, 0, 0, 1, 1], np.uint8)
    out_of_mask = np.array([[0, 1, 2, 3, 4, 5], [2, 1, 0, 3, 4, 5]], np.uint32)      # masked atom 0 -> unmasked atom 2
    many = np.tile(ident, (_abi.CLUSTER_MAX_PERMS + 1, 1))
    for call in (rmsd, clus):
        refused(call(h=None), b"null handle")
        refused(call(count=0), b"MDX_POSE_MAX_ATOMS")
        refused(call(count=_abi.POSE_MAX_ATOMS + 1), b"MDX_POSE_MAX_ATOMS")
        refused(call(a=None), b"null")
        refused(call(mask=np.zeros(count, np.uint8)), b"mask")
        refused(call(perms=many), b"MDX_CLUSTER_MAX_PERMS")
        refused(call(perms=None, n_perms=2), b"null perms")
        refused(call(perms=np.array([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 4]], np.uint32)), b"perm 1 is not a bijection")
        refused(call(perms=np.array([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 6]], np.uint32)), b"perm 1 is not a bijection")
        refused(call(perms=swap[::-1].copy()), b"perm 0 must be the identity")
        refused(call(mask=mask, perms=out_of_mask), b"perm 1 maps a masked atom to an unmasked one")
        refused(call(a=nan_pose), b"non-finite")
        refused(call(a=inf_pose), b"non-finite")
    refused(rmsd(n_a=_abi.CLUSTER_MAX_POSES + 1), b"MDX_CLUSTER_MAX_POSES")
    refused(rmsd(n_b=_abi.CLUSTER_MAX_POSES + 1), b"MDX_CLUSTER_MAX_POSES")
    refused(rmsd(b=nan_pose), b"non-finite")
    refused(rmsd(dst=None), b"null")
    refused(clus(n=_abi.CLUSTER_MAX_POSES + 1), b"MDX_CLUSTER_MAX_POSES")
    refused(clus(sc=None), b"null")
    refused(clus(k=False), b"null")
    refused(clus(sc=nan_score), b"NaN")
    for cut in (-0.5, float("nan"), float("inf")):
        refused(clus(cut=cut), b"rmsd_cut")
    assert (out == -7.0).all() and (rm == -7.0).all() and k_out.value == 77 and all((a == 77).all() for a in (lead, cl, sz))


def test_python_wrapper_validates_shape_and_dtype():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    ok = np.zeros((3, 5, 3), np.float32)
    sc = np.zeros(3)
    for bad in (np.zeros((3, 5, 3), np.float64), np.zeros((5, 3), np.float32), np.zeros((3, 5, 4), np.float32), np.zeros((3, 0, 3), np.float32),
                np.zeros((1, 257, 3), np.float32), np.zeros((_abi.CLUSTER_MAX_POSES + 1, 1, 3), np.float32), [[[0.0, 0.0, 0.0]]]):
        with pytest.raises(ParamError):
            md.pose_rmsd(bad)
        with pytest.raises(ParamError):
            md.pose_rmsd(ok, bad)
        with pytest.raises(ParamError):
            md.cluster_poses(bad, sc, 1.0)
    with pytest.raises(ParamError):
        md.pose_rmsd(ok, np.zeros((2, 6, 3), np.float32))
    for bad_mask in (np.ones(4, np.uint8), np.ones(5, np.float32), np.ones((5, 1), np.uint8)):
        with pytest.raises(ParamError):
            md.pose_rmsd(ok, mask=bad_mask)
        with pytest.raises(ParamError):
            md.cluster_poses(ok, sc, 1.0, mask=bad_mask)
    for bad_perms in (np.arange(5), np.arange(5.0)[None, :], np.arange(6)[None, :], np.array([[0, 1, 2, 3, 5]]), np.array([[0, 1, 2, 3, -1]]),
                      np.tile(np.arange(5), (_abi.CLUSTER_MAX_PERMS + 1, 1))):
        with pytest.raises(ParamError):
            md.pose_rmsd(ok, perms=bad_perms)
        with pytest.raises(ParamError):
            md.cluster_poses(ok, sc, 1.0, perms=bad_perms)
    for bad_scores in (np.zeros(3, np.float32), np.zeros(4), np.zeros((3, 1)), [0.0, 1.0, 2.0]):
        with pytest.raises(ParamError):
            md.cluster_poses(ok, bad_scores, 1.0)


def _pairs_case(count, n, seed, mask, perms, L, tmp_path, driver):
    """the driver's D, T and rmsd of n jittered and translated poses against the reference -> values of rmsd not bit-equal"""
    x = K.base(count)
    poses = K.jittered(x, n, 0.4, seed)
    rng = np.random.default_rng(seed + 1)
    poses = (poses + rng.uniform(-1.0, 1.0, (n, 1, 3)) * np.asarray(L if any(L) else (3.0, 3.0, 3.0))[None, None, :] * 0.7).astype(np.float32)
    T, D, r = driver_pairs(driver, driver_input(tmp_path / "in.bin", 0, poses, cut=1.25, mask=mask, perms=perms, L=L))
    n_m = len(R.masked_atoms(count, mask))
    Dr = R.distance(poses, None, mask, perms, L)
    assert T == R.threshold(1.25, n_m)
    assert np.array_equal(D.view(np.uint64), Dr.view(np.uint64)), f"D differs in {(D != Dr).sum()} of {D.size} pairs"
    u = ulps(r, R.rmsd_of(Dr, n_m))
    assert u.max() <= 1
    return int((u != 0).sum()), r.size


def test_the_distance_of_the_header_is_that_of_numpy(driver, tmp_path):
    """D and T bit for bit, rmsd within 1 fp32 ulp (the one rounding to fp32 behind an fp64 sqrt that two maths libraries may round
    differently in its last bit): counts 1, 12 and 50, with and without a mask, 0 / 1 / 2 / 12 perms, vacuum and a periodic box that
    the translations cross."""
    differ = total = 0
    L = K.periodic_edges()
    swap12 = np.stack([np.arange(12), np.r_[1, 0, np.arange(2, 12)]]).astype(np.uint32)
    for count, mask, perms in ((1, None, None), (1, None, np.zeros((1, 1), np.uint32)), (12, None, None), (12, None, swap12), (12, K.ring_mask(12), K.ring_perms(12)),
                               (50, None, K.ring_perms(50)), (50, K.ring_mask(50), None)):
        for box in ((0.0, 0.0, 0.0), tuple(L), (float(L[0]), 0.0, 0.0)):
            d, t = _pairs_case(count, 9, 40 + count, mask, perms, box, tmp_path, driver)
            differ, total = differ + d, total + t
    print(f"rmsd of the header against numpy: {differ} of {total} values not bit-equal")


def test_the_image_shift(driver, tmp_path):
    """A pose against its copies translated by +-L along every axis, and by 0.49 L and 0.51 L: the distance sees the nearest image of the
    centroid (0, and 0.49 L both times); in vacuum it sees the translation."""
    L = K.periodic_edges()
    x = K.base(12)
    shifts = [np.zeros(3)] + [sg * L * np.eye(3)[ax] for ax in range(3) for sg in (1.0, -1.0)] + [f * L * np.eye(3)[ax] for ax in range(3) for f in (0.49, 0.51)]
    poses = np.stack([x + s for s in shifts]).astype(np.float32)
    for box in (tuple(L), (0.0, 0.0, 0.0)):
        _, D, r = driver_pairs(driver, driver_input(tmp_path / "in.bin", 0, poses, L=box))
        assert np.array_equal(D.view(np.uint64), R.distance(poses, None, None, None, box).view(np.uint64))
        if any(box):
            assert (r[0, 1:7] < 1e-4).all(), r[0]
            assert np.allclose(r[0, 7::2], 0.49 * L, rtol=1e-5) and np.allclose(r[0, 8::2], 0.49 * L, rtol=1e-5), r[0, 7:]
        else:
            assert np.allclose(r[0, 1:7], np.repeat(L, 2), rtol=1e-6) and np.allclose(r[0, 8::2], 0.51 * L, rtol=1e-5)


CASES = K.clustering_cases()
RING_CASE = next(c for c in CASES if "12 perms and a mask" in c[0])


@pytest.mark.parametrize("case", [c for c in CASES if len(c[1]) <= 400], ids=lambda c: c[0])
def test_the_clustering_of_the_header_is_that_of_numpy(driver, tmp_path, case):
    """Leaders, cluster ids and sizes equal, rmsd_to_leader within 1 fp32 ulp - the smaller clustering cases of the GPU tests, on a
    periodic box"""
    name, poses, scores, cut, mask, perms = case
    L = K.periodic_edges()
    want = R.cluster(poses, scores, cut, mask, perms, L)
    got = driver_clusters(driver, driver_input(tmp_path / "in.bin", 1, poses, scores, cut, mask, perms, L))
    for a, b, what in zip(got, want, ("leaders", "cluster_of", "rmsd_to_leader", "sizes")):
        if what == "rmsd_to_leader":
            u = ulps(a, b)
            assert u.max() <= 1
            print(f"{name}: {int((u != 0).sum())} of {u.size} rmsd_to_leader values not bit-equal")
        else:
            assert np.array_equal(a, b), (name, what)
    assert int(got[3].sum()) == len(poses) and (got[2][got[0]] == 0.0).all()


def test_no_clustering_case_holds_a_pair_near_the_cutoff():
    """The condition on the inputs that the comparison of clusterings rests on, known to hold before a GPU is involved: cluster() of the
    reference asserts |D - T| / T > 1e-9 for every pair.  Also what the cases were built for."""
    L = K.periodic_edges()
    for case in CASES:
        name, poses, scores, cut, mask, perms = case
        for box in K.boxes_of(case):
            info = {}
            lead, cl, rm, sz = R.cluster(poses, scores, cut, mask, perms, box, info=info)
            print(f"{name}, box {box[0]:.0f}: {len(lead)} clusters of {sz.min()} - {sz.max()} members, smallest relative margin {info['margin']:.2e}")
            assert info["margin"] > R.MARGIN
            if name.startswith("families") or name.startswith("tied") or name.startswith("+inf"):
                assert len(lead) == 7, (name, len(lead))
            if name.startswith("continuum"):      # 130 steps of 0.66 A = 86 A of line, 30 A of it distinct in the periodic box
                width = 130 * 0.66 if not box[0] else K.BOX
                assert width / 4.0 - 1 <= len(lead) <= width / 2.0 + 1, len(lead)
            if name.startswith("duplicates"):
                assert len(lead) == 70 and sz.max() >= 2
    a, b = (R.cluster(*c[1:], L)[0] for c in CASES if c[0].startswith("continuum"))
    assert not np.array_equal(np.sort(a), np.sort(b)), "the continuum's leaders should depend on the score order"
    # without the ring's images the relabelled families fall apart
    name, poses, scores, cut, mask, perms = RING_CASE
    assert len(R.cluster(poses, scores, cut, mask, None, L)[0]) > 7


def test_the_driver_under_the_sanitizers(tmp_path):
    """The same stand-alone host program built with -fsanitize=address,undefined and run once in each mode"""
    exe = _compile(EXE + "_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    name, poses, scores, cut, mask, perms = RING_CASE
    L = K.periodic_edges()
    _, D, _ = driver_pairs(exe, driver_input(tmp_path / "a.bin", 0, poses[:8], cut=cut, mask=mask, perms=perms, L=L))
    assert D.shape == (8, 8)
    got = driver_clusters(exe, driver_input(tmp_path / "b.bin", 1, poses[:60], scores[:60], cut, mask, perms, L))
    assert int(got[3].sum()) == 60
    assert run_driver(exe, driver_input(tmp_path / "c.bin", 2, poses[:60], scores[:60], cut, mask, perms, L))[0].startswith("S ")


# ---- ligand_automorphisms ---------------------------------------------------------------------------------------------------------------
def _is_automorphism(p, n, bonds, keys):
    e = {frozenset(b) for b in bonds}
    return sorted(p.tolist()) == list(range(n)) and {frozenset((int(p[a]), int(p[b]))) for a, b in bonds} == e and all(keys[int(p[i])] == keys[i] for i in range(n))


def _closed(perms, masked):
    acts = {tuple(int(p[i]) for i in masked) for p in perms}
    slot = {int(a): k for k, a in enumerate(masked)}
    for p, q in itertools.product(perms, repeat=2):
        if tuple(int(p[int(q[i])]) for i in masked) not in acts:
            return False
    return all(set(a) == set(slot) for a in acts)


def test_automorphisms_of_known_graphs():
    from molchanica_amd.md_state import ParamError
    ring = ligand_automorphisms(6, K.RING, [0] * 6)
    assert ring.shape == (12, 6) and ring.dtype == np.uint32 and ring[0].tolist() == list(range(6))
    # toluene-like heavy atoms: the ring with a methyl carbon on atom 0
    tol_b = K.RING + [(0, 6)]
    tol = ligand_automorphisms(7, tol_b, [0] * 7)
    assert tol.shape == (2, 7) and tol[1].tolist() == [0, 5, 4, 3, 2, 1, 6]
    # a chain with distinct end keys
    chain_b = [(0, 1), (1, 2), (2, 3)]
    assert ligand_automorphisms(4, chain_b, [0, 1, 1, 2]).shape == (1, 4)
    assert ligand_automorphisms(4, chain_b, [0, 1, 1, 0]).shape == (2, 4)
    # a methyl group on a carbon: 3! images of the hydrogens, one with a heavy-atom mask
    me_b, me_k = [(0, 1), (0, 2), (0, 3), (0, 4)], [0, 1, 1, 1, 2]
    assert ligand_automorphisms(5, me_b, me_k).shape == (6, 5)
    heavy = ligand_automorphisms(5, me_b, me_k, mask=[1, 0, 0, 0, 1])
    assert heavy.shape == (1, 5) and heavy[0].tolist() == list(range(5))
    # toluene with its hydrogens, heavy-atom mask: the flip only
    full_b = tol_b + [(6, 7), (6, 8), (6, 9)] + [(i, 9 + i) for i in range(1, 6)]
    full_k = [0] * 7 + [1] * 8
    hm = np.array([1] * 7 + [0] * 8)
    assert ligand_automorphisms(15, full_b, full_k).shape == (12, 15)
    flip = ligand_automorphisms(15, full_b, full_k, mask=hm)
    assert flip.shape == (2, 15)
    # two tert-butyl groups on a bond: 2 x (3!)^2 = 72 images of the six methyl carbons - above a small cap, and above the default
    tb_b = [(0, 1)] + [(0, 2 + i) for i in range(3)] + [(1, 5 + i) for i in range(3)]
    for cap in (8, _abi.CLUSTER_MAX_PERMS):
        with pytest.raises(ParamError, match="cap"):
            ligand_automorphisms(8, tb_b, [0] * 8, cap=cap)
    assert ligand_automorphisms(8, tb_b, [0] * 8, cap=72).shape == (72, 8)
    for n, bonds, keys, mask, perms in ((6, K.RING, [0] * 6, None, ring), (7, tol_b, [0] * 7, None, tol), (15, full_b, full_k, hm, flip),
                                       (15, full_b, full_k, None, ligand_automorphisms(15, full_b, full_k)),
                                       (8, tb_b, [0] * 8, None, ligand_automorphisms(8, tb_b, [0] * 8, cap=72))):
        assert all(_is_automorphism(p, n, bonds, keys) for p in perms)
        assert _closed(perms, np.arange(n) if mask is None else np.flatnonzero(mask))
    for bad in (dict(keys=[0] * 5), dict(bonds=[(0, 6)]), dict(mask=[0] * 6), dict(mask=[1] * 5)):
        with pytest.raises(ParamError):
            ligand_automorphisms(**{**dict(n=6, bonds=K.RING, keys=[0] * 6), **bad})


def test_the_distance_is_symmetric_under_a_group(driver, tmp_path):
    """D(a, b) = D(b, a) bit for bit when the perms are a group: the ring's 12 images, 20 random pose pairs - in the reference and in the
    header.  With a set that is no group (the identity and one rotation of the ring) it is not."""
    rng = np.random.default_rng(5)
    x = K.base(12)[:6]
    P = ligand_automorphisms(6, K.RING, [0] * 6)
    pick = rng.integers(0, 12, 40)
    poses = np.stack([(x + rng.normal(0.0, 0.5, x.shape))[P[pick[i]]] for i in range(40)]).astype(np.float32)
    D = R.distance(poses, None, None, P)
    _, Dh, _ = driver_pairs(driver, driver_input(tmp_path / "in.bin", 0, poses, perms=P))
    assert np.array_equal(D.view(np.uint64), Dh.view(np.uint64))
    pairs = [(2 * i, 2 * i + 1) for i in range(20)]
    assert all(D[a, b] == D[b, a] for a, b in pairs), "D is not symmetric under the ring's group"
    rot = np.stack([np.arange(6), (np.arange(6) + 1) % 6]).astype(np.uint32)
    Dn = R.distance(poses, None, None, rot)
    assert any(Dn[a, b] != Dn[b, a] for a, b in pairs)
