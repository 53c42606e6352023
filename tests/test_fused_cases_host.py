"""The systems of tests/fused_cases.py, on the CPU: that they reach what they are built to reach in the fused bonded + kick + drift pass,
that the host mirror of the role and shape tables is the library's, and that a short window against the fp64 oracle (oracle/) can tell
one wrong parameter set from rounding - the conditions under which tests/test_gpu_fused_cases.py means something.

bound(n) = 4 ulp_f32(largest |coordinate|) n, the rounding rule of tests/test_gpu_restraints.py: 6.10e-5 A for n = 4, 1.22e-4 A for
n = 8 in these 49.65 A boxes.  Reaction field, dt = 0.0005 ps.  Figures of the resolving-power tests (largest displacement of an atom of
the oracle's result, in A and in bounds; FIGURES_BEGIN .. FIGURES_END is what the tests print):

FIGURES_BEGIN
mixed_solvent n = 4, bound(4) = 6.104e-05 A
  exchange bond_r0       terms   508   511  values 0.94244 0.97730  moved 1.805e-02 A =  295.7 bound  (asked 10)
  exchange bond_k        terms   508   509  values 444.57483 458.28522  moved 8.935e-04 A =   14.6 bound  (asked 10)
  exchange angle_theta0  terms     0     7  values 1.81566 1.77272  moved 5.741e-03 A =   94.1 bound  (asked 10)
  exchange angle_k       terms     0     1  values 84.24377 90.05544  moved 9.730e-04 A =   15.9 bound  (asked 4)
  water 1 with the parameters of water 2: moved 1.490e-03 A =   24.4 bound  (asked 10)
  start perturbed by 2e-6 A: moved 3.371e-06 A =   0.06 bound
chain_in_water n = 8, bound(8) = 1.221e-04 A
  no 1-4 pairs: moved 2.153e-02 A =  176.4 bound  (asked 10)
  every dihedral phase + pi: moved 2.476e-02 A =  202.8 bound  (asked 10)
FIGURES_END

The exchanges are between two terms of the same kind whose values differ by at least 2 %: the test asks 10 bound(4) of each but the angle
force constants, of which it asks 4 bound(4) (a 2 % difference of angle_k bends a water by too little in four steps).  Dihedrals and 1-4
pairs are resolved PER TERM KIND, not per term: one dihedral of this synthetic chain moves an atom by as little as 3e-7 A in eight steps,
so the window sees the whole 1-4 list missing or every phase turned by pi, not one wrong dihedral."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from molchanica_amd import MdConfig
from oracle import oracle
from tests import fused_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.0005
CFG = MdConfig(coulomb_mode=1)


@pytest.fixture(scope="module")
def mixed():
    s = K.mixed_solvent()
    tab = K.role_tables(s)
    return s, tab, K.triad_shapes(s, tab)


@pytest.fixture(scope="module")
def chain():
    s = K.chain_in_water()
    return s, K.role_tables(s)


def test_mixed_solvent_reaches_every_arm_of_the_triad_flavour(mixed):
    s, (off, rec, prm), tri = mixed
    n = s.n_atoms
    codes = tri["codes"]
    print("atoms", n, "roles per atom", off[-1] / n, "shapes", tri["n_shapes"], "max code", codes.max(), "parameter sets", prm.shape[0],
          "zero low byte", int(((codes > 0) & (codes & 0xFF == 0)).sum()), "code 0", int((codes == 0).sum()))
    assert (n, int(off[-1]), tri["n_shapes"], int(codes.max()), prm.shape[0]) == (12224, 30484, 12192, 12192, 13210)      # this seed's numbers, pinned
    assert tri["eligible"] and tri["n_shapes"] >= 4096 and codes.max() >= 4096
    assert ((codes > 0) & (codes & 0xFF == 0)).any()
    assert K.shape_combinations(tri) == K.ALL_COMBINATIONS
    free = (codes == 0) & K.mobile(s)
    assert free.sum() == K.N_IONS and free[0] and free[n - 1] and free[n // 2 - 64:n // 2 + 64].any()
    assert (np.diff(off)[free] == 0).all()
    assert (~K.mobile(s)).sum() == 3 * K.N_STATIC_WATERS == 24 and (np.asarray(s.vel)[~K.mobile(s)] == 0).all()
    assert off[-1] / n < K.ROLES_PER_SLOT_MAX
    for name in ("bond_k", "bond_r0", "angle_k", "angle_theta0"):      # f32-distinct: one parameter set per term
        v = getattr(s, name)
        assert np.unique(v).size == v.size, name


def test_the_other_two_systems_leave_the_triad_flavour(mixed, chain):
    s, _, tri = mixed
    s2, (h1, o2) = K.one_bond_too_many(s)
    off2, rec2, _ = K.role_tables(s2)
    assert not K.triad_shapes(s2, (off2, rec2, None))["eligible"]
    assert off2[h1 + 1] - off2[h1] == 4 > K.FUSED_PRE and off2[o2 + 1] - off2[o2] == 4
    assert off2[-1] / s2.n_atoms < K.ROLES_PER_SLOT_MAX and ((rec2[:, 3] & 0xF) <= K.KIND_ANGLE).all()      # still no dihedral role: the NODIH flavour
    c, (off3, rec3, _) = chain
    kinds = rec3[:, 3] & 0xF
    print("chain: atoms", c.n_atoms, "roles per atom", off3[-1] / c.n_atoms, "longest list", np.diff(off3).max(), "dihedral roles",
          int((kinds == K.KIND_DIHEDRAL).sum()), "1-4 roles", int((kinds == K.KIND_PAIR14).sum()))
    assert not K.triad_shapes(c, (off3, rec3, None))["eligible"]
    assert (kinds == K.KIND_DIHEDRAL).sum() == 4 * c.dihedral_idx.shape[0] > 0 and (kinds == K.KIND_PAIR14).sum() == 2 * c.pairs14_idx.shape[0] > 0
    assert off3[-1] / c.n_atoms < K.ROLES_PER_SLOT_MAX and np.diff(off3).max() > K.FUSED_PRE


def _triad_build(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path / "libhostutil.so")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_hostutil.cpp"), "-o", so])
    lib = C.CDLL(so)
    u32p = C.POINTER(C.c_uint32)
    fn = getattr(lib, "_Z15mdx_triad_buildPKjS0_mPjS1_jS1_")      # bool mdx_triad_build(const uint32_t*, const uint32_t*, size_t, uint32_t*, uint32_t*, uint32_t, uint32_t*)
    fn.argtypes = [u32p, u32p, C.c_size_t, u32p, u32p, C.c_uint32, u32p]
    fn.restype = C.c_bool
    return fn


def test_the_mirror_is_the_librarys_triad_build(mixed, chain, tmp_path):
    fn = _triad_build(tmp_path)
    u32p = C.POINTER(C.c_uint32)
    s = mixed[0]
    for system, tab in ((s, mixed[1]), (K.one_bond_too_many(s)[0], None), (chain[0], chain[1])):
        off, rec, _ = tab or K.role_tables(system)
        mine = K.triad_shapes(system, (off, rec, None))
        n = system.n_atoms
        off, rec = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(rec, np.uint32)
        tri, shapes, ns = np.full((n, 2), 0xDEADBEEF, np.uint32), np.zeros((65536, 4), np.uint32), C.c_uint32(7)
        ok = fn(off.ctypes.data_as(u32p), rec.ctypes.data_as(u32p), n, tri.ctypes.data_as(u32p), shapes.ctypes.data_as(u32p), 65536, C.byref(ns))
        assert bool(ok) == mine["eligible"] and ns.value == mine["n_shapes"], (system.name, ok, ns.value)
        if ok:
            assert np.array_equal(tri, mine["tri"])
            assert np.array_equal((tri[:, 0] >> 24) | ((tri[:, 1] >> 24) << 8), mine["codes"])
            assert np.array_equal(shapes[:ns.value + 1], mine["shapes"])


# ---- resolving power --------------------------------------------------------------------------------------------------------------------
def _moved(system, variant, n):
    x0, _, _ = oracle.step(system, CFG, DT, n, use_cells=True)
    x1, _, _ = oracle.step(variant, CFG, DT, n, use_cells=True)
    return np.abs(K.min_image(x1 - x0, system)).max(), x0


def _with(system, **arrays):
    v = copy.copy(system)
    for k, a in arrays.items():
        setattr(v, k, np.array(a))
    return v


def _plain_waters(s):
    ci = s.case_info
    static = set(ci["static_waters"].tolist())
    return [int(w) for w in ci["waters"] if int(w) not in static]


def _pair_differing(values, term_of, waters, rel=0.02):
    """the first plain water's term and that of the first later plain water whose value differs from it by >= rel -> two term indices"""
    a = term_of(waters[0])
    for w in waters[1:]:
        b = term_of(w)
        if abs(float(values[a]) - float(values[b])) >= rel * max(abs(float(values[a])), abs(float(values[b]))):
            return a, b
    raise AssertionError("no two terms differ")


def _swapped(values, a, b):
    v = np.array(values)
    v[[a, b]] = v[[b, a]]
    return v


def test_a_four_step_window_resolves_one_wrong_parameter_set(mixed):
    s = mixed[0]
    ci, waters = s.case_info, _plain_waters(s)
    b4 = K.bound(s, 4)
    assert b4 == 4 * 4 * 2.0 ** -18      # 6.10e-5 A: coordinates in [32, 64)
    base, _, _ = oracle.step(s, CFG, DT, 4, use_cells=True)
    print("FIGURES_BEGIN")
    print(f"mixed_solvent n = 4, bound(4) = {b4:.3e} A")
    for name, term_of, factor in (("bond_r0", lambda w: ci["bond_of"][w][0], 10.0), ("bond_k", lambda w: ci["bond_of"][w][0], 10.0),
                                  ("angle_theta0", lambda w: ci["angle_of"][w], 10.0), ("angle_k", lambda w: ci["angle_of"][w], 4.0)):
        values = getattr(s, name)
        a, b = _pair_differing(values, term_of, waters)
        x1, _, _ = oracle.step(_with(s, **{name: _swapped(values, a, b)}), CFG, DT, 4, use_cells=True)
        moved = np.abs(K.min_image(x1 - base, s)).max()
        print(f"  exchange {name:13s} terms {a:5d} {b:5d}  values {float(values[a]):.5f} {float(values[b]):.5f}  moved {moved:.3e} A = {moved / b4:6.1f} bound  (asked {factor:.0f})")
        assert moved >= factor * b4, (name, moved, b4)
    # one water carries the whole parameter set of another
    wa, wb = waters[0], waters[1]
    arrays = {k: np.array(getattr(s, k)) for k in ("bond_k", "bond_r0", "angle_k", "angle_theta0")}
    for k in ("bond_k", "bond_r0"):
        for j in range(2):
            arrays[k][ci["bond_of"][wa][j]] = getattr(s, k)[ci["bond_of"][wb][j]]
    for k in ("angle_k", "angle_theta0"):
        arrays[k][ci["angle_of"][wa]] = getattr(s, k)[ci["angle_of"][wb]]
    x1, _, _ = oracle.step(_with(s, **arrays), CFG, DT, 4, use_cells=True)
    moved = np.abs(K.min_image(x1 - base, s)).max()
    print(f"  water {wa} with the parameters of water {wb}: moved {moved:.3e} A = {moved / b4:6.1f} bound  (asked 10)")
    assert moved >= 10.0 * b4
    # ... and rounding of the start does not: 2e-6 A on every coordinate
    rng = np.random.default_rng(3)
    x1, _, _ = oracle.step(s, CFG, DT, 4, pos=np.asarray(s.pos, np.float64) + rng.uniform(-2e-6, 2e-6, (s.n_atoms, 3)) * K.mobile(s)[:, None], use_cells=True)
    moved = np.abs(K.min_image(x1 - base, s)).max()
    print(f"  start perturbed by 2e-6 A: moved {moved:.3e} A = {moved / b4:6.2f} bound")
    assert moved < 0.25 * b4


def test_an_eight_step_window_resolves_a_wrong_term_kind_on_the_chain(chain):
    """Per term kind, not per term (the module docstring): the whole 1-4 list, every dihedral phase."""
    c = chain[0]
    b8 = K.bound(c, 8)
    assert b8 == 4 * 8 * 2.0 ** -18
    base, _, _ = oracle.step(c, CFG, DT, 8, use_cells=True)
    print(f"chain_in_water n = 8, bound(8) = {b8:.3e} A")
    for what, v in (("no 1-4 pairs", _with(c, pairs14_idx=np.zeros((0, 2), np.uint32))),
                    ("every dihedral phase + pi", _with(c, dihedral_phase=(np.asarray(c.dihedral_phase, np.float64) + np.pi).astype(np.float32)))):
        x1, _, _ = oracle.step(v, CFG, DT, 8, use_cells=True)
        moved = np.abs(K.min_image(x1 - base, c)).max()
        print(f"  {what}: moved {moved:.3e} A = {moved / b8:6.1f} bound  (asked 10)")
        assert moved >= 10.0 * b8
    print("FIGURES_END")
