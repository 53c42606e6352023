"""`mdx_screen_ligands` without a GPU: the declaration and its mirrors, the argument checks that run before a device is touched, the
helpers of tests/guest_cases.py against the fp64 oracle, `GuestLigand.from_system`, and the conditions under which
tests/test_gpu_guest_screen.py means something (clash cap of the small complex, clearance of the mixed library)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import GuestLigand, MdConfig, _abi, systems
from tests import guest_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")
INTERNAL = ("bond", "angle", "dihedral", "lj14", "coulomb14")
t = gc.pose_batch_module()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    l.mdx_screen_ligands.argtypes = _abi.SCREEN_LIGANDS_ARGTYPES
    return l


def test_header_declares_the_export_and_its_mirrors():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+mdx_screen_ligands\s*\(\s*mdx_handle\s*\*", code) and "} mdx_guest_ligand;" in code
    assert "mdx_screen_ligands" in open(os.path.join(ROOT, "include", "mdx.hpp")).read()
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    assert "pub fn mdx_screen_ligands" in blk[:blk.index("\n}\n")] and "pub struct MdxGuestLigand" in txt


def test_guest_struct_layout_matches_c(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mdx.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mdx_guest_ligand), offsetof(mdx_guest_ligand, charge), offsetof(mdx_guest_ligand, n_excl),
         offsetof(mdx_guest_ligand, pairs14), offsetof(mdx_guest_ligand, n_poses), offsetof(mdx_guest_ligand, poses));
  return 0; }
'''
    src = tmp_path / "t.c"
    src.write_text(prog)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    G = _abi.CGuestLigand
    assert vals == [C.sizeof(G), G.charge.offset, G.n_excl.offset, G.pairs14.offset, G.n_poses.offset, G.poses.offset]


def test_null_arguments_are_rejected_before_any_device_is_touched(lib):
    out = np.full((2, 3), -7.0, np.float32)
    fp = C.POINTER(C.c_float)
    recs = (_abi.CGuestLigand * 1)()
    assert lib.mdx_screen_ligands(None, 1, recs, out.ctypes.data_as(fp), 2, None, None) == _abi.MDX_EPARAM
    assert b"null" in lib.mdx_last_error()
    assert lib.mdx_screen_ligands(None, 0, None, None, 2, None, None) == _abi.MDX_EPARAM
    assert (out == -7.0).all()


def test_python_wrapper_validates_before_the_library_is_asked():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)
    md._h = C.c_void_p()
    md.n_atoms = 100
    ok = dict(charge=np.zeros(4), lj_sigma=np.ones(4), lj_eps=np.ones(4))
    for bad in ([dict(ok)],                                                                    # not GuestLigand objects
                [GuestLigand(np.zeros(0), np.zeros(0), np.zeros(0))],                          # empty ligand
                [GuestLigand(np.zeros(257), np.zeros(257), np.zeros(257))],                    # above MDX_POSE_MAX_ATOMS
                [GuestLigand(np.zeros(4), np.ones(3), np.ones(4))],                            # sigma of another length
                [GuestLigand(**ok, excl_pairs=np.zeros((2, 3), np.uint32))],                   # not pairs
                [GuestLigand(**ok, poses=np.zeros((2, 5, 3), np.float32))]):                   # poses of another ligand
        with pytest.raises(ParamError):
            md.screen_ligands(bad)


def internal(orc, s):
    _, e = orc.forces(s, MdConfig(lj_cutoff=9.0, coulomb_cutoff=9.0, skin=1.5))
    return np.array([e[k] for k in INTERNAL])


def test_without_molecules_and_carve_keep_the_internal_terms(orc):
    """Bond, angle, dihedral and 1-4 energies are sums over molecules: those of the kept and of the dropped molecules add up to the
    whole system's, term by term - a wrongly remapped index array moves them."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    whole, kept, dropped = internal(orc, S), internal(orc, R), internal(orc, gc.only_molecules(S, [1]))
    print("internal terms", dict(zip(INTERNAL, whole)), "kept", kept, "dropped", dropped)
    assert np.all(np.abs(dropped[[0, 1, 2]]) > 1e-3) and np.all(np.abs(kept[:3]) > 1e-3)
    assert np.allclose(kept + dropped, whole, rtol=1e-10, atol=1e-8)
    assert R.n_atoms == S.n_atoms - (hi - lo) and len(R.mol_start) == len(S.mol_start) - 1 and int(R.mol_start[1]) == lo
    # the receptor - solvent element does not know whether the ligand is there
    cfg = t.small_configs()[0]
    ms, _ = orc.between_mols(S, cfg, t.three_groups(S), 3, use_cells=True)
    mr, _ = orc.between_mols(R, cfg, gR, 2, use_cells=True)
    assert np.allclose([mr[0, 0], mr[0, 1], mr[1, 1]], [ms[0, 0], ms[0, 2], ms[2, 2]], rtol=1e-10, atol=1e-8)
    # carve: waters around the ligand's atoms leave, nothing else does
    pts = np.asarray(S.pos, np.float64)[lo:hi]
    gone = gc.carved_molecules(S, pts, 4.0)
    assert len(gone) > 5 and gone.min() >= 2
    C_ = gc.carve(S, pts, 4.0)
    assert C_.n_atoms == S.n_atoms - 3 * len(gone)
    assert np.allclose(internal(orc, C_) + internal(orc, gc.only_molecules(S, gone)), whole, rtol=1e-10, atol=1e-8)
    assert t.min_env_distance(C_, np.concatenate([C_.pos[:lo], C_.pos[hi:]]), C_.n_atoms - (hi - lo), C_.n_atoms - (hi - lo), pts[None] if False else [pts]).min() >= 0.0
    d = np.linalg.norm(np.asarray(C_.pos, np.float64)[hi:, None, :] - pts[None], axis=2).min()
    assert d >= 4.0 - 1e-6


def class_map(n, excl, p14):
    m = np.zeros((n, n), np.uint8)
    for a, b in np.asarray(excl, np.int64).reshape(-1, 2):
        m[a, b] = m[b, a] = 1
    for a, b in np.asarray(p14, np.int64).reshape(-1, 2):
        m[a, b] = m[b, a] = 2
    return m


def test_from_system_round_trips_exclusions_and_pairs14():
    S, R, gR, (lo, hi), lig = gc.small_case()
    n = hi - lo
    assert lig.count == n and lig.excl_pairs.dtype == np.uint32 and lig.pairs14.dtype == np.uint32
    # the map mdx_create makes of the molecule: the CSR, then the 1-4 pairs over it
    off = S.excl_offsets.astype(np.int64)
    want = np.zeros((n, n), np.uint8)
    for i in range(lo, hi):
        for j in S.excl_idx[off[i]:off[i + 1]]:
            assert lo <= j < hi
            want[i - lo, j - lo] = 1
    inside = [(a - lo, b - lo) for a, b in S.pairs14_idx.astype(np.int64) if lo <= a < hi]
    for a, b in inside:
        want[a, b] = want[b, a] = 2
    assert np.array_equal(class_map(n, lig.excl_pairs, lig.pairs14), want) and (want == 1).any() and (want == 2).any()
    assert len(lig.pairs14) == len(inside) and (lig.excl_pairs[:, 0] < lig.excl_pairs[:, 1]).all()
    t_ = S.lj_type[lo:hi]
    assert np.array_equal(lig.lj_sigma, S.lj_sigma[t_]) and np.array_equal(lig.lj_eps, S.lj_eps[t_]) and np.array_equal(lig.charge, S.charge[lo:hi])
    with pytest.raises(ValueError):
        GuestLigand.from_system(S, lo, hi - 3)      # bonds and exclusions cross the cut
    # a molecule of its own system, and the system put together again gives back the same lists
    g = systems.lig50(seed=2)
    gl = GuestLigand.from_system(g, 0, g.n_atoms)
    both = gc.concat_systems([gc.only_molecules(S, [0]), g], S)
    gl2 = GuestLigand.from_system(both, int(both.mol_start[1]), both.n_atoms)
    assert np.array_equal(gl.excl_pairs, gl2.excl_pairs) and np.array_equal(gl.pairs14, gl2.pairs14)
    assert np.array_equal(gl.lj_sigma, gl2.lj_sigma) and np.array_equal(gl.lj_eps, gl2.lj_eps)


def test_small_complex_poses_stay_within_the_clash_cap(orc):
    """Tests 1, 2 and 6 of the GPU file drop at most 2 of 16 poses: the environment, the start and the seed are those of the
    resident-pose test."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    pos = orc.wrap(S, S.pos)
    poses = t.rigid_poses(t.whole(S, pos[lo:hi]), 16, t.SEED_SMALL)
    d = gc.min_distance(R, orc.wrap(R, R.pos), poses)
    d_res = t.min_env_distance(S, pos, lo, hi, poses)
    print("guest on R", np.round(np.sort(d)[:4], 3))
    assert np.allclose(d, d_res), "R is S without its ligand"
    assert (d < 1.0).sum() <= t.MAX_DROPPED
    assert not np.any(np.abs(d - 1.0) < 0.02), "a pose on the edge of the rule: fp32 positions on the device may flip it"


def test_mixed_library_is_clear_of_its_environment():
    env, groups, gs, ligs = gc.mixed_case()
    assert [l.count for l in ligs] == [1, 2, 7, 7, 8, 9, 50, 64, 65, 256]
    counts = [l.n_poses for l in ligs]
    assert tuple(counts) == gc.MIXED_POSES and sum(counts) > 256 and 0 in counts
    edges = np.cumsum([0] + counts)
    assert any(a < 256 < b for a, b in zip(edges[:-1], edges[1:])), "one ligand's poses straddle the chunk boundary"
    assert env.periodic and env.n_atoms % 3 == 0 and env.n_atoms > 900
    assert set(groups.tolist()) == {0, 1} and np.all(groups[0::3] == groups[2::3]) and groups[0] != groups[3]
    for l in ligs:
        if l.n_poses == 0:
            continue
        d = gc.min_distance(env, env.pos, l.poses)
        print(f"{l.count} atoms: closest water atom {d.min():.3f} .. {d.max():.3f} A")
        assert d.min() >= gc.CLEARANCE, "every guest - environment distance is at least 1.5 A"
        assert d.max() < 6.0, "every pose has water within the cutoff"


def test_combined_oracle_row_does_not_depend_on_where_the_guest_is_appended(orc):
    env, groups, gs, ligs = gc.mixed_case()
    cfg = t.small_configs()[1]
    for m in (0, 4, 6):
        pose = ligs[m].poses[1]
        back, gb = gc.guest_oracle_row(orc, env, groups, env.pos, gs[m], pose, cfg)
        front, gf = gc.guest_oracle_row(orc, env, groups, env.pos, gs[m], pose, cfg, front=True)
        print(f"ligand {m}: appended {back} put first {front}")
        assert np.allclose(back, front, rtol=1e-11, atol=1e-9) and np.allclose(gb, gf, rtol=1e-11, atol=1e-9)
        assert np.abs(back[:2]).max() > 1e-3
    S, R, gR, (lo, hi), lig = gc.small_case()
    pos = np.asarray(S.pos, np.float64)
    ro, gr = t.oracle_row(orc, S, cfg, t.three_groups(S), 3, pos, lo, hi, pos[lo:hi], 1)
    mine, gm = gc.guest_oracle_row(orc, R, gR, np.delete(pos, np.s_[lo:hi], 0), gc.only_molecules(S, [1]), pos[lo:hi], cfg)
    assert np.allclose(mine, ro[[0, 2, 1]], rtol=1e-11, atol=1e-9) and np.allclose(gm, gr[[0, 2, 1]], rtol=1e-11, atol=1e-9)
