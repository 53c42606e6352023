"""`mdx_refine_guests_flex` without a GPU: the declaration and its mirrors, the layout of `mdx_guest_flex`, the refusals that are
decided before a device is touched, `GuestFlex.from_system` and `topology.rotatable_bonds` against the restatements of
tests/pose_flex_ref.py, the flexible additions to the chunk planner (molchanica_amd/csrc/mdx_pose_plan.h) as a stand-alone program,
plain and under the address and undefined-behaviour sanitizers, and the conditions under which tests/test_gpu_guest_flex.py means
something: its start poses keep the clash conditions tests/test_pose_flex_host.py pins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import GuestFlex, GuestLigand, _abi, systems, topology
from tests import guest_cases as gc
from tests import guest_flex_cases as fc
from tests import pose_flex_ref as F
from tests.test_gpu_pose_batch import MAX_DROPPED
from tests.test_pose_flex_host import INTRA_MIN, intra_excluded, ligand_case, min_intra_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    l.mdx_refine_guests_flex.argtypes = _abi.REFINE_GUESTS_FLEX_ARGTYPES
    return l


def test_header_declares_the_export_and_the_mirrors_follow():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mdx_refine_guests_flex\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_refine_guests_flex"
    args = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    assert args == ["mdx_handle*", "uint32_t", "const mdx_guest_ligand*", "const mdx_guest_flex*", "const mdx_flex_opts*", "float*", "float*",
                    "uint32_t", "float*", "float*", "float*", "float*", "uint32_t*", "uint32_t*", "uint32_t*", "double*"]
    assert len(_abi.REFINE_GUESTS_FLEX_ARGTYPES) == len(args) == 16
    assert _abi.REFINE_GUESTS_FLEX_ARGTYPES[3] == C.POINTER(_abi.CGuestFlex) and _abi.REFINE_GUESTS_FLEX_ARGTYPES[4] == C.POINTER(_abi.CFlexOpts)
    comment = src[src.index("guest ligands, flexible"):src.index("typedef struct mdx_guest_flex")]
    for must in ("bit for bit", "MDX_REFINE_NONFINITE", "never wins", "lowest ligand-local index", "OWN width", "writes nothing", "any size and order",
                 "MDX_FLEX_DIHEDRALS", "MDX_OVR_BONDED_DISABLED", "list order", "ring", "leaf", "not connected", "no counterpart for guests yet"):
        assert must in comment, must
    guests = src[src.index("guest ligands with gradients"):src.index("int      mdx_guest_forces")]
    assert "Not built for guests: torsional refinement" not in guests and "mdx_refine_guests_flex" in guests and "Not built for guests: the pose" in guests
    hpp = open(os.path.join(ROOT, "include", "mdx.hpp")).read()
    assert re.search(r"\brefine_guests_flex\s*\(", hpp) and "mdx_refine_guests_flex(h_" in hpp
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    blk = blk[:blk.index("\n}\n")]
    assert "pub fn mdx_refine_guests_flex" in blk and "pub struct MdxGuestFlex" in txt
    from tests.test_abi import declared_symbols
    from tests.test_abi import test_every_export_is_bound_or_listed as held
    assert f"({len(declared_symbols())} exports)" in open(os.path.join(ROOT, "README.md")).read()
    held()


def test_guest_flex_struct_layout_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "mdx.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mdx_guest_flex), offsetof(mdx_guest_flex, bonds), offsetof(mdx_guest_flex, root),
         offsetof(mdx_guest_flex, n_torsions), offsetof(mdx_guest_flex, torsion_bonds), offsetof(mdx_guest_flex, n_dihedrals),
         offsetof(mdx_guest_flex, dihedral_idx), offsetof(mdx_guest_flex, dihedral_v), offsetof(mdx_guest_flex, dihedral_phase),
         offsetof(mdx_guest_flex, dihedral_n));
  return 0;
}
''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    f = _abi.CGuestFlex
    assert got == [C.sizeof(f)] + [getattr(f, n).offset for n in ("bonds", "root", "n_torsions", "torsion_bonds", "n_dihedrals", "dihedral_idx",
                                                                   "dihedral_v", "dihedral_phase", "dihedral_n")]


# ---- refusals decided on the arguments alone -------------------------------------------------------------------------------------------------
def test_the_library_exports_it_and_refuses_on_the_arguments_alone(lib):
    fp, up, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    out = [np.full(64, -7.0, np.float32) for _ in range(6)]
    st, ev, bp = (np.full(2, 77, np.uint32) for _ in range(3))
    bs = np.full(2, -7.0, np.float64)
    p = lambda a: a.ctypes.data_as(fp)
    u = lambda a: a.ctypes.data_as(up)
    recs = (_abi.CGuestLigand * 1)()
    frecs = (_abi.CGuestFlex * 1)()
    good = _abi.CFlexOpts(12, 0.1, 0.1, 0.1, 0.0, 0.0, 1)

    def call(h, n, ligs, flex, opts):
        return lib.mdx_refine_guests_flex(h, n, ligs, flex, None if opts is None else C.byref(opts), p(out[0]), p(out[1]), 2, p(out[2]), p(out[3]),
                                          p(out[4]), p(out[5]), u(st), u(ev), u(bp), bs.ctypes.data_as(dp))
    assert call(None, 1, recs, frecs, good) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    fake = C.create_string_buffer(64)      # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    h = C.addressof(fake)
    for args in ((h, 1, None, frecs, good), (h, 1, recs, None, good), (h, 1, recs, frecs, None)):
        assert call(*args) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    for bad, match in ((_abi.CFlexOpts(0, 0.1, 0.1, 0.1, 0, 0, 0), b"max_evals"), (_abi.CFlexOpts(_abi.REFINE_MAX_EVALS_CAP + 1, 0.1, 0.1, 0.1, 0, 0, 0), b"max_evals"),
                       (_abi.CFlexOpts(12, 0.1, 0.1, -0.1, 0, 0, 0), b"negative"), (_abi.CFlexOpts(12, 0.1, 0.1, float("nan"), 0, 0, 0), b"not finite"),
                       (_abi.CFlexOpts(12, 0.1, 0.1, 0.1, 0.3, 0.25, 0), b"h_start"), (_abi.CFlexOpts(12, 0.1, 0.1, 0.1, 0, 0, 2), b"unknown flag")):
        assert call(h, 1, recs, frecs, bad) == _abi.MDX_EPARAM
        assert match in lib.mdx_last_error() and b"mdx_refine_guests_flex" in lib.mdx_last_error(), lib.mdx_last_error()
    assert all((o == -7.0).all() for o in out) and (st == 77).all() and (ev == 77).all() and (bp == 77).all() and (bs == -7.0).all()
    assert lib.mdx_refine_guests_flex(h, 0, None, None, None, None, None, 2, None, None, None, None, None, None, None, None) == 0


def test_python_wrapper_validates_the_flexible_records():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    lig = GuestLigand(np.zeros(4), np.ones(4), np.ones(4))
    chain = np.array([[0, 1], [1, 2], [2, 3]], np.uint32)
    for bad in ([], [dict(bonds=chain)], [GuestFlex(bonds=np.zeros(5, np.uint32))], [GuestFlex(bonds=chain, root=4)],
                [GuestFlex(bonds=chain, torsion_bonds=np.array([[1.5, 2.0]]))], [GuestFlex(bonds=chain, torsion_bonds=np.array([[-1, 2]]))],
                [GuestFlex(bonds=chain, torsion_bonds=np.tile(np.array([[1, 2]], np.uint32), (33, 1)))],
                [GuestFlex(bonds=chain, dihedral_idx=np.array([[0, 1, 2, 3]], np.uint32), dihedral_v=np.ones(2), dihedral_phase=np.zeros(1),
                           dihedral_n=np.ones(1, np.int32))]):
        with pytest.raises(ParamError, match="refine_guests_flex"):
            md.refine_guests_flex([lig], bad, 12, 0.1, 0.1, 0.1)
    with pytest.raises(ParamError, match="refine_guests_flex"):
        md.refine_guests_flex([dict()], [GuestFlex()], 12, 0.1, 0.1, 0.1)


# ---- GuestFlex.from_system and topology.rotatable_bonds ----------------------------------------------------------------------------------------
def test_from_system_reproduces_the_ligand_case():
    s, lo, hi, bonds, tb, tors, terms = ligand_case()
    fx = GuestFlex.from_system(s, lo, hi)
    assert fx.root == 0 and fx.bonds.dtype == np.uint32 and np.array_equal(fx.bonds, bonds)
    assert fx.n_torsions == 31 and np.array_equal(fx.torsion_bonds, tb)
    at, v, phase, n = fc.terms_of(fx)
    assert len(at) > 0 and np.array_equal(at, terms[0]) and np.array_equal(v, terms[1]) and np.array_equal(phase, terms[2]) and np.array_equal(n, terms[3])
    assert fx.dihedral_n.dtype == np.int32 and fx.dihedral_v.dtype == np.float32
    sub = GuestFlex.from_system(s, lo, hi, 0, tb[fc.SUBSET])
    assert np.array_equal(sub.torsion_bonds, tb[fc.SUBSET]) and np.array_equal(sub.dihedral_idx, fx.dihedral_idx)
    # a range that cuts through a molecule's dihedral terms is refused; so is one outside the system
    with pytest.raises(ValueError, match="dihedral"):
        GuestFlex.from_system(s, lo, hi - 1)
    with pytest.raises(ValueError, match="bounds"):
        GuestFlex.from_system(s, lo, s.n_atoms + 1)
    # more than 32 rotatable bonds: the first 32
    big = systems.lig50(31, 256)
    all_ = topology.rotatable_bonds(256, F.local_bonds(big, 0, 256), 0)
    assert len(all_) > 32 and np.array_equal(GuestFlex.from_system(big, 0, 256).torsion_bonds, all_[:32])


@pytest.mark.parametrize("n", [4, 9, 50, 256])
def test_rotatable_bonds_are_those_of_the_restatement(n):
    s = systems.lig50(31, n)
    bonds = F.local_bonds(s, 0, n)
    for root in (0, n - 1):
        mine, ref = topology.rotatable_bonds(n, bonds, root), F.rotatable_bonds(n, bonds, root)
        assert mine.dtype == np.uint32 and mine.shape == ref.shape and np.array_equal(mine, ref), (n, root)
        F.moving_sides(n, bonds, root, mine)      # (every one of them is accepted as a torsion)
    assert len(topology.rotatable_bonds(n, bonds, 0)) >= 1
    ring = np.array([[0, 1], [1, 2], [2, 0], [2, 3]], np.uint32)      # a ring with a leaf: nothing turns
    assert topology.rotatable_bonds(4, ring, 0).shape == (0, 2) and F.rotatable_bonds(4, ring, 0).shape == (0, 2)
    assert topology.rotatable_bonds(4, bonds[:1], 0).shape == (0, 2) if n == 4 else True      # (a disconnected graph has none)
    assert topology.rotatable_bonds(n, bonds, n).shape == (0, 2)


# ---- the planner's flexible additions as a stand-alone program ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan_driver(request, tmp_path_factory):
    """tests/cpp/guest_flex_plan_driver.cpp, built plain and with the address and undefined-behaviour sanitizers"""
    exe = tmp_path_factory.mktemp("guest_flex_plan_" + request.param) / "guest_flex_plan_driver"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + extra + ["-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                                                                      os.path.join(ROOT, "tests", "cpp", "guest_flex_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def _plan(exe, shapes):
    text = f"{len(shapes)}\n" + "\n".join(" ".join(str(v) for v in s) for s in shapes) + "\n"
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    lines = run.stdout.decode().splitlines()
    assert run.returncode == 0 and lines and lines[0].split()[0] == "ok", (run.stdout.decode(), run.stderr.decode()[-2000:])
    head = lines[0].split()
    return int(head[1]), int(head[2]), int(head[3]), [[int(v) for v in l.split()[3:]] for l in lines[1:]]


def test_planner_lays_out_the_mixed_library(plan_driver):
    """The driver checks per chunk: table offsets disjoint and 16-byte aligned, the poses' eterm stretches disjoint and summing to the
    chunk's total, every record its ligand's.  Here: the chunks are those expected, and the straddling ligand's tables are in both."""
    env, groups, ligs, flex = fc.mixed_flex_case()
    shapes = [(l.count, l.n_poses, len(l.pairs14), f.n_torsions, len(f.dihedral_idx)) for l, f in zip(ligs, flex)]
    n_chunks, total, largest, held = _plan(plan_driver, shapes)
    assert (n_chunks, total) == (2, sum(l.n_poses for l in ligs)) and total == 318
    assert held[0] == [0, 1, 3, 4, 5, 6, 7] and held[1] == [7, 8, 9, 10], held      # (ligand 2 is empty; ligand 7 straddles pose 256)
    terms = sum(len(f.dihedral_idx) * l.n_poses for l, f in zip(ligs, flex))
    assert largest >= 8 * 13 * terms // 2


@pytest.mark.parametrize("shapes,n_chunks", [
    ([(5, 1, 0, 0, 0)], 1), ([(4, 257, 1, 1, 1)], 2), ([(256, 256, 40, 32, 449)], 1), ([(3, 0, 0, 0, 0), (256, 0, 0, 32, 9)], 0),
    ([(7, 100, 1, 2, 5), (64, 600, 2, 32, 111), (9, 30, 0, 3, 0)], 3), ([(4, 256, 0, 1, 3), (6, 0, 2, 2, 7), (5, 3, 1, 0, 1)], 2)])
def test_planner_at_other_shapes(plan_driver, shapes, n_chunks):
    assert _plan(plan_driver, shapes)[:2] == (n_chunks, sum(s[1] for s in shapes))


# ---- the conditions of the GPU tests ---------------------------------------------------------------------------------------------------------
def test_the_start_poses_are_those_whose_clash_conditions_are_pinned(orc):
    """tests/test_gpu_guest_flex.py refines the 16 start poses of tests/test_pose_flex_host.py as a guest of R.  R is S without its
    ligand, atom for atom and bit for bit, so R plus a pose of the guest is S with that pose: the distances to the environment are the
    same numbers, and what test_the_start_poses_keep_their_conditions asserts of them (at most MAX_DROPPED of 16 closer than 1.0 A to the
    environment, none within 0.02 A of that rule's edge, no unexcluded intra-ligand pair below 1.6 A - before and after 12 evaluations)
    holds for the guest.  Asserted here for the starts, with R as the environment."""
    S, R, gR, (lo, hi), lig, tb = fc.small_flex_case()
    s, lo2, hi2, bonds, tb2, tors, terms = ligand_case()
    pos = orc.wrap(S, S.pos)
    assert np.array_equal(np.delete(np.asarray(S.pos), np.s_[lo:hi], 0), np.asarray(R.pos)) and R.n_atoms == S.n_atoms - (hi - lo)
    assert np.array_equal(np.asarray(S.box_lo), np.asarray(R.box_lo)) and np.array_equal(np.asarray(S.box_hi), np.asarray(R.box_hi))
    from tests.test_pose_flex_host import start_poses
    from tests.test_gpu_pose_batch import min_env_distance
    assert np.array_equal(lig.poses, start_poses(S, pos, lo, hi, tors)) and lig.poses.shape == (16, hi - lo, 3) and np.array_equal(tb, tb2)
    d = gc.min_distance(R, np.delete(pos, np.s_[lo:hi], 0), lig.poses)
    assert np.array_equal(d, min_env_distance(S, pos, lo, hi, lig.poses)), "the same geometry: the same distances"
    it = min_intra_distance(intra_excluded(S, lo, hi), lig.poses)
    print(f"starts: {(d < 1.0).sum()} closer than 1.0 A, closest to the rule's edge {np.abs(d - 1.0).min():.3f} A, closest intra-ligand pair {it.min():.3f} A")
    assert (d < 1.0).sum() <= MAX_DROPPED and np.abs(d - 1.0).min() >= 0.02 and it.min() >= INTRA_MIN
    # the chain added to the mixed library lies clear of the water, as the library's other ligands do
    env, groups, ligs, flex = fc.mixed_flex_case()
    assert gc.min_distance(env, env.pos, ligs[-1].poses).min() >= gc.CLEARANCE and flex[-1].n_torsions == 1 and len(flex[-1].dihedral_idx) == 1
