"""`mdx_search_guests` without a GPU: the declaration and its mirrors, the two header sentences that used to say the search was not
built, the refusals that are decided before a device is touched, the Python wrapper's own checks, and the search block of the chunk
planner (molchanica_amd/csrc/mdx_pose_plan.h: SearchLayout, GUEST_SEARCH) as a stand-alone program, plain and under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import GuestFlex, GuestLigand, _abi
from tests import guest_flex_cases as fc
from tests import guest_search_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    l.mdx_search_guests.argtypes = _abi.SEARCH_GUESTS_ARGTYPES
    return l


def test_header_declares_the_export_and_the_mirrors_follow():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mdx_search_guests\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_search_guests"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["mdx_handle* h", "uint32_t n_ligands", "const mdx_guest_ligand* ligs", "const mdx_guest_flex* flex", "const uint64_t* streams_or_null",
                    "const mdx_search_opts* opts", "float* best_out", "float* best_rows_out_or_null", "uint32_t n_groups",
                    "double* best_score_out_or_null", "float* best_dih_out_or_null", "uint32_t* best_round_out_or_null", "uint32_t* stats_out_or_null",
                    "uint32_t* best_walker_or_null", "double* best_ligand_score_or_null"]
    at = _abi.SEARCH_GUESTS_ARGTYPES
    assert len(at) == len(args) == 15
    assert at[3] == C.POINTER(_abi.CGuestFlex) and at[4] == C.POINTER(C.c_uint64) and at[5] == C.POINTER(_abi.CSearchOpts)
    assert at[9] == at[14] == C.POINTER(C.c_double) and at[8] == C.c_uint32
    comment = src[src.index("guest ligands, pose search"):src.index("int      mdx_search_guests")]
    for must in ("bit for bit", "word for word", "LIGAND-LOCAL", "any size and order", "lowest ligand-local index", "never wins", "0xFFFFFFFF",
                 "writes nothing", "one upload", "n_rounds x (1 + 2 max_evals) + 1 launches plus the pick", "one read-back and one wait",
                 "MDX_SEARCH_MAX_ROUNDS", "65536", "tors_amp > pi", "no move enabled", "mdx_cluster_poses", "n_rounds == 1"):
        assert must in comment, must
    hpp = open(os.path.join(ROOT, "include", "mdx.hpp")).read()
    assert re.search(r"\bsearch_guests\s*\(", hpp) and "mdx_search_guests(h_" in hpp
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    blk = blk[:blk.index("\n}\n")]
    assert "pub fn mdx_search_guests" in blk
    from tests.test_abi import declared_symbols
    from tests.test_abi import test_every_export_is_bound_or_listed as held
    assert "mdx_search_guests" in declared_symbols()
    assert f"({len(declared_symbols())} exports)" in open(os.path.join(ROOT, "README.md")).read()
    held()


def test_the_two_sentences_no_longer_say_the_search_is_missing():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    flat = lambda s: re.sub(r"\s*\n \* ", " ", s)
    guests = flat(src[src.index("guest ligands with gradients"):src.index("int      mdx_guest_forces")])
    flexible = flat(src[src.index("guest ligands, flexible"):src.index("typedef struct mdx_guest_flex")])
    for block in (guests, flexible):
        assert "mdx_search_guests" in block
    assert "the pose search (mdx_search_poses for a library)" not in guests
    assert "mdx_search_poses has no counterpart for guests yet." not in flexible
    assert "had no counterpart for guests yet; it is mdx_search_guests" in flexible
    for name in ("DESIGN.md", "INTEGRATION.md"):
        txt = open(os.path.join(ROOT, name)).read()
        assert "Not built: the pose search for guests" not in txt and "search for guests are not built" not in txt, name
        assert "(`mdx_search_poses` for a library) is not built" not in txt, name


# ---- refusals decided on the arguments alone -------------------------------------------------------------------------------------------------
def test_the_library_exports_it_and_refuses_on_the_arguments_alone(lib):
    o, clean = sc.preset_outputs(2, 64, 3, 2)
    recs = (_abi.CGuestLigand * 1)()
    frecs = (_abi.CGuestFlex * 1)()
    good = sc.search_opts(2, evals=12)
    assert sc.raw_search(lib, None, 1, recs, frecs, good, o, 2)[0] == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    fake = C.create_string_buffer(64)      # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    h = C.addressof(fake)
    for args in ((None, frecs, good), (recs, None, good), (recs, frecs, None)):
        rc, msg = sc.raw_search(lib, h, 1, args[0], args[1], args[2], o, 2)
        assert rc == _abi.MDX_EPARAM and "null" in msg and "mdx_search_guests" in msg, msg
    nan, pi32 = float("nan"), float(np.nextafter(np.float32(math.pi), np.float32(4.0)))
    for bad, match in ((sc.search_opts(0), "n_rounds"), (sc.search_opts(_abi.SEARCH_MAX_ROUNDS + 1, evals=1), "n_rounds"),
                       (sc.search_opts(1024, evals=65), "65536"), (sc.search_opts(17, evals=4096), "65536"),
                       (sc.search_opts(moves=(-0.5, 0.1, 0.1)), "negative"), (sc.search_opts(moves=(0.5, nan, 0.1)), "not finite"),
                       (sc.search_opts(moves=(0.5, 0.1, -1.0)), "negative"), (sc.search_opts(kT=-1.0), "negative"), (sc.search_opts(kT=nan), "not finite"),
                       (sc.search_opts(moves=(0.5, 0.1, float("inf"))), "not finite"), (sc.search_opts(moves=(0.5, 0.1, pi32)), "tors_amp exceeds pi"),
                       (sc.search_opts(moves=(0.0, 0.0, 0.0)), "no move is enabled"),
                       (sc.search_opts(evals=0), "max_evals"), (sc.search_opts(tors_tol=-0.1), "negative"), (sc.search_opts(h_start=0.3, h_max=0.25), "h_start"),
                       (sc.search_opts(flags=2), "unknown flag")):
        rc, msg = sc.raw_search(lib, h, 1, recs, frecs, bad, o, 2)
        assert rc == _abi.MDX_EPARAM and match in msg and "mdx_search_guests" in msg, (match, msg)
    assert clean(), "a refused mdx_search_guests must leave every output untouched"
    assert lib.mdx_search_guests(h, 0, None, None, None, None, None, None, 2, None, None, None, None, None, None) == 0
    assert clean()


def test_python_wrapper_validates_before_the_library_is_asked():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    chain = np.array([[0, 1], [1, 2], [2, 3]], np.uint32)
    poses = np.zeros((3, 4, 3), np.float32)
    lig = GuestLigand(np.zeros(4), np.ones(4), np.ones(4), poses=poses)
    fx = GuestFlex(bonds=chain, torsion_bonds=np.array([[1, 2]], np.uint32))
    rigid = GuestFlex(bonds=chain)
    ok = dict(n_rounds=3, trans_amp=0.5, rot_amp=0.1, tors_amp=0.4, kT=1.0, seed=7, max_evals=4, f_tol=0.0, tau_tol=0.0, tors_tol=0.0)
    for flex in ([], [dict(bonds=chain)], [GuestFlex(bonds=chain, root=4)]):
        with pytest.raises(ParamError, match="search_guests"):
            md.search_guests([lig], flex, **ok)
    with pytest.raises(ParamError, match="search_guests"):
        md.search_guests([dict()], [fx], **ok)
    for change in (dict(n_rounds=0), dict(n_rounds=1025), dict(n_rounds=1024, max_evals=65), dict(max_evals=0), dict(trans_amp=-1.0),
                   dict(rot_amp=float("nan")), dict(kT=-1.0), dict(tors_amp=3.2), dict(trans_amp=0.0, rot_amp=0.0, tors_amp=0.0), dict(seed=1 << 64),
                   dict(seed=-1), dict(streams=np.arange(2)), dict(streams=np.array([0.5, 1, 2])), dict(streams=np.array([0, -1, 2]))):
        with pytest.raises(ParamError, match="search_guests"):
            md.search_guests([lig], [fx], **{**ok, **change})
    with pytest.raises(ParamError, match="ligand 1: no move is enabled"):      # only the torsion amplitude, and ligand 1 has no torsion
        md.search_guests([lig, lig], [fx, rigid], **{**ok, "trans_amp": 0.0, "rot_amp": 0.0})


# ---- the planner's search block as a stand-alone program -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan_driver(request, tmp_path_factory):
    """tests/cpp/guest_search_plan_driver.cpp, built plain and with the address and undefined-behaviour sanitizers"""
    exe = tmp_path_factory.mktemp("guest_search_plan_" + request.param) / "guest_search_plan_driver"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + extra + ["-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                                                                      os.path.join(ROOT, "tests", "cpp", "guest_search_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def _plan(exe, shapes):
    text = f"{len(shapes)}\n" + "\n".join(" ".join(str(v) for v in s) for s in shapes) + "\n"
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    lines = run.stdout.decode().splitlines()
    assert run.returncode == 0 and lines and lines[0].split()[0] == "ok", (run.stdout.decode(), run.stderr.decode()[-2000:])
    head = lines[0].split()
    return int(head[1]), int(head[2]), int(head[3]), [[int(v) for v in l.split()[3::2]] for l in lines[1:]]


def test_planner_lays_out_the_mixed_library(plan_driver):
    """The driver checks per chunk what its head states; here: the chunks are those expected and every walker is in one."""
    env, groups, ligs, flex = fc.mixed_flex_case()
    assert [l.count for l in ligs] == [1, 2, 7, 7, 8, 9, 50, 64, 65, 256, 4] and ligs[2].n_poses == 0
    assert flex[9].n_torsions == 32 and len(flex[9].dihedral_idx) == 449
    shapes = [(l.count, l.n_poses, len(l.pairs14), f.n_torsions, len(f.dihedral_idx)) for l, f in zip(ligs, flex)]
    n_chunks, total, largest, per_chunk = _plan(plan_driver, shapes)
    assert (n_chunks, total) == (2, 318) and [c[0] for c in per_chunk] == [256, 62]
    for walkers, search in per_chunk:
        assert search % 16 == 0 and search > 0
    assert largest > max(c[1] for c in per_chunk)


@pytest.mark.parametrize("shapes,chunks", [
    ([(1, 1, 0, 0, 0)], [1]), ([(4, 256, 1, 1, 1)], [256]), ([(4, 257, 1, 1, 1)], [256, 1]), ([(5, 255, 0, 2, 0), (1, 2, 0, 0, 0)], [256, 1]),
    ([(256, 256, 40, 32, 449)], [256]), ([(3, 0, 0, 0, 0), (256, 0, 0, 32, 9)], []),
    ([(7, 100, 1, 2, 5), (64, 600, 2, 32, 111), (9, 30, 0, 3, 0)], [256, 256, 218])])
def test_planner_at_other_shapes(plan_driver, shapes, chunks):
    n_chunks, total, largest, per_chunk = _plan(plan_driver, shapes)
    assert total == sum(s[1] for s in shapes) and [c[0] for c in per_chunk] == chunks and n_chunks == len(chunks)
