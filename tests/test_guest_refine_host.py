"""`mdx_guest_forces` / `mdx_refine_guests` without a GPU: the declarations and their mirrors, the argument checks that run before a
device is touched, the Python wrappers, the numpy stepper under a G + 1-wide evaluate function, the shared chunk planner
(molchanica_amd/csrc/mdx_pose_plan.h) as a stand-alone program under the address and undefined-behaviour sanitizers, and the conditions
under which tests/test_gpu_guest_refine.py means something (the oracle's slack cap on the poses it compares)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import GuestLigand, _abi
from tests import guest_cases as gc
from tests import pose_force_ref as pfr
from tests import pose_refine_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")

t = gc.pose_batch_module()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    l.mdx_guest_forces.argtypes = _abi.GUEST_FORCES_ARGTYPES
    l.mdx_refine_guests.argtypes = _abi.REFINE_GUESTS_ARGTYPES
    return l


def _declared(name):
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", code)
    assert m, f"mdx.h does not declare {name}"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")], src


def test_header_declares_both_exports_and_the_mirrors_follow():
    args, src = _declared("mdx_guest_forces")
    assert [a.rsplit(" ", 1)[0] for a in args] == ["mdx_handle*", "uint32_t", "const mdx_guest_ligand*", "float*", "uint32_t", "float*", "float*"]
    assert len(_abi.GUEST_FORCES_ARGTYPES) == len(args) == 7
    args, _ = _declared("mdx_refine_guests")
    assert [a.rsplit(" ", 1)[0] for a in args] == ["mdx_handle*", "uint32_t", "const mdx_guest_ligand*", "const mdx_refine_opts*", "float*", "float*",
                                                   "uint32_t", "float*", "float*", "uint32_t*", "uint32_t*", "uint32_t*", "double*"]
    assert len(_abi.REFINE_GUESTS_ARGTYPES) == len(args) == 13
    assert _abi.REFINE_GUESTS_ARGTYPES[3] == C.POINTER(_abi.CRefineOpts) and _abi.REFINE_GUESTS_ARGTYPES[12] == C.POINTER(C.c_double)
    comment = src[src.index("guest ligands with gradients"):src.index("int      mdx_guest_forces")]
    for must in ("bit for bit", "MDX_REFINE_NONFINITE", "never wins", "lowest ligand-local index", "ligand-major", "MDX_ENAN", "writes nothing",
                 "any size and order", "alchemical", "softened-Coulomb", "MDX_OVR_BONDED_DISABLED"):
        assert must in comment, must
    hpp = open(os.path.join(ROOT, "include", "mdx.hpp")).read()
    assert re.search(r"\bguest_forces\s*\(", hpp) and re.search(r"\brefine_guests\s*\(", hpp)
    assert "mdx_guest_forces(h_" in hpp and "mdx_refine_guests(h_" in hpp
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    blk = blk[:blk.index("\n}\n")]
    assert "pub fn mdx_guest_forces" in blk and "pub fn mdx_refine_guests" in blk
    from tests.test_abi import declared_symbols
    assert f"({len(declared_symbols())} exports)" in open(os.path.join(ROOT, "README.md")).read()


def test_every_export_is_still_bound_or_listed():
    from tests.test_abi import test_every_export_is_bound_or_listed as held
    held()


def test_the_library_exports_both_and_refuses_on_the_arguments_alone(lib):
    fp, up, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    recs = (_abi.CGuestLigand * 1)()
    out = [np.full(24, -7.0, np.float32) for _ in range(5)]
    st, ev, bp = (np.full(2, 77, np.uint32) for _ in range(3))
    bs = np.full(2, -7.0, np.float64)
    p = lambda a: a.ctypes.data_as(fp)
    u = lambda a: a.ctypes.data_as(up)
    good = _abi.CRefineOpts(12, 0.1, 0.1, 0.0, 0.0)
    assert lib.mdx_guest_forces(None, 1, recs, p(out[0]), 2, p(out[1]), p(out[2])) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    assert lib.mdx_guest_forces(None, 0, None, None, 2, None, None) == _abi.MDX_EPARAM

    def refine(h, n, ligs, opts):
        return lib.mdx_refine_guests(h, n, ligs, None if opts is None else C.byref(opts), p(out[0]), p(out[1]), 2, p(out[2]), p(out[3]), u(st),
                                     u(ev), u(bp), bs.ctypes.data_as(dp))
    assert refine(None, 1, recs, good) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    fake = C.create_string_buffer(64)
    h = C.addressof(fake)
    assert refine(h, 1, None, good) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    assert refine(h, 1, recs, None) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    assert lib.mdx_guest_forces(h, 1, None, p(out[0]), 2, p(out[1]), p(out[2])) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    for bad, match in ((_abi.CRefineOpts(0, 0.1, 0.1, 0, 0), b"max_evals"), (_abi.CRefineOpts(_abi.REFINE_MAX_EVALS_CAP + 1, 0.1, 0.1, 0, 0), b"max_evals"),
                       (_abi.CRefineOpts(12, -0.1, 0.1, 0, 0), b"negative"), (_abi.CRefineOpts(12, 0.1, float("nan"), 0, 0), b"not finite"),
                       (_abi.CRefineOpts(12, 0.1, 0.1, 0.3, 0.25), b"h_start"), (_abi.CRefineOpts(12, 0.1, 0.1, 0.0, 0.005), b"h_start")):
        assert refine(h, 1, recs, bad) == _abi.MDX_EPARAM
        assert match in lib.mdx_last_error() and b"mdx_refine_guests" in lib.mdx_last_error(), lib.mdx_last_error()
    assert all((o == -7.0).all() for o in out) and (st == 77).all() and (ev == 77).all() and (bp == 77).all() and (bs == -7.0).all()
    # no ligand: succeeds and does nothing, whatever else is passed
    assert lib.mdx_guest_forces(h, 0, None, None, 2, None, None) == 0
    assert lib.mdx_refine_guests(h, 0, None, None, None, None, 2, None, None, None, None, None, None) == 0


def test_python_wrappers_validate_the_library():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    ok = dict(charge=np.zeros(4), lj_sigma=np.ones(4), lj_eps=np.ones(4))
    for bad in ([dict(ok)],                                                                    # not GuestLigand objects
                [GuestLigand(np.zeros(0), np.zeros(0), np.zeros(0))],                          # empty ligand
                [GuestLigand(np.zeros(257), np.zeros(257), np.zeros(257))],                    # above MDX_POSE_MAX_ATOMS
                [GuestLigand(np.zeros(4), np.ones(3), np.ones(4))],                            # sigma of another length
                [GuestLigand(**ok, pairs14=np.zeros(5, np.uint32))],                           # not pairs
                [GuestLigand(**ok), GuestLigand(**ok, poses=np.zeros((2, 5, 3), np.float32))],  # poses of another ligand
                [GuestLigand(**ok, poses="x")]):                                               # not numbers
        with pytest.raises(ParamError, match="guest_forces"):
            md.guest_forces(bad)
        with pytest.raises(ParamError, match="refine_guests"):
            md.refine_guests(bad, 12, 0.1, 0.1)


def test_per_ligand_views_of_a_flat_result():
    from molchanica_amd.md_state import MdState
    flat = np.arange(3 * (2 * 5 + 0 * 7 + 3 * 1), dtype=np.float32)
    parts = MdState._per_ligand(flat, [2, 0, 3], [5, 7, 1])
    assert [p.shape for p in parts] == [(2, 5, 3), (0, 7, 3), (3, 1, 3)]
    assert np.array_equal(np.concatenate([p.ravel() for p in parts]), flat)
    rows = MdState._per_ligand(np.arange(15, dtype=np.float32).reshape(5, 3), [2, 0, 3])
    assert [r.shape for r in rows] == [(2, 3), (0, 3), (3, 3)] and rows[2][0, 0] == 6.0


# ---- the numpy stepper under a G + 1-wide row --------------------------------------------------------------------------------------------------
def test_the_numpy_stepper_with_a_wide_row_reproduces_its_closed_cases():
    """The stepper sums whatever row `evaluate` returns in column order.  (a) The quadratic field's energy in the LAST of three columns
    (the guests' own-pair column) behind two zeros: every output is the one-column run's, bit for bit.  (b) The energy split over three
    columns: S is a sum of three fp32 numbers now, the closed form still holds - a body pulled to a rotated and shifted copy of itself
    arrives there (the minimum is the target, S = 0), rigid, downhill."""
    rng = np.random.default_rng(3)
    x0 = (rng.normal(0, 4, (50, 3)) + [30, -20, 55]).astype(np.float32)
    x = x0.astype(np.float64)
    c = x.mean(0)
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = (x - c) @ (np.eye(3) + np.sin(0.4) * K + (1 - np.cos(0.4)) * K @ K).T + c + [0.6, -0.3, 0.4]
    narrow = P.synthetic_evaluate(T, 2.0)

    def last_column(Y):
        row, rigid = narrow(Y)
        return np.array([0.0, 0.0, row[0]], np.float32), rigid

    def split(Y):
        row, rigid = narrow(Y)
        return np.array([0.25, 0.25, 0.5], np.float32) * row[0], rigid

    one = P.refine(x0, narrow, 40, 1e-3, 1e-3, 0.05, 1.0)
    wide = P.refine(x0, last_column, 40, 1e-3, 1e-3, 0.05, 1.0)
    assert wide["row"].shape == (3,) and one["row"].shape == (1,)
    for k in ("pose", "rigid", "q", "t"):
        assert np.array_equal(one[k], wide[k]), k
    assert (one["status"], one["evals"], one["S"]) == (wide["status"], wide["evals"], wide["S"])
    res = P.refine(x0, split, 400, 1e-2, 1e-2, 0.05, 1.0)
    assert res["status"] == P.CONVERGED and res["row"].shape == (3,)
    y = res["pose"].astype(np.float64)
    assert np.abs(y - T).max() <= 1e-2 and res["S"] < 1e-3 < float(narrow(x0)[0][0])
    d0 = np.linalg.norm(x[:, None] - x[None], axis=2)
    assert np.abs(np.linalg.norm(y[:, None] - y[None], axis=2) - d0).max() <= 4 * np.spacing(np.float32(np.abs(y).max()))
    # a non-finite own-pair column at evaluation 0 is the pose's status
    bad = P.refine(x0, lambda Y: (np.array([1.0, 2.0, np.inf], np.float32), np.zeros(6, np.float32)), 5, 0, 0)
    assert bad["status"] == P.NONFINITE and bad["evals"] == 1 and np.array_equal(bad["pose"], x0)


# ---- the chunk planner as a stand-alone program ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    """tests/cpp/guest_plan_driver.cpp: the planner header on one host thread, built with the address and undefined-behaviour sanitizers"""
    exe = tmp_path_factory.mktemp("guest_plan") / "guest_plan_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "molchanica_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "guest_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


PLAN_LIBRARIES = {
    "one ligand, one pose": ([(5, 1, 0)], 1, 1),
    "256 poses": ([(50, 256, 3)], 1, 256),
    "257 poses": ([(50, 257, 3)], 2, 257),
    "256 poses over two ligands": ([(9, 200, 1), (8, 56, 0)], 1, 256),
    "a ligand straddling two chunk boundaries": ([(7, 100, 1), (64, 600, 2), (9, 30, 0)], 3, 730),
    "ligands with no poses at the start, middle and end": ([(3, 0, 0), (4, 10, 1), (3, 0, 5), (5, 300, 2), (3, 0, 0)], 2, 310),
    "an empty ligand exactly at a chunk boundary": ([(4, 256, 0), (6, 0, 2), (5, 3, 1)], 2, 259),
    "sizes 1 and 256 in one chunk": ([(1, 128, 0), (256, 128, 9)], 1, 256),
    "the largest chunk there is": ([(256, 256, 40)], 1, 256),
    "nothing but empty ligands": ([(3, 0, 0), (256, 0, 0)], 0, 0),
}


@pytest.mark.parametrize("name", list(PLAN_LIBRARIES))
def test_chunk_planner_under_the_sanitizers(plan_driver, name):
    """Per library and mode the driver checks: every offset aligned, the parts of a block disjoint and inside it, the records tiling the
    pose range exactly and pointing inside the chunk's tables."""
    ligs, n_chunks, total = PLAN_LIBRARIES[name]
    text = f"{len(ligs)}\n" + "\n".join(f"{c} {p} {k}" for c, p, k in ligs) + "\n"
    run = subprocess.run([plan_driver], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = run.stdout.decode().split()
    assert run.returncode == 0 and out[0] == "ok", (name, run.stdout.decode(), run.stderr.decode()[-2000:])
    assert (int(out[1]), int(out[2])) == (n_chunks, total), (name, out)
    if total:
        # the refinement's block holds at least the slab and the force slab of its poses
        assert int(out[3]) >= 8 * 17 * 3 * min(c for c, p, _ in ligs if p)


# ---- the conditions of the GPU test's oracle comparison ----------------------------------------------------------------------------------------
def test_the_oracle_alone_keeps_the_caps_on_the_compared_poses(orc):
    """tests/test_gpu_guest_refine.py compares the guest's forces on the small complex's 16 poses with the oracle on the COMBINED system
    under the bound of tests/test_gpu_pose_forces.py; that bound carries two conditions - at most MAX_DROPPED poses clash, at most
    MAX_SLACK_ROWS of the compared rows carry slack - which are properties of the poses and the oracle alone."""
    S, R, gR, (lo, hi), lig = gc.small_case()
    comb, g, n, (clo, chi), env_at = gc.combined(R, gR, gc.only_molecules(S, [1]))
    pos_s = orc.wrap(S, S.pos)
    poses = t.rigid_poses(t.whole(S, pos_s[lo:hi]), 16, t.SEED_SMALL)
    pos = np.concatenate([np.delete(pos_s, np.s_[lo:hi], 0), poses[0]])
    assert (chi - clo, comb.n_atoms) == (hi - lo, S.n_atoms)
    for cfg in t.small_configs():
        dropped, slacked, rows, _ = pfr.caps(orc, comb, cfg, pos, clo, chi, poses)
        print(f"coulomb mode {cfg.coulomb_mode}: {dropped} poses dropped, {slacked} of {rows} rows with slack")
        assert dropped <= pfr.MAX_DROPPED and slacked <= pfr.MAX_SLACK_ROWS * rows
