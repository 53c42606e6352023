"""`mdx_search_poses` without a GPU: the declarations, the argument and option checks that run before any device is touched, the
Python-side validation of `MdState.search_poses`, and the rule's header (molchanica_amd/csrc/mdx_search_step.h with the two stepper
headers under it, the code the kernels run) compiled into a stand-alone host program and held against the numpy restatement of
tests/pose_search_ref.py: the streams, the moves, the new starts, and whole searches on an analytic field with two wells."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import _abi, systems
from tests import pose_flex_ref as F
from tests import pose_refine_ref as P
from tests import pose_search_ref as S
from tests.test_pose_refine_host import _rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")
OUT = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT, "pose_search_driver")
SRC = os.path.join(ROOT, "tests", "cpp", "pose_search_driver.cpp")

# The two-well searches: walkers (stream ids) of seed SEED that start in the shallow well.  Chosen on the CPU with the restatement:
# test_a_search_on_two_wells asserts what they were chosen for.
SEED, WALKERS = 2024, (0, 1, 2, 3, 4)


def hx(v):
    return float(v).hex()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    return l


def _compile(exe, extra=()):
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "molchanica_amd", "csrc"), SRC,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver():
    return _compile(EXE)


def run_driver(exe, text):
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    return run.stdout.split("\n")


def ligand(n_tors):
    """lig50 at coordinates of 15 - 30 A with the first n_tors of its rotatable bonds -> (x0 fp32, bonds, torsion bonds, moving sides)"""
    s = systems.lig50()
    n = s.n_atoms
    bonds = F.local_bonds(s, 0, n)
    tb = F.rotatable_bonds(n, bonds, 0)[[20, 3, 11, 29, 7][:n_tors]] if n_tors else np.zeros((0, 2), np.uint32)
    x0 = (np.asarray(s.pos, np.float64) + [20.0, 15.0, 25.0]).astype(np.float32)
    return x0, bonds, tb, F.moving_sides(n, bonds, 0, tb)


def _graph_lines(bonds, tb):
    return "".join(f"{p} {q}\n" for p, q in bonds) + "".join(f"{p} {q}\n" for p, q in tb)


def _rows(a):
    return "\n".join(" ".join(hx(v) for v in row) for row in a) + "\n"


def test_header_declares_the_export(tmp_path):
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mdx_search_poses\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_search_poses"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 17 and args[0].startswith("mdx_handle") and args[4].startswith("const float") and args[5].startswith("const uint64_t*")
    assert args[6] == "uint32_t root" and args[7] == "uint32_t n_torsions" and args[9].startswith("const mdx_search_opts")
    assert args[10].startswith("float") and args[13].startswith("double*") and args[16].startswith("uint32_t*")
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+n_rounds;\s*float\s+trans_amp,\s*rot_amp,\s*tors_amp,\s*kT;\s*uint64_t\s+seed;\s*mdx_flex_opts\s+refine;\s*\}\s*mdx_search_opts;", code)
    cap = re.search(r"#define\s+MDX_SEARCH_MAX_ROUNDS\s+(\d+)u?\b", code)
    assert cap and int(cap.group(1)) == _abi.SEARCH_MAX_ROUNDS == S.MAX_ROUNDS
    comment = src[src.index("pose search: per walker"):src.index("#define MDX_SEARCH_MAX_ROUNDS")]
    for must in ("splitmix64", "M(M(M(seed) ^ id) ^ r)", "2^-53", "51 draws", "sixteen points", "u_50 < exp", "strictly", "bit for bit", "+inf",
                 "n_rounds x max_evals > 65536"):
        assert must in comment, must
    # the struct as the C compiler lays it out
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(mdx_search_opts), '
                    'offsetof(mdx_search_opts, seed), offsetof(mdx_search_opts, refine)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    O = _abi.CSearchOpts
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == [C.sizeof(O), O.seed.offset, O.refine.offset] == [64, 24, 32]
    assert re.search(r"\bsearch_poses\s*\(", open(os.path.join(ROOT, "include", "mdx.hpp")).read())
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    assert "pub fn mdx_search_poses" in blk[:blk.index("\n}\n")]
    step = open(os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_search_step.h")).read()
    assert int(re.search(r"#define\s+MDX_SR_BALL_TRIES\s+(\d+)u", step).group(1)) == S.BALL_TRIES
    mix = open(os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_splitmix64.h")).read()
    assert '#include "mdx_internal.h"' not in step and "#include \"mdx_" not in mix      # a stand-alone host program can include it
    assert (S.DRAW_CHOICE, S.DRAW_BALL, S.DRAW_TORSION, S.DRAW_ACCEPT) == (0, 1, 49, 50)


def test_null_arguments_and_options_are_rejected_before_any_device_is_touched(lib):
    fp, up, qp, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    lib.mdx_search_poses.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, fp, qp, C.c_uint32, C.c_uint32, up, C.POINTER(_abi.CSearchOpts),
                                     fp, fp, C.c_uint32, dp, fp, up, up]
    starts = np.zeros((2, 4, 3), np.float32)
    tb = np.array([[1, 2]], np.uint32)
    out = [np.full((2, 4, 3), -7.0, np.float32), np.full((2, 3), -7.0, np.float32), np.full(2, -7.0, np.float64), np.full(2, -7.0, np.float32)]
    br, stt = np.full(2, 77, np.uint32), np.full((2, 4), 77, np.uint32)
    p = lambda a: a.ctypes.data_as(fp)
    R = lambda evals=12, **kw: _abi.CFlexOpts(evals, kw.get("f_tol", 0.1), 0.1, kw.get("tors_tol", 0.1), kw.get("h_start", 0.0), kw.get("h_max", 0.0), kw.get("flags", 1))
    O = lambda n_rounds=4, ta=1.0, ra=0.3, ka=0.5, kT=0.6, refine=None: _abi.CSearchOpts(n_rounds, ta, ra, ka, kT, 7, refine if refine is not None else R())

    def call(h, opts, best=True, starts_in=True, n_tors=1, bonds=True):
        return lib.mdx_search_poses(h, 0, 4, 2, p(starts) if starts_in else None, None, 0, n_tors, tb.ctypes.data_as(up) if bonds else None,
                                    C.byref(opts) if opts is not None else None, p(out[0]) if best else None, p(out[1]), 3,
                                    out[2].ctypes.data_as(dp), p(out[3]), br.ctypes.data_as(up), stt.ctypes.data_as(up))
    assert call(None, O()) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    fake = C.create_string_buffer(64)      # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    h = C.addressof(fake)
    for kw in (dict(opts=None), dict(opts=O(), best=False), dict(opts=O(), starts_in=False), dict(opts=O(), bonds=False)):
        assert call(h, **kw) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error(), kw
    assert call(h, O(), n_tors=_abi.POSE_MAX_TORSIONS + 1) == _abi.MDX_EPARAM and b"MDX_POSE_MAX_TORSIONS" in lib.mdx_last_error()
    nan, inf = float("nan"), float("inf")
    for bad, match in ((O(n_rounds=0), b"n_rounds"), (O(n_rounds=_abi.SEARCH_MAX_ROUNDS + 1), b"n_rounds"),
                       (O(n_rounds=1024, refine=R(65)), b"65536"), (O(n_rounds=17, refine=R(4096)), b"65536"),
                       (O(ta=-1.0), b"negative"), (O(ra=nan), b"not finite"), (O(ka=inf), b"not finite"), (O(kT=-0.1), b"negative"),
                       (O(kT=nan), b"not finite"), (O(ka=3.15), b"pi"), (O(ta=0.0, ra=0.0, ka=0.0), b"no move"),
                       # those of the refinement's options
                       (O(refine=R(0)), b"max_evals"), (O(n_rounds=1, refine=R(_abi.REFINE_MAX_EVALS_CAP + 1)), b"max_evals"),
                       (O(refine=R(f_tol=-0.1)), b"negative"), (O(refine=R(tors_tol=nan)), b"not finite"),
                       (O(refine=R(h_start=0.3, h_max=0.25)), b"h_start"), (O(refine=R(flags=2)), b"flag")):
        assert call(h, bad) == _abi.MDX_EPARAM
        assert match in lib.mdx_last_error(), (match, lib.mdx_last_error())
    assert call(h, O(ta=0.0, ra=0.0), n_tors=0, bonds=False) == _abi.MDX_EPARAM and b"no move" in lib.mdx_last_error()
    assert all((o == -7.0).all() for o in out) and (br == 77).all() and (stt == 77).all()
    # n_walkers == 0 succeeds and does nothing, whatever else is passed
    none = (None,) * 2
    assert lib.mdx_search_poses(h, 0, 4, 0, None, None, 0, 0, None, None, *none, 3, None, None, None, None) == 0
    assert lib.mdx_search_poses(None, 0, 4, 0, None, None, 0, 0, None, None, *none, 3, None, None, None, None) == _abi.MDX_EPARAM


def test_python_wrapper_validates_shape_and_dtype():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    tb = np.array([[1, 2]], np.uint32)
    rest = (4, 1.0, 0.3, 0.5, 0.6, 7, 12, 0.1, 0.1, 0.1)
    for bad in (np.zeros((2, 5, 3), np.float64), np.zeros((5, 3), np.float32), np.zeros((2, 5, 4), np.float32), np.zeros((2, 0, 3), np.float32),
                np.zeros((1, 257, 3), np.float32), [[[0.0, 0.0, 0.0]]]):
        with pytest.raises(ParamError):
            md.search_poses(0, bad, 0, tb, *rest)
    ok = np.zeros((2, 5, 3), np.float32)
    for first in (98, -1):
        with pytest.raises(ParamError):
            md.search_poses(first, ok, 0, tb, *rest)
    for bad_tb in (np.array([1, 2], np.uint32), np.array([[1.0, 2.0]]), np.array([[1, 5]], np.uint32), np.tile(tb, (33, 1))):
        with pytest.raises(ParamError):
            md.search_poses(0, ok, 0, bad_tb, *rest)
    with pytest.raises(ParamError):
        md.search_poses(0, ok, 5, tb, *rest)
    for bad_streams in (np.array([1.0, 2.0]), np.array([1, 2, 3], np.uint64), np.array([-1, 2], np.int64)):
        with pytest.raises(ParamError):
            md.search_poses(0, ok, 0, tb, *rest, streams=bad_streams)
    with pytest.raises(ParamError):
        md.search_poses(0, ok, 0, tb, 4, 1.0, 0.3, 0.5, 0.6, 1 << 64, 12, 0.1, 0.1, 0.1)


def test_the_streams_of_the_header_are_those_of_numpy(driver):
    """Start states, output words and u01 values of (seed, id, r), bit for bit: 3 stream ids x 20 rounds x 51 draws; the known splitmix64
    outputs of state 0; no two rounds' streams of 64 ids x 20 rounds overlap (start states further apart than 51 steps)."""
    assert [S.bits(0, k) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]      # splitmix64 from state 0
    seed = 0x1234567890ABCDEF
    for sid in (0, 5, (1 << 64) - 1):
        out = run_driver(driver, f"V {seed} {sid} 20\n")
        li = 0
        for r in range(20):
            s0 = S.stream(seed, sid, r)
            assert out[li] == f"S {s0:016x}", (sid, r, out[li])
            for k in range(S.DRAW_ACCEPT + 1):
                w, u = out[li + 1 + k].split()
                x = S.bits(s0, k)
                assert int(w, 16) == x and float.fromhex(u) == S.u01(x) and 0.0 < S.u01(x) <= 1.0, (sid, r, k)
            li += S.DRAW_ACCEPT + 2
    # a stream is a function of (seed, id, r) alone - whatever other walkers exist - and the streams do not overlap
    alone = {(sid, r): S.stream(seed, sid, r) for sid in (63, 7, 0) for r in (19, 3)}
    starts = {}
    for sid in range(64):
        for r in range(20):
            starts[S.stream(seed, sid, r)] = (sid, r)
    assert len(starts) == 64 * 20 and all(starts[v] == k for k, v in alone.items())
    inv = pow(S.GOLD, -1, 1 << 64)      # steps between two start states = (s1 - s0) / GOLD mod 2^64
    steps = sorted(((s * inv) & S.M64) for s in starts)
    gaps = [b - a for a, b in zip(steps, steps[1:])] + [steps[0] + (1 << 64) - steps[-1]]
    assert min(gaps) > S.DRAW_ACCEPT, min(gaps)
    assert S.stream(seed + 1, 5, 3) != S.stream(seed, 5, 3) != S.stream(seed, 5, 4)


def _moves_against_the_driver(exe, what, n_tors, amps, seed, sid, n_rounds=20):
    x0, bonds, tb, tors = ligand(n_tors)
    ta, ra, ka = (float(np.float32(v)) for v in amps)
    text = f"M {len(x0)} {hx(ta)} {hx(ra)} {hx(ka)} {seed} {sid} {n_rounds} 0 {len(bonds)} {len(tb)}\n" + _rows(x0) + _graph_lines(bonds, tb)
    out = run_driver(exe, text)
    Y, li, worst, differ, kinds = x0, 0, 0, 0, []
    for r in range(1, n_rounds + 1):
        mv = S.move(ta, ra, ka, len(tors), S.stream(seed, sid, r))
        w = out[li].split()
        assert w[0] == "M" and [int(v) for v in w[1:5]] == [mv["kind"], mv["torsion"], mv["choice"], mv["tries"]], (what, r, out[li], mv)
        got = np.array([float.fromhex(v) for v in w[5:]])
        assert np.array_equal(got, np.concatenate([mv["v"], mv["w"], [mv["dtheta"]]])), (what, r, "the move's numbers are not bit-equal")
        assert np.linalg.norm(mv["v"]) <= ta and np.linalg.norm(mv["w"]) <= ra and abs(mv["dtheta"]) <= ka
        b = np.array([[int(v, 16) for v in out[li + 1 + i].split()] for i in range(len(x0))], np.uint32)
        li += 1 + len(x0)
        Xn = S.perturb(Y, tors, mv)
        ulp = np.abs(b.view(np.int32).astype(np.int64) - Xn.view(np.int32).astype(np.int64))
        assert ulp.max() <= 2, f"{what}, round {r}: X0' differs by {ulp.max()} fp32 ulp"
        worst, differ = max(worst, int(ulp.max())), differ + int((ulp != 0).sum())
        assert not np.array_equal(Xn, Y) or mv["tries"] == S.BALL_TRIES, (what, r, "the move moved nothing")
        kinds.append(mv["kind"])
        Y = b.view(np.float32)      # (the program's X0' is the next round's input on both sides)
    print(f"{what}: kinds {kinds}, {differ} coordinates of X0' not bit-equal, worst {worst} ulp")
    return kinds


def test_the_moves_of_the_header_are_those_of_numpy(driver):
    """Chosen coordinate, ball draw, move and new start, 20 rounds each, every round from the X0' before it: integers and the move's fp64
    numbers bit for bit, X0' within 2 fp32 ulp (the bound of tests/test_pose_flex_host.py for trial coordinates).  T = 0, 1 and 5, three
    stream ids, each amplitude switched off in turn.  Worst seen: 0 ulp, no coordinate not bit-equal."""
    seed = 99
    seen = set()
    for sid in (0, 17, 1 << 40):
        for n_tors in (0, 1, 5):
            k = _moves_against_the_driver(driver, f"stream {sid}, T = {n_tors}, all moves", n_tors, (1.5, 0.4, 0.6), seed, sid)
            seen |= set(k)
            assert set(k) <= ({S.TRANSLATION, S.ROTATION} if n_tors == 0 else {S.TRANSLATION, S.ROTATION, S.TORSION})
    assert seen == {S.TRANSLATION, S.ROTATION, S.TORSION}
    for amps, allowed in (((0.0, 0.4, 0.6), {S.ROTATION, S.TORSION}), ((1.5, 0.0, 0.6), {S.TRANSLATION, S.TORSION}), ((1.5, 0.4, 0.0), {S.TRANSLATION, S.ROTATION}),
                          ((0.0, 0.0, math.pi), {S.TORSION}), ((0.0, 0.2, 0.0), {S.ROTATION}), ((2.0, 0.0, 0.0), {S.TRANSLATION})):
        k = _moves_against_the_driver(driver, f"amplitudes {amps}", 5, amps, seed, 3)
        assert set(k) == allowed, (amps, k)
    # every one of the five torsions is reached, uniformly enough: 7 choices, 400 rounds
    mv = [S.move(1.0, 1.0, 1.0, 5, S.stream(1, 2, r)) for r in range(1, 401)]
    counts = np.bincount([m["choice"] for m in mv], minlength=7)
    assert counts.min() >= 35 and max(m["tries"] for m in mv) < S.BALL_TRIES, counts
    assert abs(np.mean([m["tries"] == 0 for m in mv]) - math.pi / 6) < 0.08


def two_wells(x0, tors, k=2.0, d1=0.0, d2=-40.0, hole=0.0, hp=(0.0, 0.0, 0.0)):
    """The field of the driver's W mode: well 1 around the ligand with its torsions turned a little, well 2 that shape turned further,
    rotated by 0.25 rad and 1.6 A away, deeper by d1 - d2.  -> (targets 1, targets 2, evaluate)"""
    rng = np.random.default_rng(11)
    T1 = F.turn(x0.astype(np.float64), tors, 0.15 * rng.uniform(-1, 1, len(tors)))
    T2 = F.turn(T1, tors, 0.4 * rng.uniform(-1, 1, len(tors)))
    c = T2.mean(0)
    T2 = (T2 - c) @ _rot([2, -1, 1], 0.25).T + c + [1.2, -0.8, 0.7]
    e1, e2 = F.synthetic_evaluate(T1, k), F.synthetic_evaluate(T2, k)
    hp = np.asarray(hp, np.float64)

    def evaluate(Y):
        r1, r2 = e1(Y), e2(Y)
        a, b = float(r1[0][0]) + d1, float(r2[0][0]) + d2
        row, rigid, f = (np.array([a], np.float32), r1[1], r1[2]) if a <= b else (np.array([b], np.float32), r2[1], r2[2])
        if hole > 0.0 and P.norm3(np.asarray(Y, np.float32).astype(np.float64)[0] - hp) < hole:
            row = np.array([np.nan], np.float32)
        return row, rigid, f
    return T1, T2, evaluate


def well_of(pose, T1, T2):
    y = np.asarray(pose, np.float64)
    return 1 if ((y - T1) ** 2).sum() <= ((y - T2) ** 2).sum() else 2


REFINE = dict(max_evals=12, f_tol=1e-3, tau_tol=1e-3, tors_tol=1e-3, h_start=0.05, h_max=0.5)


def _search_both(exe, x0, bonds, tb, tors, field, n_rounds, amps, kT, seed, sid, k=2.0, d=(0.0, -40.0), hole=0.0, hp=(0.0, 0.0, 0.0)):
    """One walker through the program and through the restatement -> (the restatement's result, its trace); asserts they agree"""
    T1, T2, evaluate = field
    ta, ra, ka, kT = (float(np.float32(v)) for v in (*amps, kT))
    o = REFINE
    text = (f"W {len(x0)} {hx(k)} {hx(d[0])} {hx(d[1])} {hx(hole)} {hx(hp[0])} {hx(hp[1])} {hx(hp[2])} {o['max_evals']} "
            + " ".join(hx(np.float32(o[v])) for v in ("f_tol", "tau_tol", "tors_tol", "h_start", "h_max"))
            + f" {hx(ta)} {hx(ra)} {hx(ka)} {hx(kT)} {seed} {sid} {n_rounds} 0 {len(bonds)} {len(tb)}\n" + _rows(x0) + _rows(T1) + _rows(T2) + _graph_lines(bonds, tb))
    out = run_driver(exe, text)
    trace = []
    res = S.search(x0, S.numpy_refiner(evaluate, tors, F.NO_TERMS, **o), tors, n_rounds, ta, ra, ka, kT, seed, sid, trace=trace)
    for r, t in enumerate(trace):
        tag, fl, Sr, fin, ev = out[r].split()
        flags = (1 if t["accept"] else 0) | (2 if t["uphill"] else 0) | (4 if t["best"] else 0)
        assert tag == "D" and int(fl) == flags and int(fin) == int(t["result"]["finite"]) and int(ev) == t["result"]["evals"], (sid, r, out[r], flags, t["result"]["evals"])
        if t["result"]["finite"]:
            assert abs(float.fromhex(Sr) - t["result"]["S"]) <= 1e-9 * max(1.0, abs(t["result"]["S"])), (sid, r, Sr, t["result"]["S"])
    w = out[n_rounds].split()
    assert w[0] == "B" and [int(v) for v in w[1:6]] == [res["best_round"]] + res["stats"].tolist(), (sid, out[n_rounds], res["best_round"], res["stats"])
    b = np.array([[int(v, 16) for v in out[n_rounds + 1 + i].split()] for i in range(len(x0))], np.uint32)
    ulp = np.abs(b.view(np.int32).astype(np.int64) - res["pose"].view(np.int32).astype(np.int64))
    assert ulp.max() <= 2, f"walker {sid}: the best pose differs by {ulp.max()} fp32 ulp"
    return res, trace


def test_a_search_on_two_wells(driver):
    """Whole searches, program against restatement: per round the decision's flags, finiteness and evaluation count, at the end best round,
    the four counters and the best pose (within 2 fp32 ulp; the refinements inside are those of tests/test_pose_flex_host.py).  lig50
    with five torsions in a field of two quadratic wells 1.6 A apart, the second 40 kcal/mol deeper; every walker starts in the shallow
    one.  12 rounds x 12 evaluations, moves of up to 1.2 A / 0.3 rad / 0.5 rad, kT = 15 kcal/mol: at least one of the five walkers ends
    with its best in the deeper well, and some round is accepted uphill; the refinement alone (n_rounds = 1) leaves all five in the
    shallow one; with kT = 0 the same walkers never accept uphill."""
    x0, bonds, tb, tors = ligand(5)
    field = two_wells(x0, tors)
    T1, T2, evaluate = field
    assert well_of(x0, T1, T2) == 1
    amps = (1.2, 0.3, 0.5)
    wells, uphill, accepted = [], 0, 0
    for sid in WALKERS:
        alone, _ = _search_both(driver, x0, bonds, tb, tors, field, 1, amps, 15.0, SEED, sid)
        assert well_of(alone["pose"], T1, T2) == 1 and alone["best_round"] == 0 and alone["stats"][:3].tolist() == [0, 0, 0]
        res, trace = _search_both(driver, x0, bonds, tb, tors, field, 12, amps, 15.0, SEED, sid)
        # the prefix property of the rule: round 0 of the long search is the short one
        assert np.array_equal(trace[0]["result"]["pose"], alone["pose"]) and res["S"] <= alone["S"]
        wells.append(well_of(res["pose"], T1, T2))
        uphill, accepted = uphill + int(res["stats"][1]), accepted + int(res["stats"][0])
        cold, tr0 = _search_both(driver, x0, bonds, tb, tors, field, 12, amps, 0.0, SEED, sid)
        assert cold["stats"][1] == 0 and all(t["margin"] is None for t in tr0)
        S_cur = math.inf
        for t in tr0:      # downhill only: the accepted objective never rises
            if t["accept"]:
                assert t["result"]["S"] < S_cur or t is tr0[0]
                S_cur = t["result"]["S"]
    print(f"two wells: best in well {wells}, {accepted} rounds accepted, {uphill} of them uphill")
    assert 2 in wells and uphill >= 1 and accepted > uphill


def test_a_non_finite_round_0_is_replaced_by_the_first_finite_round(driver):
    """The field has a hole of 0.8 A around atom 0 of the start, where the row is NaN: round 0 ends NONFINITE after one evaluation, S_cur =
    S_best = +inf and the best is the input; rounds whose move leaves atom 0 inside the hole are non-finite and rejected; the first finite
    round is accepted and becomes the best.  Only torsion moves that do not move atom 0 (the root) stay inside: with translations only,
    of at most 1 A, some rounds do."""
    x0, bonds, tb, tors = ligand(5)
    hp = x0[0].astype(np.float64)
    field = two_wells(x0, tors, hole=0.8, hp=hp)
    res, trace = _search_both(driver, x0, bonds, tb, tors, field, 8, (1.0, 0.0, 0.0), 0.0, 5, 2, hole=0.8, hp=hp)
    fin = [t["result"]["finite"] for t in trace]
    assert not fin[0] and trace[0]["result"]["evals"] == 1 and np.array_equal(trace[0]["result"]["pose"], x0)
    first = fin.index(True)
    assert first >= 2, f"some round after round 0 should still lie in the hole: {fin}"
    assert trace[first]["accept"] and trace[first]["best"] and not any(t["accept"] for t in trace[1:first])
    assert res["stats"][2] == fin.count(False) and res["best_round"] >= first and math.isfinite(res["S"])
    # no finite round at all: the best is the input, S = +inf
    none, tr = _search_both(driver, x0, bonds, tb, tors, field, 3, (0.01, 0.0, 0.0), 0.0, 5, 2, hole=0.8, hp=hp)
    assert none["S"] == math.inf and none["best_round"] == 0 and np.array_equal(none["pose"], x0) and none["stats"].tolist() == [0, 0, 3, 3]


def test_the_driver_under_the_sanitizers():
    """The same stand-alone host program built with -fsanitize=address,undefined and run once on a short case of each mode."""
    exe = _compile(EXE + "_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_driver(exe, "V 1 2 2\n")[0].startswith("S ")
    x0, bonds, tb, tors = ligand(5)
    text = f"M {len(x0)} {hx(1.0)} {hx(0.5)} {hx(0.5)} 3 4 6 0 {len(bonds)} {len(tb)}\n" + _rows(x0) + _graph_lines(bonds, tb)
    assert run_driver(exe, text)[0].startswith("M ")
    T1, T2, _ = two_wells(x0, tors)
    o = REFINE
    text = (f"W {len(x0)} {hx(2.0)} {hx(0.0)} {hx(-40.0)} {hx(0.0)} {hx(0.0)} {hx(0.0)} {hx(0.0)} 6 "
            + " ".join(hx(np.float32(o[v])) for v in ("f_tol", "tau_tol", "tors_tol", "h_start", "h_max"))
            + f" {hx(1.0)} {hx(0.3)} {hx(0.5)} {hx(15.0)} 1 0 3 0 {len(bonds)} {len(tb)}\n" + _rows(x0) + _rows(T1) + _rows(T2) + _graph_lines(bonds, tb))
    out = run_driver(exe, text)
    assert out[0].startswith("D ") and out[3].startswith("B ")
