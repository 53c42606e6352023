"""`mdx_refine_poses` without a GPU: the declarations, the argument and option checks that run before any device is touched, the
Python-side validation of `MdState.refine_poses`, the stepper header (molchanica_amd/csrc/mdx_refine_step.h, the code the step kernel
runs) compiled into a stand-alone host program and held against the numpy stepper of tests/pose_refine_ref.py, and that numpy
stepper driven by the fp64 oracle on the poses of tests/test_gpu_pose_refine.py: the caps of tests/pose_force_ref.py hold for the
starts and for the refined poses, and the convergence parameters of the GPU test converge on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import _abi, systems
from tests import pose_force_ref as R
from tests import pose_refine_ref as P
from tests.test_gpu_pose_batch import (MAX_DROPPED, SEED_SMALL, ligand_range, min_env_distance, rigid_poses, small_configs, three_groups,
                                       whole)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")
OUT = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT, "pose_refine_driver")

# tests/test_gpu_pose_refine.py::test_convergence_on_the_crystal: one molecule of systems.molecular_crystal() as the range.  Chosen on the
# CPU with the oracle-driven loop below: all 16 poses converge, the slowest after 151 evaluations.
CRYSTAL_SEED, CRYSTAL_ROT, CRYSTAL_TR = 1, 0.3, 1.0
CRYSTAL_F_TOL, CRYSTAL_TAU_TOL, CRYSTAL_MAX_EVALS = 0.5, 1.0, 200


def crystal_case():
    """-> (system, config, group map, lo, hi) of the convergence test"""
    from molchanica_amd import MdConfig
    s = systems.molecular_crystal()
    lo, hi = int(s.mol_start[0]), int(s.mol_start[1])
    g = np.zeros(s.n_atoms, np.uint8)
    g[lo:hi] = 1
    return s, MdConfig(lj_cutoff=8.0, coulomb_cutoff=8.0, skin=1.0), g, lo, hi      # (the box is 40 x 20 x 20 A: 2 (cutoff + skin) must stay below 20)


def crystal_poses(start):
    return rigid_poses(start, 16, CRYSTAL_SEED, max_rot=CRYSTAL_ROT, max_tr=CRYSTAL_TR)


def oracle_evaluate(orc, s, cfg, g, n_groups, pos, lo, hi, lig_group, use_cells=True):
    """`evaluate` of the numpy stepper from the oracle alone: its ligand row and the rigid sums of its non-bonded forces, as fp32"""
    s_nb = R.nonbonded_only(s)

    def evaluate(Y):
        x = R.full_set(pos, lo, hi, Y)
        mo, _ = orc.between_mols(s, cfg, g, n_groups, pos=x, use_cells=use_cells)
        fo = orc.forces(s_nb, cfg, pos=x, use_cells=use_cells)[0][lo:hi]
        return mo[lig_group].astype(np.float32), R.rigid_of(Y, fo).astype(np.float32)
    return evaluate


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    return l


def test_header_declares_the_export():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mdx_refine_poses\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_refine_poses"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13 and args[0].startswith("mdx_handle") and args[4].startswith("const float")
    assert args[5].startswith("const mdx_refine_opts") and args[6].startswith("float") and args[11].startswith("uint32_t*")
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+max_evals;\s*float\s+f_tol,\s*tau_tol,\s*h_start,\s*h_max;\s*\}\s*mdx_refine_opts;", code)
    for name, val in (("CONVERGED", 0), ("MAX_EVALS", 1), ("STALLED", 2), ("NONFINITE", 3)):
        assert re.search(rf"#define\s+MDX_REFINE_{name}\s+{val}u?\b", code), name
        assert getattr(_abi, "REFINE_" + name) == val
    cap = re.search(r"#define\s+MDX_REFINE_MAX_EVALS_CAP\s+(\d+)u?\b", code)
    assert cap and int(cap.group(1)) == _abi.REFINE_MAX_EVALS_CAP
    comment = src[src.index("local refinement of the same batch"):src.index("typedef struct { uint32_t max_evals")]
    for must in ("whole molecule", "alone or in a batch of any size", "lambda", "0.5 h", "1.2 h", "MDX_REFINE_STALLED"):
        assert must in comment, must
    assert C.sizeof(_abi.CRefineOpts) == 20
    assert re.search(r"\brefine_poses\s*\(", open(os.path.join(ROOT, "include", "mdx.hpp")).read())
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    assert "pub fn mdx_refine_poses" in blk[:blk.index("\n}\n")]
    # the header's constants are the stepper's
    step = open(os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_refine_step.h")).read()
    for name, val in (("H_MIN", P.H_MIN), ("LAMBDA_REL", P.LAMBDA_REL), ("LAMBDA_ABS", P.LAMBDA_ABS)):
        assert float(re.search(rf"#define\s+MDX_RF_{name}\s+(\S+)", step).group(1)) == val


def test_null_arguments_and_options_are_rejected_before_any_device_is_touched(lib):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    lib.mdx_refine_poses.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, fp, C.POINTER(_abi.CRefineOpts), fp, fp, C.c_uint32, fp,
                                     fp, up, up]
    poses = np.zeros((2, 4, 3), np.float32)
    out = [np.full((2, 4, 3), -7.0, np.float32), np.full((2, 3), -7.0, np.float32), np.full((2, 6), -7.0, np.float32),
           np.full((2, 7), -7.0, np.float32)]
    st, ev = np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    p = lambda a: a.ctypes.data_as(fp)
    good = _abi.CRefineOpts(12, 0.1, 0.1, 0.0, 0.0)

    def call(h, opts, poses_out=True, poses_in=True):
        return lib.mdx_refine_poses(h, 0, 4, 2, p(poses) if poses_in else None, C.byref(opts) if opts is not None else None,
                                    p(out[0]) if poses_out else None, p(out[1]), 3, p(out[2]), p(out[3]), st.ctypes.data_as(up),
                                    ev.ctypes.data_as(up))
    assert call(None, good) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    assert lib.mdx_refine_poses(None, 0, 4, 0, None, None, None, None, 3, None, None, None, None) == _abi.MDX_EPARAM
    # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    fake = C.create_string_buffer(64)
    h = C.addressof(fake)
    for kw in (dict(opts=None), dict(opts=good, poses_out=False), dict(opts=good, poses_in=False)):
        assert call(h, **kw) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error(), kw
    for bad, match in ((_abi.CRefineOpts(0, 0.1, 0.1, 0, 0), b"max_evals"),
                       (_abi.CRefineOpts(_abi.REFINE_MAX_EVALS_CAP + 1, 0.1, 0.1, 0, 0), b"max_evals"),
                       (_abi.CRefineOpts(12, -0.1, 0.1, 0, 0), b"negative"), (_abi.CRefineOpts(12, 0.1, float("nan"), 0, 0), b"not finite"),
                       (_abi.CRefineOpts(12, 0.1, 0.1, float("inf"), 0), b"not finite"), (_abi.CRefineOpts(12, 0.1, 0.1, 0, -1.0), b"negative"),
                       (_abi.CRefineOpts(12, 0.1, 0.1, 0.3, 0.25), b"h_start"),
                       (_abi.CRefineOpts(12, 0.1, 0.1, 0.3, 0.0), b"h_start"),      # h_max = 0 selects 0.2 A, below h_start
                       (_abi.CRefineOpts(12, 0.1, 0.1, 0.0, 0.005), b"h_start")):   # h_start = 0 selects 0.01 A, above h_max
        assert call(h, bad) == _abi.MDX_EPARAM
        assert match in lib.mdx_last_error(), (match, lib.mdx_last_error())
    assert all((o == -7.0).all() for o in out) and (st == 77).all() and (ev == 77).all()
    # n_poses == 0 succeeds and does nothing, whatever else is passed
    assert lib.mdx_refine_poses(h, 0, 4, 0, None, None, None, None, 3, None, None, None, None) == 0


def test_python_wrapper_validates_shape_and_dtype():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    for bad in (np.zeros((2, 5, 3), np.float64), np.zeros((5, 3), np.float32), np.zeros((2, 5, 4), np.float32),
                np.zeros((2, 0, 3), np.float32), np.zeros((1, 257, 3), np.float32), [[[0.0, 0.0, 0.0]]]):
        with pytest.raises(ParamError):
            md.refine_poses(0, bad, 12, 0.1, 0.1)
    with pytest.raises(ParamError):
        md.refine_poses(98, np.zeros((1, 5, 3), np.float32), 12, 0.1, 0.1)
    with pytest.raises(ParamError):
        md.refine_poses(-1, np.zeros((1, 5, 3), np.float32), 12, 0.1, 0.1)


def test_coords_of_the_identity_are_the_input_bits():
    rng = np.random.default_rng(17)
    for scale, off in ((4.0, (30.0, -20.0, 55.0)), (1.0, (0.0, 0.0, 0.0)), (8.0, (-400.0, 250.0, 1000.0))):
        x0 = (rng.normal(0, scale, (50, 3)) + off).astype(np.float32)
        x0[7] = 0.0      # an atom at the origin
        y = P.coords(P.mean(x0.astype(np.float64)), np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]), x0)
        assert np.array_equal(y.view(np.uint32), x0.view(np.uint32))


def _bodies():
    rng = np.random.default_rng(3)
    return (("a general 50-atom body", (rng.normal(0, 4, (50, 3)) + [30, -20, 55]).astype(np.float32)),
            ("three atoms", (rng.normal(0, 1, (3, 3)) + [10, 10, 10]).astype(np.float32)),
            ("one atom", np.array([[5.0, 6.0, 7.0]], np.float32)),
            ("two atoms", np.array([[5.0, 6.0, 7.0], [6.2, 6.5, 7.9]], np.float32)),
            ("three collinear atoms", (np.array([[1.0, 2.0, 3.0]]) + np.outer([0.0, 1.1, 2.7], [0.3, -0.5, 0.8])).astype(np.float32)))


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * k @ k


def test_the_stepper_header_as_a_host_program_matches_the_numpy_stepper():
    """mdx_refine_step.h compiled by the host compiler into tests/cpp/pose_refine_driver.cpp, against tests/pose_refine_ref.py: a
    quadratic field pulls every body to a rotated and shifted copy of itself, h_start 0.05 A and h_max 1 A so that the step
    overshoots and the run holds accepts and rejects.  Per evaluation the decision (store / finished) and the step length must be
    equal and the next trial's coordinates agree within 2 fp32 ulp; so must status, evaluation count and the accepted (q, t)."""
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "pose_refine_driver.cpp"), "-o", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hx = lambda v: float(v).hex()
    k, evals, f_tol, tau_tol, h_start, h_max = 2.0, 40, 1e-3, 1e-3, 0.05, 1.0
    for what, x0 in _bodies():
        x = x0.astype(np.float64)
        c = x.mean(0)
        T = (x - c) @ _rot([1, 2, 3], 0.4).T + c + [0.6, -0.3, 0.4]
        trace = []
        res = P.refine(x0, P.synthetic_evaluate(T, k), evals, f_tol, tau_tol, h_start, h_max, trace=trace)
        text = f"{len(x0)} {hx(k)} {evals} " + " ".join(hx(np.float32(v)) for v in (f_tol, tau_tol, h_start, h_max)) + "\n"
        text += "\n".join(" ".join(hx(v) for v in row) for row in x0) + "\n" + "\n".join(" ".join(hx(v) for v in row) for row in T) + "\n"
        run = subprocess.run([EXE], input=text, capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        out = run.stdout.split("\n")
        assert out[0] == "I 0", f"{what}: coords(identity, 0) is not the input: {out[0]}"
        li, worst, differ = 1, 0, 0
        for k_eval, (flags, h, Y) in enumerate(trace):
            tag, fl, hh = out[li].split()
            li += 1
            assert tag == "E" and int(fl) == flags and float.fromhex(hh) == h, f"{what}, evaluation {k_eval}: program {out[li - 1]!r}, numpy {flags} {h!r}"
            if Y is None:
                continue
            b = np.array([[int(v, 16) for v in out[li + i].split()] for i in range(len(x0))], np.uint32)
            li += len(x0)
            ulp = np.abs(b.view(np.int32).astype(np.int64) - Y.view(np.int32).astype(np.int64))
            assert ulp.max() <= 2, f"{what}, evaluation {k_eval}: trial coordinates differ by {ulp.max()} fp32 ulp"
            worst, differ = max(worst, int(ulp.max())), differ + int((ulp != 0).sum())
        assert out[li].split() == ["R", str(res["status"]), str(res["evals"])], (what, out[li], res["status"], res["evals"])
        qt = np.array([float.fromhex(v) for v in out[li + 1].split()])
        assert np.abs(qt - np.concatenate([res["q"], res["t"]])).max() <= 1e-12
        decisions = [t[0] for t in trace]
        print(f"{what}: {res['evals']} evaluations, {decisions.count(P.STORE)} accepts, {decisions.count(0)} rejects, status {res['status']}, "
              f"{differ} coordinates not bit-equal, worst {worst} ulp")
        assert decisions.count(P.STORE) >= 3 and decisions.count(0) >= 3, f"{what}: the run must hold accepts and rejects: {decisions}"
        if len(x0) == 1:
            assert np.array_equal(res["q"], [1.0, 0.0, 0.0, 0.0]), "one atom does not rotate"
        # the body stayed rigid and went downhill
        d0 = np.linalg.norm(x[:, None] - x[None], axis=2)
        y = res["pose"].astype(np.float64)
        assert np.abs(np.linalg.norm(y[:, None] - y[None], axis=2) - d0).max() <= 4 * np.spacing(np.float32(np.abs(y).max()))
        assert res["S"] < float(P.synthetic_evaluate(T, k)(x0)[0][0])


def test_the_oracle_driven_loop_keeps_the_caps(orc):
    """The numpy stepper driven by the oracle alone on the poses of the GPU tests (small_complex, SEED_SMALL, 12 evaluations): at most
    2 of the 16 starts and at most 2 of the refined poses lie closer than 1.0 A to the environment, none on the edge of that rule,
    every row sum went down or stayed, and descent moves the ligand away from its clashes rather than into one."""
    s = systems.small_complex()
    g = three_groups(s)
    lo, hi = ligand_range(s)
    pos = orc.wrap(s, s.pos)
    cfg = small_configs()[0]
    poses = rigid_poses(whole(s, pos[lo:hi]), 16, SEED_SMALL)
    ev = oracle_evaluate(orc, s, cfg, g, 3, pos, lo, hi, 1)
    out, rows, rigid, xform, status, evals = P.refine_batch(poses, ev, 12, 0.0, 0.0)
    d0, d1 = min_env_distance(s, pos, lo, hi, poses), min_env_distance(s, pos, lo, hi, out)
    print(f"starts closer than 1.0 A: {(d0 < 1.0).sum()}, refined: {(d1 < 1.0).sum()}; closest to the rule's edge {np.abs(d0 - 1.0).min():.3f} / "
          f"{np.abs(d1 - 1.0).min():.3f} A; evaluations {evals.tolist()}")
    assert (d0 < 1.0).sum() <= MAX_DROPPED and (d1 < 1.0).sum() <= MAX_DROPPED
    assert np.abs(d0 - 1.0).min() >= 0.02 and np.abs(d1 - 1.0).min() >= 0.02, "a pose on the edge of the rule: fp32 positions on the device may flip it"
    start = np.array([float(np.sum(ev(p)[0].astype(np.float64))) for p in poses])
    drop = start - rows.astype(np.float64).sum(1)
    print("decrease of the row sum, kcal/mol:", np.round(drop, 3).tolist())
    assert (drop >= 0).all() and (drop > 0).sum() >= 8 and (evals >= 1).all()
    assert (status == P.MAX_EVALS).all()      # tolerances of 0: nothing converges, and 12 evaluations cannot exhaust the step


def test_the_convergence_parameters_converge_on_the_cpu(orc):
    """CRYSTAL_F_TOL / CRYSTAL_TAU_TOL / CRYSTAL_MAX_EVALS: the oracle-driven loop converges for at least half of the 16 poses, and
    what it calls converged is converged: |F_net| <= f_tol and |tau| <= tau_tol of the oracle's own forces."""
    s, cfg, g, lo, hi = crystal_case()
    pos = orc.wrap(s, s.pos)
    poses = crystal_poses(whole(s, pos[lo:hi]))
    assert (min_env_distance(s, pos, lo, hi, poses) >= 1.0).all()
    ev = oracle_evaluate(orc, s, cfg, g, 2, pos, lo, hi, 1)
    out, rows, rigid, xform, status, evals = P.refine_batch(poses, ev, CRYSTAL_MAX_EVALS, CRYSTAL_F_TOL, CRYSTAL_TAU_TOL)
    conv = status == P.CONVERGED
    print(f"{int(conv.sum())} of 16 converged, status {status.tolist()}, evaluations {evals.tolist()}")
    assert conv.sum() >= 8
    assert (min_env_distance(s, pos, lo, hi, out) >= 1.0).all()
    for k in np.flatnonzero(conv):
        assert np.linalg.norm(rigid[k, :3]) <= CRYSTAL_F_TOL and np.linalg.norm(rigid[k, 3:]) <= CRYSTAL_TAU_TOL
