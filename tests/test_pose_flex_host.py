"""`mdx_refine_poses_flex` without a GPU: the declarations, the argument, option and flag checks that run before any device is touched,
the Python-side validation of `MdState.refine_poses_flex`, the stepper header (molchanica_amd/csrc/mdx_flex_step.h, the code the step
kernel runs) compiled into a stand-alone host program and held against the numpy restatement of tests/pose_flex_ref.py - stepper,
moving sides, dihedral terms -, that restatement against the fp64 oracle (torsion gradient = minus the derivative of the objective;
dihedral energy and forces), and the start poses of tests/test_gpu_pose_flex.py against their clash conditions."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from molchanica_amd import _abi, systems
from tests import pose_flex_ref as F
from tests import pose_force_ref as R
from tests import pose_refine_ref as P
from tests.test_gpu_pose_batch import MAX_DROPPED, ligand_range, min_env_distance, small_configs, three_groups, whole
from tests.test_pose_refine_host import _rot, oracle_evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")
OUT = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT, "pose_flex_driver")

# Start poses of tests/test_gpu_pose_flex.py on small_complex: rigid_poses(SEED) with the 31 torsions of the ligand then turned by
# AMP u w^2 (pose_flex_ref.flex_poses).  Chosen on the CPU: test_the_start_poses_keep_their_conditions asserts what they were chosen for.
SEED, AMP = 21, 0.3
INTRA_MIN = 1.6


def hx(v):
    return float(v).hex()


def ligand_case():
    """-> (system, lo, hi, ligand-local bonds, torsion bonds [31, 2], moving sides, dihedral terms) of small_complex with root 0"""
    s = systems.small_complex()
    lo, hi = ligand_range(s)
    bonds = F.local_bonds(s, lo, hi)
    tb = F.rotatable_bonds(hi - lo, bonds, 0)
    return s, lo, hi, bonds, tb, F.moving_sides(hi - lo, bonds, 0, tb), F.dihedral_terms(s, lo, hi)


def start_poses(s, pos, lo, hi, tors, n=16):
    return F.flex_poses(whole(s, pos[lo:hi]), tors, n, SEED, AMP)


def intra_excluded(s, lo, hi):
    """[count, count] bool: pairs of the range that are excluded or scaled 1-4 pairs (and the diagonal)"""
    n = hi - lo
    ex = np.eye(n, dtype=bool)
    off, idx = np.asarray(s.excl_offsets), np.asarray(s.excl_idx)
    for i in range(lo, hi):
        for j in idx[off[i]:off[i + 1]]:
            if lo <= j < hi:
                ex[i - lo, j - lo] = ex[j - lo, i - lo] = True
    for a, b in np.asarray(s.pairs14_idx).reshape(-1, 2):
        if lo <= a < hi and lo <= b < hi:
            ex[a - lo, b - lo] = ex[b - lo, a - lo] = True
    return ex


def min_intra_distance(ex, poses):
    out = []
    for p in np.asarray(poses, np.float64):
        out.append(np.linalg.norm(p[:, None] - p[None], axis=2)[~ex].min())
    return np.array(out)


def oracle_flex_evaluate(orc, s, cfg, g, n_groups, pos, lo, hi, lig_group):
    """`evaluate` of the numpy flexible stepper from the oracle alone: oracle_evaluate of the rigid tests plus the per-atom forces"""
    rigid_ev = oracle_evaluate(orc, s, cfg, g, n_groups, pos, lo, hi, lig_group)
    s_nb = R.nonbonded_only(s)

    def evaluate(Y):
        row, rigid = rigid_ev(Y)
        fo = orc.forces(s_nb, cfg, pos=R.full_set(pos, lo, hi, Y), use_cells=True)[0][lo:hi]
        return row, rigid, fo.astype(np.float32)
    return evaluate


def dihedral_only(s, lo, hi):
    """A copy of the system whose only bonded terms are the dihedral terms inside [lo, hi)"""
    idx = np.asarray(s.dihedral_idx).reshape(-1, 4)
    keep = ((idx >= lo) & (idx < hi)).all(1)
    return dataclasses.replace(R.nonbonded_only(s), dihedral_idx=np.ascontiguousarray(idx[keep], np.uint32),
                               dihedral_v=np.ascontiguousarray(np.asarray(s.dihedral_v)[keep], np.float32),
                               dihedral_phase=np.ascontiguousarray(np.asarray(s.dihedral_phase)[keep], np.float32),
                               dihedral_n=np.ascontiguousarray(np.asarray(s.dihedral_n)[keep], np.int32))


def oracle_dihedral(orc, s, cfg, pos, lo, hi, pose):
    """-> (energy, forces [count, 3]) of the ligand's dihedral terms by the oracle: the system with them alone minus the one without"""
    x = R.full_set(pos, lo, hi, pose)
    f1, e1 = orc.forces(dihedral_only(s, lo, hi), cfg, pos=x, use_cells=True)
    f0, _ = orc.forces(R.nonbonded_only(s), cfg, pos=x, use_cells=True)
    return e1["dihedral"], (f1 - f0)[lo:hi]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    l = C.CDLL(LIB)
    l.mdx_last_error.restype = C.c_char_p
    return l


@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "molchanica_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "pose_flex_driver.cpp"), "-o", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def run_driver(exe, text):
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    return run.stdout.split("\n")


def test_header_declares_the_export():
    src = open(os.path.join(ROOT, "include", "mdx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mdx_refine_poses_flex\s*\(([^;]*)\)\s*;", code)
    assert m, "mdx.h does not declare mdx_refine_poses_flex"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 18 and args[0].startswith("mdx_handle") and args[4].startswith("const float") and args[5] == "uint32_t root"
    assert args[6] == "uint32_t n_torsions" and args[7].startswith("const uint32_t*") and args[8].startswith("const mdx_flex_opts")
    assert args[9].startswith("float") and args[16].startswith("uint32_t*") and args[17].startswith("uint32_t*")
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+max_evals;\s*float\s+f_tol,\s*tau_tol,\s*tors_tol,\s*h_start,\s*h_max;\s*uint32_t\s+flags;\s*\}\s*mdx_flex_opts;", code)
    cap = re.search(r"#define\s+MDX_POSE_MAX_TORSIONS\s+(\d+)u?\b", code)
    assert cap and int(cap.group(1)) == _abi.POSE_MAX_TORSIONS == F.MAX_TORSIONS
    flag = re.search(r"#define\s+MDX_FLEX_DIHEDRALS\s+(\d+)u?\b", code)
    assert flag and int(flag.group(1)) == _abi.FLEX_DIHEDRALS
    assert C.sizeof(_abi.CFlexOpts) == 28
    comment = src[src.index("flexible refinement: the same descent"):src.index("#define MDX_POSE_MAX_TORSIONS")]
    for must in ("nested or disjoint", "a ring bond", "a leaf bond", "bit for bit", "tors_tol", "list order", "g_k", "1e-6 J_k", "theta_try"):
        assert must in comment, must
    assert "so the refinement is rigid;" not in src      # the sentence that called flexible refinement out of scope
    assert re.search(r"\brefine_poses_flex\s*\(", open(os.path.join(ROOT, "include", "mdx.hpp")).read())
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    assert "pub fn mdx_refine_poses_flex" in blk[:blk.index("\n}\n")]
    step = open(os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_flex_step.h")).read()
    assert int(re.search(r"#define\s+MDX_FX_MAX_TORSIONS\s+(\d+)u", step).group(1)) == _abi.POSE_MAX_TORSIONS
    for name in ("ROOT", "INDEX", "SELF", "NOT_BONDED", "TWICE", "RING", "LEAF", "DISCONNECTED"):
        assert int(re.search(rf"#define\s+MDX_FX_E_{name}\s+(\d+)", step).group(1)) == getattr(F, "E_" + name)


def test_null_arguments_options_and_flags_are_rejected_before_any_device_is_touched(lib):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    lib.mdx_refine_poses_flex.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, fp, C.c_uint32, C.c_uint32, up,
                                          C.POINTER(_abi.CFlexOpts), fp, fp, C.c_uint32, fp, fp, fp, fp, up, up]
    poses = np.zeros((2, 4, 3), np.float32)
    tb = np.array([[1, 2]], np.uint32)
    out = [np.full((2, 4, 3), -7.0, np.float32), np.full((2, 3), -7.0, np.float32), np.full((2, 6), -7.0, np.float32),
           np.full((2, 8), -7.0, np.float32), np.full(2, -7.0, np.float32), np.full((2, 1), -7.0, np.float32)]
    st, ev = np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    p = lambda a: a.ctypes.data_as(fp)
    good = _abi.CFlexOpts(12, 0.1, 0.1, 0.1, 0.0, 0.0, 1)

    def call(h, opts, poses_out=True, poses_in=True, n_tors=1, bonds=True):
        return lib.mdx_refine_poses_flex(h, 0, 4, 2, p(poses) if poses_in else None, 0, n_tors, tb.ctypes.data_as(up) if bonds else None,
                                         C.byref(opts) if opts is not None else None, p(out[0]) if poses_out else None, p(out[1]), 3,
                                         p(out[2]), p(out[3]), p(out[4]), p(out[5]), st.ctypes.data_as(up), ev.ctypes.data_as(up))
    assert call(None, good) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error()
    # a handle that is not null: refused on the arguments alone (the pointer is never followed)
    fake = C.create_string_buffer(64)
    h = C.addressof(fake)
    for kw in (dict(opts=None), dict(opts=good, poses_out=False), dict(opts=good, poses_in=False), dict(opts=good, bonds=False)):
        assert call(h, **kw) == _abi.MDX_EPARAM and b"null" in lib.mdx_last_error(), kw
    assert call(h, good, n_tors=_abi.POSE_MAX_TORSIONS + 1) == _abi.MDX_EPARAM and b"MDX_POSE_MAX_TORSIONS" in lib.mdx_last_error()
    O = _abi.CFlexOpts
    for bad, match in ((O(0, 0.1, 0.1, 0.1, 0, 0, 0), b"max_evals"), (O(_abi.REFINE_MAX_EVALS_CAP + 1, 0.1, 0.1, 0.1, 0, 0, 0), b"max_evals"),
                       (O(12, -0.1, 0.1, 0.1, 0, 0, 0), b"negative"), (O(12, 0.1, float("nan"), 0.1, 0, 0, 0), b"not finite"),
                       (O(12, 0.1, 0.1, -1.0, 0, 0, 0), b"negative"), (O(12, 0.1, 0.1, float("nan"), 0, 0, 0), b"not finite"),
                       (O(12, 0.1, 0.1, float("inf"), 0, 0, 1), b"not finite"),
                       (O(12, 0.1, 0.1, 0.1, float("inf"), 0, 0), b"not finite"), (O(12, 0.1, 0.1, 0.1, 0, -1.0, 0), b"negative"),
                       (O(12, 0.1, 0.1, 0.1, 0.3, 0.25, 0), b"h_start"), (O(12, 0.1, 0.1, 0.1, 0.3, 0.0, 0), b"h_start"),
                       (O(12, 0.1, 0.1, 0.1, 0.0, 0.005, 0), b"h_start"),
                       (O(12, 0.1, 0.1, 0.1, 0, 0, 2), b"flag"), (O(12, 0.1, 0.1, 0.1, 0, 0, 0x80000001), b"flag")):
        assert call(h, bad) == _abi.MDX_EPARAM
        assert match in lib.mdx_last_error(), (match, lib.mdx_last_error())
    assert all((o == -7.0).all() for o in out) and (st == 77).all() and (ev == 77).all()
    # n_poses == 0 succeeds and does nothing, whatever else is passed
    assert lib.mdx_refine_poses_flex(h, 0, 4, 0, None, 0, 0, None, None, None, None, 3, None, None, None, None, None, None) == 0
    assert lib.mdx_refine_poses_flex(None, 0, 4, 0, None, 0, 0, None, None, None, None, 3, None, None, None, None, None, None) == _abi.MDX_EPARAM


def test_python_wrapper_validates_shape_and_dtype():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    tb = np.array([[1, 2]], np.uint32)
    for bad in (np.zeros((2, 5, 3), np.float64), np.zeros((5, 3), np.float32), np.zeros((2, 5, 4), np.float32),
                np.zeros((2, 0, 3), np.float32), np.zeros((1, 257, 3), np.float32), [[[0.0, 0.0, 0.0]]]):
        with pytest.raises(ParamError):
            md.refine_poses_flex(0, bad, 0, tb, 12, 0.1, 0.1, 0.1)
    ok = np.zeros((1, 5, 3), np.float32)
    for first in (98, -1):
        with pytest.raises(ParamError):
            md.refine_poses_flex(first, ok, 0, tb, 12, 0.1, 0.1, 0.1)
    for bad_tb in (np.array([1, 2], np.uint32), np.array([[1, 2, 3]], np.uint32), np.array([[1.0, 2.0]]), np.array([[1, 5]], np.uint32),
                   np.array([[-1, 2]], np.int64), np.tile(tb, (33, 1))):
        with pytest.raises(ParamError):
            md.refine_poses_flex(0, ok, 0, bad_tb, 12, 0.1, 0.1, 0.1)
    for root in (5, -1):
        with pytest.raises(ParamError):
            md.refine_poses_flex(0, ok, root, tb, 12, 0.1, 0.1, 0.1)


def _graph_text(count, root, bonds, tb):
    bonds, tb = np.asarray(bonds, np.int64).reshape(-1, 2), np.asarray(tb, np.int64).reshape(-1, 2)
    return f"{count} {root} {len(bonds)} {len(tb)}\n" + "".join(f"{p} {q}\n" for p, q in bonds) + "".join(f"{p} {q}\n" for p, q in tb)


def test_moving_sides_of_the_header_are_those_of_numpy(driver):
    """lig50 with root 0: a tree of 50 atoms, 31 bonds with both ends of degree >= 2, moving sides of 2 to 42 atoms; a different root
    turns the other side of the bonds on the path between the two roots."""
    s = systems.lig50()
    n = s.n_atoms
    bonds = F.local_bonds(s, 0, n)
    assert len(bonds) == n - 1
    tb = F.rotatable_bonds(n, bonds, 0)
    deg = np.bincount(bonds.reshape(-1), minlength=n)
    assert len(tb) == 31 == int(((deg[bonds[:, 0]] >= 2) & (deg[bonds[:, 1]] >= 2)).sum())
    for root in (0, 17, 49):
        tors = F.moving_sides(n, bonds, root, tb)
        out = run_driver(driver, "G " + _graph_text(n, root, bonds, tb))
        assert out[0] == "M 0 0"
        for k, (a, b, mask) in enumerate(tors):
            w = out[1 + k].split()
            bits = np.array([(int(w[2 + (i >> 5)], 16) >> (i & 31)) & 1 for i in range(256)], bool)
            assert (int(w[0]), int(w[1])) == (a, b) and np.array_equal(bits[:n], mask) and not bits[n:].any(), (root, k)
            assert mask[b] and not mask[a] and not mask[root] and {a, b} == set(map(int, tb[k]))
        if root == 0:
            sizes = sorted(int(m.sum()) for _, _, m in tors)
            assert sizes[0] == 2 and sizes[-1] == 42
            # nested or disjoint
            for _, _, m1 in tors:
                for _, _, m2 in tors:
                    both = int((m1 & m2).sum())
                    assert both in (0, int(m1.sum()), int(m2.sum()))


def test_every_graph_rule_is_refused_by_the_header_and_by_numpy(driver):
    # 0-1-2-3-4-5 with a three-membered ring 2-3-6 and a leaf 7 on atom 1
    bonds = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (2, 6), (3, 6), (1, 7)]
    n = 8
    cases = (([(1, 2)], 0, F.E_ROOT, 0, dict(root=8)), ([(1, 2), (3, 9)], 0, F.E_INDEX, 1, {}), ([(1, 2), (3, 3)], 0, F.E_SELF, 1, {}),
             ([(1, 3)], 0, F.E_NOT_BONDED, 0, {}), ([(3, 4), (1, 2), (4, 3)], 0, F.E_TWICE, 2, {}), ([(1, 2), (2, 3)], 0, F.E_RING, 1, {}),
             ([(2, 6)], 0, F.E_RING, 0, {}), ([(3, 4), (4, 5)], 0, F.E_LEAF, 1, {}), ([(0, 1)], 3, F.E_LEAF, 0, {}), ([(1, 7)], 0, F.E_LEAF, 0, {}),
             ([(1, 2)], 0, F.E_DISCONNECTED, 0, dict(bonds=bonds + [(8, 9)], n=10)))
    for tb, root, code, bad, kw in cases:
        b, cnt, root = kw.get("bonds", bonds), kw.get("n", n), kw.get("root", root)
        with pytest.raises(F.GraphError) as e:
            F.moving_sides(cnt, b, root, tb)
        assert (e.value.code, e.value.torsion) == (code, bad), (tb, e.value.code, e.value.torsion)
        assert run_driver(driver, "G " + _graph_text(cnt, root, b, tb))[0] == f"M {code} {bad}", tb
    # what is left: the two bonds that split the molecule properly, from either side
    for root in (0, 5):
        tors = F.moving_sides(n, bonds, root, [(1, 2), (4, 3)])
        assert run_driver(driver, "G " + _graph_text(n, root, bonds, [(1, 2), (4, 3)]))[0] == "M 0 0"
        assert [int(m.sum()) for _, _, m in tors] == ([5, 2] if root == 0 else [3, 6])
    # no torsion: nothing is asked of the graph but the root
    assert F.moving_sides(10, bonds + [(8, 9)], 0, []) == []
    assert run_driver(driver, "G " + _graph_text(10, 0, bonds + [(8, 9)], []))[0] == "M 0 0"


def _stepper_text(x0, T, k, evals, f_tol, tau_tol, tors_tol, h_start, h_max, root, bonds, tb):
    text = f"S {len(x0)} {hx(k)} {evals} " + " ".join(hx(np.float32(v)) for v in (f_tol, tau_tol, tors_tol, h_start, h_max))
    text += f" {root} {len(bonds)} {len(tb)}\n"
    text += "\n".join(" ".join(hx(v) for v in row) for row in x0) + "\n" + "\n".join(" ".join(hx(v) for v in row) for row in T) + "\n"
    return text + "".join(f"{p} {q}\n" for p, q in bonds) + "".join(f"{p} {q}\n" for p, q in tb)


def _against_the_driver(exe, what, x0, T, k, evals, tols, h_start, h_max, bonds, tb):
    tors = F.moving_sides(len(x0), bonds, 0, tb)
    trace = []
    res = F.refine(x0, F.synthetic_evaluate(T, k), tors, F.NO_TERMS, evals, tols[0], tols[1], tols[2], h_start, h_max, trace=trace)
    out = run_driver(exe, _stepper_text(x0, T, k, evals, tols[0], tols[1], tols[2], h_start, h_max, 0, bonds, tb))
    assert out[0] == "I 0", f"{what}: coords(identity, 0, 0) is not the input: {out[0]}"
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
    assert np.abs(qt - np.concatenate([res["q"], res["t"], res["theta"]])).max() <= 1e-10
    decisions = [t[0] for t in trace]
    print(f"{what}: {res['evals']} evaluations, {decisions.count(P.STORE)} accepts, {decisions.count(0)} rejects, status {res['status']}, "
          f"S {res['S']:.4g}, {differ} coordinates not bit-equal, worst {worst} ulp")
    return res, decisions


def test_the_stepper_header_as_a_host_program_matches_the_numpy_stepper(driver):
    """mdx_flex_step.h compiled by the host compiler into tests/cpp/pose_flex_driver.cpp, against tests/pose_flex_ref.py.  The
    ligand of systems.lig50 at coordinates of 15 - 30 A; the target is the ligand with its 31 torsions turned (up to 0.5 rad), then
    rotated by 0.4 rad and shifted; a quadratic field (k = 2) pulls every atom to its target, h_start 0.05 A and h_max 1 A so that the
    step overshoots.  Per evaluation the decision and the step length must be equal and the next trial's coordinates agree within
    2 fp32 ulp; so must status, evaluation count and the accepted (q, t, theta).  400 evaluations: the flexible run ends below 1 % of the
    starting S (measured: 514.2 -> 0.0028, 316 accepts and 84 rejects), the rigid run on the same field stalls above it (54.8)."""
    s = systems.lig50()
    n = s.n_atoms
    bonds = F.local_bonds(s, 0, n)
    tb = F.rotatable_bonds(n, bonds, 0)
    tors = F.moving_sides(n, bonds, 0, tb)
    x0 = (np.asarray(s.pos, np.float64) + [20.0, 15.0, 25.0]).astype(np.float32)
    rng = np.random.default_rng(5)
    T = F.turn(x0.astype(np.float64), tors, 0.5 * rng.uniform(-1, 1, len(tors)))
    c = T.mean(0)
    T = (T - c) @ _rot([1, 2, 3], 0.4).T + c + [0.6, -0.3, 0.4]
    k, evals, tols, h_start, h_max = 2.0, 400, (1e-3, 1e-3, 1e-3), 0.05, 1.0
    S0 = float(F.synthetic_evaluate(T, k)(x0)[0][0])
    flex, d = _against_the_driver(driver, "31 torsions", x0, T, k, evals, tols, h_start, h_max, bonds, tb)
    assert d.count(P.STORE) >= 3 and d.count(0) >= 3, f"the run must hold accepts and rejects: {d}"
    assert flex["S"] < 0.01 * S0, (flex["S"], S0)
    assert np.abs(flex["theta"]).max() > 0.05
    rigid, d0 = _against_the_driver(driver, "no torsion", x0, T, k, evals, tols, h_start, h_max, bonds, np.zeros((0, 2), np.uint32))
    assert d0.count(P.STORE) >= 3 and d0.count(0) >= 3
    assert rigid["S"] > 0.01 * S0, (rigid["S"], S0)
    # with no torsion the flexible stepper is the rigid one, decision by decision and bit by bit
    trace_f, trace_r = [], []
    a = F.refine(x0, F.synthetic_evaluate(T, k), [], F.NO_TERMS, evals, *tols, h_start, h_max, trace=trace_f)
    b = P.refine(x0, P.synthetic_evaluate(T, k), evals, tols[0], tols[1], h_start, h_max, trace=trace_r)
    assert len(trace_f) == len(trace_r) and a["status"] == b["status"] and np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32))
    for (f1, h1, y1), (f2, h2, y2) in zip(trace_f, trace_r):
        assert f1 == f2 and h1 == h2 and (y1 is None) == (y2 is None) and (y1 is None or np.array_equal(y1.view(np.uint32), y2.view(np.uint32)))
    # a subset of 8 torsions, listed in another order, and a shape of the flexible run: every bond length within fp32 rounding
    sub = tb[[20, 3, 11, 29, 7, 0, 16, 25]]
    _against_the_driver(driver, "8 torsions out of order", x0, T, k, 60, tols, h_start, h_max, bonds, sub)
    y, x = flex["pose"].astype(np.float64), x0.astype(np.float64)
    bl = lambda z: np.linalg.norm(z[bonds[:, 0]] - z[bonds[:, 1]], axis=1)
    assert np.abs(bl(y) - bl(x)).max() <= 4 * np.spacing(np.float32(np.abs(y).max()))


def test_the_driver_under_the_sanitizers(driver):
    """The same stand-alone host program built with -fsanitize=address,undefined and run once on a short case of each mode."""
    exe = EXE + "_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "molchanica_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pose_flex_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    s = systems.lig50()
    n = s.n_atoms
    bonds = F.local_bonds(s, 0, n)
    tb = F.rotatable_bonds(n, bonds, 0)
    tors = F.moving_sides(n, bonds, 0, tb)
    x0 = (np.asarray(s.pos, np.float64) + [20.0, 15.0, 25.0]).astype(np.float32)
    T = F.turn(x0.astype(np.float64), tors, np.full(len(tors), 0.2)) + [0.3, 0.0, -0.2]
    out = run_driver(exe, _stepper_text(x0, T, 2.0, 30, 1e-3, 1e-3, 1e-3, 0.05, 1.0, 0, bonds, tb))
    assert out[0] == "I 0" and any(l.startswith("R ") for l in out)
    assert run_driver(exe, "G " + _graph_text(n, 0, bonds, tb))[0] == "M 0 0"
    assert run_driver(exe, "G " + _graph_text(n, 0, bonds, [(0, 0)]))[0].startswith("M ")
    at, v, ph, nn = F.dihedral_terms(s, 0, n)
    text = f"D {n} {len(at)} 0x0p+0 0x0p+0 0x0p+0\n" + "\n".join(" ".join(hx(c) for c in row) for row in x0) + "\n"
    text += "".join(" ".join(str(int(i)) for i in a) + f" {hx(b)} {hx(c)} {hx(d)}\n" for a, b, c, d in zip(at, v, ph, nn))
    assert run_driver(exe, text)[0].startswith("E ")


def test_the_dihedral_terms_of_the_header_of_numpy_and_of_the_oracle_agree(driver, orc):
    """E_dih and f^dih of the ligand of small_complex at the 16 start poses: the restatement against the fp64 oracle (the system with
    the ligand's dihedral terms alone minus the system without) and against the header, bound 1e-9 x sum 2 |v| (kcal/mol, and
    kcal/mol/A per atom).  Measured: 0 / 4.9e-13 off the oracle, 0 / 1.5e-14 off the header, of a bound of 1.7e-7."""
    s, lo, hi, bonds, tb, tors, terms = ligand_case()
    pos = orc.wrap(s, s.pos)
    cfg = small_configs()[0]
    poses = start_poses(s, pos, lo, hi, tors)
    at, v, ph, nn = terms
    assert len(at) > 50 and (np.asarray(s.dihedral_idx).reshape(-1, 4) < lo).all(1).any(), "the chain has dihedral terms too: they must be left out"
    bound = 1e-9 * float((2.0 * np.abs(v)).sum())
    box = np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in (0, 3, 9, 15):
        E, f = F.dihedral(poses[k], terms, box)
        Eo, fo = oracle_dihedral(orc, s, cfg, pos, lo, hi, poses[k])
        text = f"D {hi - lo} {len(at)} " + " ".join(hx(b) for b in box) + "\n" + "\n".join(" ".join(hx(c) for c in row) for row in poses[k]) + "\n"
        text += "".join(" ".join(str(int(i)) for i in a) + f" {hx(b)} {hx(c)} {hx(d)}\n" for a, b, c, d in zip(at, v, ph, nn))
        out = run_driver(driver, text)
        Ed = float.fromhex(out[0].split()[1])
        fd = np.array([[float.fromhex(c) for c in out[1 + i].split()] for i in range(hi - lo)])
        worst = [max(worst[0], abs(E - Eo)), max(worst[1], float(np.abs(f - fo).max())), max(worst[2], abs(E - Ed)), max(worst[3], float(np.abs(f - fd).max()))]
        assert abs(f.sum(0)).max() <= bound and abs(np.cross(poses[k].astype(np.float64), f).sum(0)).max() <= 100 * bound      # no net force, no torque
        assert E > 0 and np.abs(f).max() > 0.1
    print(f"restated dihedral terms: energy {worst[0]:.1e}, force {worst[1]:.1e} off the oracle; {worst[2]:.1e} / {worst[3]:.1e} off the header; bound {bound:.1e}")
    assert max(worst) <= bound


def test_the_torsion_gradient_is_minus_the_derivative_of_the_objective(orc):
    """g_k of the restatement = -dS/dtheta_k by central differences (1e-5 rad) of the restated objective in its own coordinates,
    S(theta) = the sum of the oracle's ligand row + the oracle's dihedral energy of the ligand's terms at c0 + t + R(q) (B(theta) -
    mean B(theta)) in fp64, small_complex, start poses 3 and 9 at small non-zero (q, t, theta), ten of the 31 torsions.  Bound: 1e-6 of
    max(|central difference|, 1), that of tests/test_pose_forces_host.py for the per-atom forces.  Measured worst: 3.3e-8, on gradients of 0.9 to 9900 kcal/mol/rad."""
    s, lo, hi, bonds, tb, tors, terms = ligand_case()
    g3 = three_groups(s)
    pos = orc.wrap(s, s.pos)
    cfg = small_configs()[0]
    poses = start_poses(s, pos, lo, hi, tors)
    s_nb, s_dih = R.nonbonded_only(s), dihedral_only(s, lo, hi)
    rng = np.random.default_rng(9)
    h = 1e-5
    worst, gmin, gmax = 0.0, np.inf, 0.0
    for k in (3, 9):
        x0 = poses[k].astype(np.float64)
        c0 = x0.mean(0)
        theta0 = 0.05 * rng.uniform(-1, 1, len(tors))
        Rq = _rot(rng.normal(size=3), 0.03)
        t = rng.normal(size=3) * 0.05

        def image(theta):
            B = F.turn(x0, tors, theta)
            return c0 + t + (B - B.mean(0)) @ Rq.T

        def S(theta):
            x = R.full_set(pos, lo, hi, image(theta))
            return orc.between_mols(s, cfg, g3, 3, pos=x, use_cells=True)[0][1].sum() + orc.forces(s_dih, cfg, pos=x, use_cells=True)[1]["dihedral"]

        Y = image(theta0)
        x = R.full_set(pos, lo, hi, Y)
        f = orc.forces(s_dih, cfg, pos=x, use_cells=True)[0][lo:hi]      # non-bonded + the ligand's dihedral terms
        f_nb = orc.forces(s_nb, cfg, pos=x, use_cells=True)[0][lo:hi]
        g, J, A, U = F.gradient(Y, f, f_nb.sum(0) / float(hi - lo), tors)
        for j in (0, 4, 8, 12, 17, 20, 23, 26, 29, 30):
            e = []
            for sign in (1.0, -1.0):
                th = theta0.copy()
                th[j] += sign * h
                e.append(S(th))
            fd = -(e[0] - e[1]) / (2 * h)
            rel = abs(g[j] - fd) / max(abs(fd), 1.0)
            worst, gmin, gmax = max(worst, rel), min(gmin, abs(g[j])), max(gmax, abs(g[j]))
            assert rel <= 1e-6, (k, j, g[j], fd, rel)
    print(f"torsion gradient against the central difference of the objective: worst relative difference {worst:.1e} on gradients of "
          f"{gmin:.3g} to {gmax:.3g} kcal/mol/rad")


def test_the_start_poses_keep_their_conditions(orc):
    """What SEED and AMP were chosen for, so that the GPU tests cannot hide behind dropped poses: at most MAX_DROPPED of the 16 start
    poses lie closer than 1.0 A to the environment, none within 0.02 A of that rule's edge, no intra-ligand pair that is neither
    excluded nor a 1-4 pair is closer than 1.6 A - and the same after 12 evaluations of the numpy stepper driven by the oracle, with the
    dihedral terms and without.  Pose 0 is the start."""
    s, lo, hi, bonds, tb, tors, terms = ligand_case()
    g3 = three_groups(s)
    pos = orc.wrap(s, s.pos)
    cfg = small_configs()[0]
    poses = start_poses(s, pos, lo, hi, tors)
    assert np.array_equal(poses[0], whole(s, pos[lo:hi]).astype(np.float32)) and len(tors) == 31
    ex = intra_excluded(s, lo, hi)
    ev = oracle_flex_evaluate(orc, s, cfg, g3, 3, pos, lo, hi, 1)

    def conditions(p, what):
        d, it = min_env_distance(s, pos, lo, hi, p), min_intra_distance(ex, p)
        print(f"{what}: {(d < 1.0).sum()} closer than 1.0 A, closest to the rule's edge {np.abs(d - 1.0).min():.3f} A, closest intra-ligand pair {it.min():.3f} A")
        assert (d < 1.0).sum() <= MAX_DROPPED and np.abs(d - 1.0).min() >= 0.02 and it.min() >= INTRA_MIN
    conditions(poses, "starts")
    for what, tm in (("with the dihedral terms", terms), ("without", F.NO_TERMS)):
        out = F.refine_batch(poses, ev, tors, tm, 12, 0.0, 0.0, 0.0)
        conditions(out[0], f"after 12 evaluations {what}")
        S0 = np.array([float(ev(p)[0].astype(np.float64).sum()) + float(np.float32(F.dihedral(p, tm)[0])) for p in poses])
        drop = S0 - (out[1].astype(np.float64).sum(1) + out[4].astype(np.float64))
        print("decrease of the objective, kcal/mol:", np.round(drop, 3).tolist())
        assert (drop >= 0).all() and (drop > 0).sum() >= 8 and (out[6] == P.MAX_EVALS).all()
        assert np.abs(out[3][:, 7:]).max() > 1e-3, "the torsions must have moved"
