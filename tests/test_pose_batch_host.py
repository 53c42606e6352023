"""`mdx_score_poses` without a GPU: the declaration, the argument checks that run before any device is touched, the Python-side
validation of `MdState.score_poses`, and the pose seeds of tests/test_gpu_pose_batch.py against its 1.0 A clash rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from molchanica_amd import _abi, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "molchanica_amd", "libmdx.so")


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
    assert re.search(r"\bint\s+mdx_score_poses\s*\(\s*mdx_handle\s*\*", code)
    m = re.search(r"#define\s+MDX_POSE_MAX_ATOMS\s+(\d+)", code)
    assert m and int(m.group(1)) == 256 == _abi.POSE_MAX_ATOMS
    assert "mdx_score_poses" in open(os.path.join(ROOT, "include", "mdx.hpp")).read()
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = txt[txt.index('extern "C" {'):]
    assert "pub fn mdx_score_poses" in blk[:blk.index("\n}\n")]


def test_null_arguments_are_rejected_before_any_device_is_touched(lib):
    fp = C.POINTER(C.c_float)
    lib.mdx_score_poses.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, fp, fp, C.c_uint32]
    poses = np.zeros((2, 4, 3), np.float32)
    out = np.full((2, 3), -7.0, np.float32)
    assert lib.mdx_score_poses(None, 0, 4, 2, poses.ctypes.data_as(fp), out.ctypes.data_as(fp), 3) == _abi.MDX_EPARAM
    assert b"null" in lib.mdx_last_error()
    assert lib.mdx_score_poses(None, 0, 4, 2, None, None, 3) == _abi.MDX_EPARAM
    assert lib.mdx_score_poses(None, 0, 4, 0, None, None, 3) == _abi.MDX_EPARAM
    assert (out == -7.0).all()


def test_python_wrapper_validates_shape_and_dtype():
    from molchanica_amd.md_state import MdState, ParamError
    md = MdState.__new__(MdState)      # no handle: the checks below must fire before the library is asked anything
    md._h = C.c_void_p()
    md.n_atoms = 100
    for bad in (np.zeros((2, 5, 3), np.float64),          # dtype
                np.zeros((5, 3), np.float32),             # one pose without the batch axis
                np.zeros((2, 5, 4), np.float32),          # not xyz
                np.zeros((2, 0, 3), np.float32),          # empty ligand
                np.zeros((1, 257, 3), np.float32),        # above MDX_POSE_MAX_ATOMS
                [[[0.0, 0.0, 0.0]]]):                     # not an ndarray
        with pytest.raises(ParamError):
            md.score_poses(0, bad)
    with pytest.raises(ParamError):
        md.score_poses(98, np.zeros((1, 5, 3), np.float32))      # range beyond the atoms
    with pytest.raises(ParamError):
        md.score_poses(-1, np.zeros((1, 5, 3), np.float32))


def test_pose_seeds_stay_within_the_clash_cap(orc):
    """The seeds of the GPU tests, checked where no GPU is: at most 2 of 16 poses (2 of the 6 sampled at complex50k) bring a ligand
    atom within 1.0 A of the environment.  The start coordinates here are the system's own, wrapped as the handle wraps them."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pose_batch_gpu_tests", os.path.join(ROOT, "tests", "test_gpu_pose_batch.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    s = systems.small_complex()
    lo, hi = t.ligand_range(s)
    pos = orc.wrap(s, s.pos)
    for seed, jitter in ((t.SEED_SMALL, 0.0), (t.SEED_FLEX, 0.05)):
        d = t.min_env_distance(s, pos, lo, hi, t.rigid_poses(t.whole(s, pos[lo:hi]), 16, seed, jitter=jitter))
        print("small_complex seed", seed, "jitter", jitter, np.round(np.sort(d)[:4], 3))
        assert (d < 1.0).sum() <= t.MAX_DROPPED
        assert not np.any(np.abs(d - 1.0) < 0.02), "a pose on the edge of the rule: fp32 positions on the device may flip it"
    s = systems.complex50k()
    lo, hi = t.ligand_range(s)
    pos = orc.wrap(s, s.pos)
    poses = t.rigid_poses(t.whole(s, pos[lo:hi]), 256, t.SEED_50K)
    d = t.min_env_distance(s, pos, lo, hi, poses[list(t.SAMPLED_50K)])
    print("complex50k sampled", np.round(d, 3))
    assert (d < 1.0).sum() <= 2
