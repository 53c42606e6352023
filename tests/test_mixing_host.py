"""The rule of mdx_solubility_mixing on the host: the numpy restatement against the reference's own two pinned vectors and against closed
forms, the conditions the GPU cases rely on, the C struct, and the rule header built into a stand-alone program.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from molchanica_amd import _abi
from tests import mixing_cases as mc
from tests import mixing_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference's own vectors (its tolerance: 1e-3) ---------------------------------------------------------------------------------
PINNED_WANT = {
    # an even grid: every solute has its water at sqrt(3) A and no other solute in reach; no contacts; centres further apart than uniform
    "mixed": dict(score=1.0, raw_score=1.0, local_mixing=1.0, solute_dispersion=1.0, mixture_score=1.0, aggregation_factor=1.0,
                  aggregation_penalty=0.0, largest_cluster_fraction=0.0, contacted_fraction=0.0, contact_pair_fraction=0.0),
    # separate slabs: every sum underflows, so every atom scores 0
    "split": dict(score=0.0, raw_score=0.0, local_mixing=0.0, solute_dispersion=1.0, mixture_score=0.0, aggregation_factor=1.0,
                  aggregation_penalty=0.0, largest_cluster_fraction=0.0, contacted_fraction=0.0, contact_pair_fraction=0.0),
}


@pytest.mark.parametrize("which", ["mixed", "split"])
@pytest.mark.parametrize("scale", [1.0, 1.0 / 64.0])
def test_restatement_reproduces_the_pinned_vectors(which, scale):
    sol, wat, lo, hi, want = mc.pinned(which, scale)
    got = ref.diagnostics(sol, wat, lo, hi)
    assert PINNED_WANT[which]["score"] == want
    for name in ref.FIELDS:
        assert abs(float(got[name]) - PINNED_WANT[which][name]) <= mc.PINNED_EPS, (name, got[name])


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_one_copy_gives_dispersion_one_and_the_default_aggregation():
    c = mc.BY_NAME["one_row"]
    s = c.system()
    sol, wat = c.split(s.pos)
    got = ref.diagnostics(sol, wat, s.box_lo, s.box_hi)
    assert got["solute_dispersion"] == 1.0 and got["aggregation_factor"] == 1.0
    assert got["aggregation_penalty"] == got["largest_cluster_fraction"] == got["contacted_fraction"] == got["contact_pair_fraction"] == 0.0
    # one copy has no other copy: S = 0, every atom scores 2 W' / W' = 1
    assert got["local_mixing"] == 1.0 and got["mixture_score"] == 1.0 and got["score"] == 1.0


def test_two_touching_copies():
    rng = np.random.default_rng(4)
    a = rng.uniform(12.0, 15.0, size=(1, 4, 3))
    sol = np.concatenate([a, a + np.array([3.0, 0.0, 0.0])]).astype(np.float32)
    wat = rng.uniform(0.0, 30.0, size=(50, 3)).astype(np.float32)
    got = ref.diagnostics(sol, wat, (0, 0, 0), (30, 30, 30))
    assert got["largest_cluster_fraction"] == got["contacted_fraction"] == got["contact_pair_fraction"] == 1.0
    assert got["aggregation_penalty"] == 1.0
    assert abs(float(got["aggregation_factor"]) - np.exp(-3.5)) < 1e-7
    # two centres 3 A apart in a 30 A cube: rms 3, uniform rms sqrt(3 * 900 / 12) = 15
    assert abs(float(got["solute_dispersion"]) - 0.2) < 1e-6
    # across a face the same pair still touches
    sol2 = sol.copy()
    sol2[1, :, 0] += 30.0
    got2 = ref.diagnostics(sol2, wat, (0, 0, 0), (30, 30, 30))
    for name in ref.FIELDS:
        assert abs(float(got2[name]) - float(got[name])) < 1e-6, name


def test_sigma_clipping_follows_the_shortest_edge():
    assert list(ref.sigmas(np.array([30.0, 30.0, 30.0]))) == [4.0, 7.0, 10.0]
    s = ref.sigmas(np.array([21.0, 26.0, 30.0]))
    assert s[0] == 4.0 and s[1] == 7.0 and abs(s[2] - 9.45) < 1e-6
    s = ref.sigmas(np.array([15.0, 24.0, 30.0]))
    assert s[0] == 4.0 and abs(s[1] - 6.75) < 1e-6 and abs(s[2] - 6.75) < 1e-6
    assert list(ref.sigmas(np.array([1.5, 30.0, 30.0]))) == [1.0, 1.0, 1.0]


# ---- the conditions the GPU cases rely on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_case_conditions(case):
    s = case.system()
    sol, wat = case.split(s.pos)
    assert sol.shape[0] * sol.shape[1] <= 320 and len(wat) <= 600
    got, ex = ref.diagnostics(sol, wat, s.box_lo, s.box_hi, full=True)
    # no selected-atom pair of two copies within a relative 1e-5 of the contact cutoff in d2
    cut2 = float(np.float32(ref.CONTACT) * np.float32(ref.CONTACT))
    d2 = ex["d2"][ex["other"]]
    assert d2.size == 0 or np.abs(d2 / cut2 - 1.0).min() > 1e-5
    # no S' + W' within a factor 10 of FLT_EPSILON
    dens = ex["S"] + ex["W"]
    assert not ((dens > ref.FLT_EPSILON / 10) & (dens < ref.FLT_EPSILON * 10)).any()
    if case.sharp:      # saturated scores hide a wrong sum
        inside = (ex["scores"] > 0.05) & (ex["scores"] < 0.95)
        assert inside.mean() >= 0.5, inside.mean()
    # the derived bound on local_mixing stays a tenth of the reference's own tolerance
    b = ref.local_mixing_bound(ex["sums"], ref.sum_bounds(sol, wat, s.box_lo, s.box_hi), sol.shape[0], sol.shape[1], len(wat))
    assert b <= 1e-4, b


def test_cases_cover_the_shapes():
    rows = sorted(c.copies * c.n_sel for c in mc.CASES)
    assert {1, 63, 65, 257} <= set(rows)
    assert any(c.apc == 1 for c in mc.CASES) and any(c.copies == 1 for c in mc.CASES) and any(c.sel is not None for c in mc.CASES)
    assert any(min(c.box) < 22.0 and min(c.box) >= 2 * 7.0 / 0.9 for c in mc.CASES)      # only sigma = 10 clipped
    assert any(min(c.box) < 2 * 7.0 / 0.9 for c in mc.CASES)                               # 7 and 10 clipped
    assert any(any(c.origin) for c in mc.CASES) and any(c.faces for c in mc.CASES) and sum(c.sharp for c in mc.CASES) >= 2


# ---- the C side ------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_c(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mdx.h"
int main(void) {
  printf("%zu %zu %zu %zu %u\n", sizeof(mdx_solubility), offsetof(mdx_solubility, score), offsetof(mdx_solubility, aggregation_factor),
         offsetof(mdx_solubility, contact_pair_fraction), MDX_SOLUTE_MAX_COPIES);
  return 0; }
'''
    src = tmp_path / "t.c"
    src.write_text(prog)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    S = _abi.CSolubility
    assert vals == [C.sizeof(S), S.score.offset, S.aggregation_factor.offset, S.contact_pair_fraction.offset, _abi.SOLUTE_MAX_COPIES]
    assert [n for n, _ in S._fields_] == list(ref.FIELDS)


def test_library_exports_the_three_calls():
    lib_path = os.path.join(ROOT, "molchanica_amd", "libmdx.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(lib_path)
    for name in ("mdx_set_solute_copies", "mdx_solubility_mixing", "mdx_snapshot_read_solubility"):
        assert hasattr(lib, name)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/cpp/mixing_driver.cpp: the rule header on one host thread, built with the address and undefined-behaviour sanitizers"""
    exe = tmp_path_factory.mktemp("mixing") / "mixing_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "molchanica_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "mixing_driver.cpp"), "-o", str(exe)])
    return str(exe)


def _run_driver(exe, sol, wat, lo, hi):
    n_copies, n_sel, _ = sol.shape
    text = f"{n_copies} {n_sel} {len(wat)}\n" + " ".join(repr(float(v)) for v in (*lo, *hi)) + "\n"
    text += "\n".join(" ".join(repr(float(v)) for v in p) for p in np.concatenate([sol.reshape(-1, 3), wat])) + "\n"
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
    return dict(zip(ref.FIELDS, (np.float32(v) for v in out[:10]))), np.array(out[10:], np.float64).reshape(-1, 3, 2)


@pytest.mark.parametrize("which", ["mixed", "split"])
def test_rule_header_reproduces_the_pinned_vectors(driver, which):
    sol, wat, lo, hi, _ = mc.pinned(which)
    got, _ = _run_driver(driver, sol, wat, lo, hi)
    for name in ref.FIELDS:
        assert abs(float(got[name]) - PINNED_WANT[which][name]) <= mc.PINNED_EPS, (name, got[name])


@pytest.mark.parametrize("name", ["cubic30_clustered", "rows65_orth15", "faces_unwrapped"])
def test_rule_header_against_the_restatement(driver, name):
    """The host's fp32 pair arithmetic is the device's up to the exp2 of the C library: the same derived bounds hold."""
    case = mc.BY_NAME[name]
    s = case.system()
    sol, wat = case.split(s.pos)
    want, ex = ref.diagnostics(sol, wat, s.box_lo, s.box_hi, full=True)
    got, sums = _run_driver(driver, sol, wat, s.box_lo, s.box_hi)
    bounds = ref.sum_bounds(sol, wat, s.box_lo, s.box_hi)
    assert (np.abs(sums - ex["sums"]) <= bounds).all(), float((np.abs(sums - ex["sums"]) / bounds).max())
    fb = ref.field_bounds(want, ref.local_mixing_bound(ex["sums"], bounds, sol.shape[0], sol.shape[1], len(wat)))
    for f in ref.FIELDS:
        assert abs(float(got[f]) - float(want[f])) <= fb[f], (f, got[f], want[f], fb[f])
