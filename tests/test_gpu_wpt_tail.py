"""Mixed waves per tile in the pair launch of the one-wave class (MDX_WPT_TAIL): the closing tiles of every XCD
range go out as 2 or 4 one-wave units that share the tile's chunks.  The knob is read once per process, so every arrangement runs in
a child (tests/wpt_tail_child.py), as the MDX_WPT tests do.

Bounds.  Against the oracle: SURVEY 8(c)'s per-atom bound with the allowance tests/test_gpu_timed_body.py uses at water1M (five atoms
in a million between 1 x and 2 x, none beyond) - unchanged.  Between two arrangements at the same positions: the half-list kernel adds
with atomics, so two runs of ONE arrangement already differ; DESIGN.md section 5 records 1.0e-5 kcal/mol/A rms for two runs of
`--dump-outputs` at water1M, and that is the bound here (the arrangement only changes which unit adds which partial sum)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "wpt_tail_child.py")


def run_child(args, **knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_")}
    env.update(knobs)
    p = subprocess.run([sys.executable, CHILD] + [str(a) for a in args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-25:])
    assert p.returncode == 0 and "WPT-TAIL-OK" in p.stdout, tail
    print(tail)


def test_water1m_tail_split_step_loop_forces_against_the_oracle():
    run_child(["big"], MDX_WPT_TAIL="4/8")


@pytest.mark.parametrize("tail,w", [("0", 0), ("4/1", 4), ("2/1", 2), ("4/2", 4), ("2/4", 2)])
@pytest.mark.parametrize("rebuild_inner", [False, True])
def test_edge_shapes_on_a_small_forced_one_wave_class(tail, w, rebuild_inner):
    """T_tail = 0 (the parent arrangement), T_tail = T (units behind the last tile of the last range: the null tile in the tail), short
    lists with fewer plain chunks than units; with the inner list written by the pair kernel's pruning pass and (rebuild_inner) by the
    list rebuild's own one-wave pruning pass."""
    knobs = dict(MDX_WPT="1", MDX_TILE_LPT="2", MDX_WPT8_BELOW="32", MDX_WPT_TAIL=tail)
    if rebuild_inner:
        knobs["MDX_PRUNE_MW_BELOW"] = "0"
    run_child(["small", w], **knobs)


@pytest.mark.parametrize("rebuild_inner", ["1", "0"])
def test_tail_split_and_parent_arrangement_agree_at_the_same_positions(tmp_path, rebuild_inner):
    """786 k atoms frozen.  MDX_REBUILD_INNER=1: the tail units walk the list the rebuild wrote; 0: the force call behind the rebuild is the
    pair kernel's pruning pass - the tail tile's units WRITE the inner list - and the steps behind it walk what they wrote.  Either way
    the forces the step loop left behind are held against the MDX_WPT_TAIL=0 run and against the plain list's evaluation."""
    out = {}
    for tag, tail, w in (("off", "0", 0), ("on", "4/8", 4)):
        path = str(tmp_path / f"f_{tag}.npy")
        run_child(["dump", path, w], MDX_WPT_TAIL=tail, MDX_REBUILD_INNER=rebuild_inner)
        out[tag] = np.load(path)
    rms = lambda d: math.sqrt((d ** 2).sum(1).mean())
    figures = {"step loop, tail on vs off": rms(out["on"][0] - out["off"][0]), "tail on, step loop vs plain list": rms(out["on"][0] - out["on"][1]),
               "tail off, step loop vs plain list": rms(out["off"][0] - out["off"][1])}
    print(", ".join(f"{k}: {v:.2e}" for k, v in figures.items()))
    assert all(v <= 1.0e-5 for v in figures.values()), figures
