"""Child of tests/test_gpu_wpt_tail.py: one process per MDX_WPT_TAIL value (the library reads its knobs once per process).

usage: python tests/wpt_tail_child.py big | small <expect_w> | dump <out.npy> <expect_w>
  big    water1M with the closing tiles of every XCD range split (MDX_WPT_TAIL in the environment): 32 steps across a list rebuild and
         several pruning passes, then the forces the step loop left behind against one oracle evaluation at the downloaded positions -
         the bound and the allowance tests/test_gpu_timed_body.py uses at that size;
  small  12 k atoms forced into the one-wave class and the order by length (MDX_WPT=1, MDX_TILE_LPT=2): the edge shapes;
  dump   the 786 k-atom water box, atoms frozen (dt = 1e-9 ps: fp32 positions do not move): the forces the step loop left behind and the
         plain-list evaluation of the same positions, saved for the parent to compare between arrangements."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from molchanica_amd import MdConfig, systems  # noqa: E402
from molchanica_amd import md_state  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests.test_gpu_timed_body import step_loop_forces_vs_oracle  # noqa: E402


def check_tail(md, expect_w):
    info = md.pair_launch_info()
    step, tail = info["step"], info["tail"]
    assert (step["waves_per_tile"], step["dual"], step["half"], step["energy"]) == (1, 3, 1, 0), info
    assert tail["waves_per_tile"] == expect_w, info
    assert (tail["tiles"] > 0) == (expect_w > 0), info
    return step, tail


def big():
    w = int(os.environ["MDX_WPT_TAIL"].split("/")[0])
    s, cfg = systems.water1m(), MdConfig()
    with md_state.MdState(s, cfg) as md:
        md.step(0.0005, None, 20)
        step, tail = check_tail(md, w)
        assert step["tiles"] >= 12000 and 0 < tail["tiles"] < step["tiles"], (step, tail)
        md.step(0.0005, None, 12)
        st = md.stats()
        assert st["rebuild_count"] >= 2 and st["prune_passes"] >= 3 and st["rebuild_fallbacks"] == 0, (st["rebuild_count"], st["prune_passes"])
        check_tail(md, w)
        print(f"water1M: tail {tail}, rebuilds {st['rebuild_count']}, pruning passes {st['prune_passes']}")
        step_loop_forces_vs_oracle(md, orc, s, cfg, "water1M, tail split, after 32 steps", slack_rel=4e-5, outliers=5)


def small(expect_w):
    assert os.environ.get("MDX_WPT") == "1" and os.environ.get("MDX_TILE_LPT") == "2"
    cases = [
        ("water12k", systems.water_box(16, seed=41), MdConfig()),
        # rc 3 + skin 1 (the dual list wants its inner skin of 0.5 below the skin): a tile's half list is two or three chunks, the masked
        # run among them - fewer plain chunks than units
        ("water12k-short-cutoff", systems.water_box(16, seed=41), MdConfig(lj_cutoff=3.0, coulomb_cutoff=3.0, skin=1.0)),
    ]
    for name, s, cfg in cases:
        with md_state.MdState(s, cfg) as md:
            done = 0
            for burst in (7, 20, 33):
                md.step(0.0005, None, burst)
                done += burst
                step, tail = check_tail(md, expect_w)
                if os.environ.get("MDX_WPT_TAIL", "").endswith("/1"):      # every tile, and the units behind the last tile of the last range
                    assert tail["tiles"] == step["tiles"] and step["tiles"] % 8 != 0, (step, tail)
                step_loop_forces_vs_oracle(md, orc, s, cfg, f"{name} tail {os.environ.get('MDX_WPT_TAIL')} after {done} steps")
            st = md.stats()
            assert st["prune_passes"] >= 3 and st["rebuild_count"] >= 2, (st["prune_passes"], st["rebuild_count"])
            print(f"{name}: tail {tail} of {step['tiles']} tiles, cluster pairs per tile {st['n_cluster_pairs'] / step['tiles']:.0f}, "
                  f"pruning passes {st['prune_passes']}, rebuilds {st['rebuild_count']}")


def dump(path, expect_w):
    s, cfg = systems.water_box(64, seed=5), MdConfig()
    with md_state.MdState(s, cfg) as md:
        md.step(1e-9, None, 6)
        step, _ = check_tail(md, expect_w)
        assert step["tiles"] >= 12000, step
        f_step = md.forces().astype(np.float64)          # what the last step's pair launch produced, NOT re-evaluated
        md.energy()                                      # plain list, energy flavour, same positions
        f_plain = md.forces().astype(np.float64)
        st = md.stats()
        np.save(path, np.stack([f_step, f_plain]))
        print(f"water64: pruning passes {st['prune_passes']}, inner lists from rebuilds {md.pair_launch_info()['inner_lists_from_rebuilds']}")


if __name__ == "__main__":
    assert md_state.device_count() >= 1
    orc.lib()
    mode = sys.argv[1]
    if mode == "big":
        big()
    elif mode == "small":
        small(int(sys.argv[2]))
    else:
        dump(sys.argv[2], int(sys.argv[3]))
    print("WPT-TAIL-OK")
