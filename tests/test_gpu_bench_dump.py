"""`bench.py --dump-outputs DIR`: the arrays two builds are compared by.  Files, shapes and dtype; two runs with the same
arguments agree to rounding (the dumped steps start from the same bits: a preparation on the deterministic pair kernel);
with the deterministic pair kernel in the timed path too the dumps are the same bits; the decomposed handle writes the
same arrays through its collective download."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("positions", "velocities", "forces")
ARGS = ["--gpus", "1", "--workload", "dna100k", "--steps", "20", "--warmup", "5"]


def _line(out):
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d, n_atoms):
    arrs = {}
    for n in NAMES:
        a = np.load(os.path.join(d, n + ".npy"))
        assert a.dtype == np.float32 and a.shape == (n_atoms, 3), (n, a.dtype, a.shape)
        assert np.isfinite(a).all(), n
        arrs[n] = a.astype(np.float64)
    return arrs


def _bench(d, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(d), *extra],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    j = _line(out)
    return j, _load(d, j["config"]["n_atoms"])


def _diff(a, b, box):
    """-> {name: (rms of the difference, 99.9th percentile of |difference|, each / rms of the array; max |difference|)};
    positions by minimum image.  The percentile lets through what a pair within rounding of rc does when it flips: it moves
    its two atoms by the whole pair force - a handful of components, never the bulk."""
    res = {}
    for n in NAMES:
        d = a[n] - b[n]
        if n == "positions":
            d -= np.round(d / box) * box
        scale = float(np.sqrt((b[n] ** 2).mean()))
        d = np.abs(d)
        res[n] = (float(np.sqrt((d ** 2).mean())) / scale, float(np.percentile(d, 99.9)) / scale, float(d.max()))
    return res


@pytest.fixture(scope="module")
def box():
    from molchanica_amd import systems
    s = systems.BY_NAME["dna100k"]()
    return np.asarray(s.box_hi, np.float64) - np.asarray(s.box_lo, np.float64)


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("dump_a"))


def test_two_runs_agree_to_rounding(first, box, tmp_path):
    j, a = first
    assert j["steps"] == 20 and j["ms_per_step"] > 0
    _, b = _bench(tmp_path)
    d = _diff(a, b, box)
    print("run to run (rms / rms of the array, max):", d)
    # the pair kernel's j-forces are f32 atomics: the last bits of a force differ with their order, nothing more (water1M:
    # forces 1.2e-6 of the rms apart at the 99.99th percentile; 16 dumped steps instead of 2 leave them 5e-4 apart there)
    for n in NAMES:
        assert d[n][1] <= 3e-6 and d[n][0] <= 1e-3, d
    assert d["positions"][2] <= 1e-2, d


def test_deterministic_pair_kernel_dumps_the_same_bits(tmp_path):
    """nb_variant 2 in the timed path too: every step of the run is reproducible, so the dumps of two runs are equal - which
    holds only if the preparation (minimiser, thermostat, both on nb_variant 2) is the same bits in every run."""
    _, a = _bench(tmp_path / "a", "--nb-variant", "2")
    _, b = _bench(tmp_path / "b", "--nb-variant", "2")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n


def test_decomposed_handle_dumps_the_same_arrays(first, box, tmp_path):
    """The launcher's line with one rank on the decomposed path: the dumped steps run below the ABI's decomposition and the
    arrays come back through its collective download, in caller order."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), *ARGS, "--decomposed", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), capture_output=True, text=True, timeout=600)
    j = _line(out)
    assert "1x1x1" in j["config"]["parallelism"]
    d = _diff(_load(tmp_path, j["config"]["n_atoms"]), first[1], box)
    print("decomposed vs single handle (rms / rms of the array, max):", d)
    # not the same arithmetic as one handle (brick-local coordinates, its own lists and launch arrangement): the decomposed path
    # follows the single handle within the decomposition tests' bounds, not to the last bits - measured on dna100k, the same in
    # every run: rms 5e-8 (positions), 1.3e-4 (velocities), 9.4e-4 (forces) of the array's rms.  Arrays out of caller order or
    # from another state would be O(1) apart.
    assert d["positions"][0] <= 1e-6 and d["positions"][2] <= 1e-2, d
    assert d["velocities"][0] <= 1e-3 and d["forces"][0] <= 5e-3, d
