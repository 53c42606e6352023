"""mdx_triad_build (molchanica_amd/csrc/mdx_hostutil.cpp), the host decision behind the triad flavour of the fused bonded + kick + drift
pass: a stand-alone program (tests/triad_detect_main.cpp, its own main) is built with the function's translation unit - with
AddressSanitizer and UBSan where the host compiler links them - and run.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "triad_detect_main.cpp"), os.path.join(ROOT, "molchanica_amd", "csrc", "mdx_hostutil.cpp")]


def test_triad_cases_in_a_sanitized_standalone_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "triad_detect")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall"] + SRC + ["-o", exe]
    # (the runtimes linked into the program itself: it runs as it is wherever the suite runs, whatever else the process environment loads)
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:      # a compiler without the static sanitizer runtimes: the cases still run
        print("no sanitizer runtimes:", san.stderr.splitlines()[-1:] if san.stderr else "")
        subprocess.check_call(base)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "TRIAD-DETECT-OK" in p.stdout, p.stdout + p.stderr
