"""rk_accepted_h_abs (csrc/mpcx_device.hpp) -- the step-size controller that evaluates its pow only where the value decides the
next step -- against the plain formula, on the host: tests/tools/rk_step_factor_check.cpp is compiled as host code with the
address and undefined-behaviour sanitizers and compares, bit for bit, the next step's size after the integrators' clamp over
error norms on a log grid from 1e-300 to 1 plus 0 and the +-8 ulp neighbours of every threshold, h_try / max_step in {1, 1 - 2^-52,
0.9, 0.5, 1e-3} plus the ratios that put the max_step case on its boundary, after a rejection and not, for both error exponents."""
import os
import re
import subprocess

from mpconstellation_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_factor_helper_matches_the_formula(tmp_path):
    exe = str(tmp_path / "rk_step_factor_check")
    subprocess.check_call([build.HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "tools", "rk_step_factor_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    m = re.search(r"cases: at_bound (\d+), small (\d+), above_max_step (\d+), pow (\d+); mismatches (\d+)", r.stdout)
    assert m and all(int(v) > 0 for v in m.groups()[:4]) and int(m.group(5)) == 0
