"""CPU: the Winograd F(2x4,3x3) arithmetic of csrc/wino_f24.h, through a stand-alone host
program (tests/wino_f24_host.cpp) that includes the header the HIP kernels include: filter
transform in double rounded once, data / output transforms in fp32, the cin contraction as an
fp32 fmaf chain per transform-domain point, against its own double-precision direct conv."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "wino_f24_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)),
               None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("wino_f24") / "wino_f24_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(PKG, "csrc"), SRC,
                           "-o", exe])
    return exe


def _run(prog, *args):
    out = subprocess.run([prog, *args], capture_output=True, text=True, check=True).stdout
    return {k: float(v) for k, v in re.findall(r"(\w+) ([-+.\deE]+|nan|inf)", out)}


def test_f24_algebra_is_exact_on_small_integers(prog):
    """Inputs in [-4, 4], weights 15 x integers (U integral or half-integral): every product and
    sum is exact in fp32, so any wrong constant, sign or index of B^T / G / A^T shows as a
    non-zero difference."""
    r = _run(prog, "exact")
    assert r["max_ref"] > 100.0
    assert r["max_abs_diff"] == 0.0


def test_f24_fp32_error_at_128_channels(prog):
    """128 -> 128 on a 16 x 32 image, silu(randn) inputs, randn / (3 sqrt(cin)) weights: max
    error <= 5e-6 of max|ref| (4 x the 1.2-1.3e-6 of the arithmetic's design estimate, half the
    1e-5 gate of the Winograd op tests).  Measured with this program: 1.16e-6."""
    r = _run(prog, "error", "128", "128", "16", "32")
    print(f"F(2x4,3x3) 128->128 16x32: max err / max|ref| = {r['rel']:.3e}")
    assert r["max_ref"] > 0.5
    assert r["rel"] <= 5e-6
