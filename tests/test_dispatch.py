"""The step from a run-time padded dimension / kernel kind to a kernel instantiation exists once (with_dp / with_kind of
trieste_amd/csrc/tgp_internal.hpp) and every templated launch goes through it.  CPU test: tools/check_dispatch.hip is a
host-only program that launches nothing -- the callable records the DP it is handed.

Why it is a test: the kernels index their rows as ``Xs[k * DP + c]``; a dispatch that hands a dp to the wrong instantiation
reads with the wrong stride and returns numbers, not an error, and the GPU suites cover dp = 16 and 32 thinly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_every_padded_dimension_and_kind_reaches_its_own_instantiation(tmp_path):
    exe = os.path.join(tmp_path, "check_dispatch")
    subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-Wall", "-I", os.path.join(ROOT, "trieste_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_dispatch.hip"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "check_dispatch: ok" in run.stdout
