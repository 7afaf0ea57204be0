"""HcclScatter's and HcclAllGatherV's host code under AddressSanitizer and UndefinedBehaviorSanitizer: tests/sanitize/
scatter_gatherv_sweep.cc, a stand-alone program, sweeps the planner's functions for the two new kinds
(hccl_amd/csrc/ipc_plan.cc) and the two schedule generators (hccl_amd/csrc/schedule.cc) and checks the invariants the
kernel and the executor rely on. It is compiled with the host compiler and run directly, as
tests/test_sanitize_alltoall.py builds alltoall_sweep.cc. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_scatter_gatherv_sweep_is_clean_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "hccl_amd", "csrc")
    exe = tmp_path / "scatter_gatherv_sweep"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN,
                    os.path.join(ROOT, "tests", "sanitize", "scatter_gatherv_sweep.cc"),
                    os.path.join(csrc, "ipc_plan.cc"), os.path.join(csrc, "schedule.cc"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "failures 0" in out.stdout
