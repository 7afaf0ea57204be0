"""The point-to-point planner and HcclBatchSendRecv's list handling under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/sanitize/p2p_plan_sweep.cc, a stand-alone program, sweeps P2pPlanFor and
BatchSendRecvOrder (hccl_amd/csrc/ipc_plan.cc) and checks the invariants the kernel and the entry point rely on. It is
compiled with the host compiler and run directly, as tests/test_sanitize_scatter_gatherv.py builds its sweep. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_p2p_plan_sweep_is_clean_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "hccl_amd", "csrc")
    exe = tmp_path / "p2p_plan_sweep"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN,
                    os.path.join(ROOT, "tests", "sanitize", "p2p_plan_sweep.cc"),
                    os.path.join(csrc, "ipc_plan.cc"), os.path.join(csrc, "schedule.cc"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "failures 0" in out.stdout
