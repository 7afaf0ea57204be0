"""Host code under AddressSanitizer and UndefinedBehaviorSanitizer (the build's race/safety net is the
IR checks plus sanitizers on host code): tests/sanitize/sched_replay_asan.cc builds every schedule family with
hccl_amd/csrc/schedule.cc and replays it with the oracle's C replayer, with buffers malloc'd at exactly their declared
sizes, so an out-of-range IR offset or any undefined behaviour ends the run; tests/sanitize/ipc_plan_sweep.cc sweeps
the one-sided path's planner (hccl_amd/csrc/ipc_plan.cc) and checks the invariants its kernels rely on. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="needs gcc/g++")
def test_schedules_and_replay_are_clean_under_asan_ubsan(tmp_path):
    san = SAN
    oracle_o = tmp_path / "oracle.o"
    subprocess.run(["gcc", "-std=c11", *san, "-c", os.path.join(ROOT, "oracle", "hccl_oracle.c"), "-o", str(oracle_o)],
                   check=True)
    exe = tmp_path / "sched_replay_asan"
    subprocess.run(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "sanitize", "sched_replay_asan.cc"),
                    os.path.join(ROOT, "hccl_amd", "csrc", "schedule.cc"), str(oracle_o), "-o", str(exe)], check=True)
    env = dict(os.environ, **SAN_ENV)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "failures 0" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ipc_planner_sweep_is_clean_under_asan_ubsan(tmp_path):
    """The planner compiles with a plain host compiler (no HIP include path) and holds its invariants over the sweep."""
    csrc = os.path.join(ROOT, "hccl_amd", "csrc")
    exe = tmp_path / "ipc_plan_sweep"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN,
                    os.path.join(ROOT, "tests", "sanitize", "ipc_plan_sweep.cc"), os.path.join(csrc, "ipc_plan.cc"),
                    os.path.join(csrc, "schedule.cc"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "failures 0" in out.stdout
