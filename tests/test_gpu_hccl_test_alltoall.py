"""The hccl_test workflow's all_to_all_test (tools/hccl_test, built by __graft_entry__.build()): HcclAlltoAll through a
plain native caller, every element of every size checked by the tool against the host-computed permutation. The
loopback world's threads (schedule below and above the small-call bound's default, and the one-sided kernel forced) and
the IPC communicator with two processes sharing the GPU."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "hccl_test", "bin")


@pytest.mark.parametrize("args", [
    "-b 8K -e 16M -f 8 -d int8 -p 8 -t loopback",
    "-b 1K -e 4M -f 16 -d fp16 -p 3 -t loopback -a 9",
    "-b 1K -e 16M -f 8 -d fp64 -p 2 -t ipc",
])
def test_all_to_all_test(args):
    exe = os.path.join(BIN, "all_to_all_test")
    assert os.path.exists(exe), "tools/hccl_test not built (__graft_entry__.build())"
    env = dict(os.environ, HCCL_AMD_IPC_TIMEOUT_MS="20000")
    p = subprocess.run([exe] + args.split() + ["-n", "5", "-w", "2"], capture_output=True, text=True, timeout=180,
                       env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.strip() and ln.split()[0].isdigit()]
    assert rows, p.stdout
    assert all(r[-1] == "success" for r in rows), p.stdout
