"""The hccl_test workflow's scatter_test and all_gather_v_test (tools/hccl_test, built by __graft_entry__.build()):
HcclScatter and HcclAllGatherV through a plain native caller, every element of every size checked by the tool against
the host-computed result. The loopback world's threads (the schedule, and the one-sided kernel forced) and the IPC
communicator with two processes sharing the GPU. all_gather_test, whose name all_gather_v_test extends, still runs
HcclAllGather."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "hccl_test", "bin")


def run_tool(name, args, extra_env=None):
    exe = os.path.join(BIN, name)
    assert os.path.exists(exe), "tools/hccl_test not built (__graft_entry__.build())"
    env = dict(os.environ, HCCL_AMD_IPC_TIMEOUT_MS="20000", **(extra_env or {}))
    p = subprocess.run([exe] + args.split() + ["-n", "5", "-w", "2"], capture_output=True, text=True, timeout=180,
                       env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.strip() and ln.split()[0].isdigit()]
    assert rows, p.stdout
    assert all(r[-1] == "success" for r in rows), p.stdout
    return p


@pytest.mark.parametrize("name", ["scatter_test", "all_gather_v_test"])
@pytest.mark.parametrize("args", [
    "-b 8 -e 1M -f 4 -d int8 -p 8 -t loopback",
    "-b 8 -e 1M -f 4 -d fp16 -p 3 -t loopback -a 9",
    "-b 8 -e 1M -f 4 -d fp64 -p 2 -t ipc",
])
def test_new_binaries_verify(name, args):
    run_tool(name, args)


def test_all_gather_test_still_runs_all_gather():
    """The tool's header names the operator it runs: the binary whose name is a prefix of all_gather_v_test still
    selects AllGather, and --op overrides the name either way."""
    def op_of(p):
        return p.stdout.splitlines()[0].rsplit("op is ", 1)[1].strip()

    args = "-b 1K -e 64K -f 8 -d fp32 -p 2 -t loopback -a 1"
    assert op_of(run_tool("all_gather_test", args)) == "all_gather"
    assert op_of(run_tool("all_gather_v_test", args)) == "all_gather_v"
    assert op_of(run_tool("scatter_test", args)) == "scatter"
    assert op_of(run_tool("all_gather_test", args + " --op all_gather_v")) == "all_gather_v"
