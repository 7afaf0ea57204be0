"""The cross-rank argument check in RANK mode: 2 and 4 processes sharing the GPU, each one rank with its own launch of
k_ipc_check, the peers' check areas opened from IPC handles (the harness of tests/test_gpu_ipc_ranks.py: gloo
bootstrap, one log per rank, every child under its own time limit, no process started after one has failed). The logs
go to the directory HCCL_AMD_TEST_LOG_DIR names, or to the system's temporary directory.

The communicators are IPC-only (the host-exchange transport has no send/recv), so every call runs one-sided and a
failed check leaves nothing waiting. Modes of the worker:
  * "consistent": AllGather and AllReduce (every mode begins with them), Broadcast, AllGather, Barrier, ReduceScatter
    with the switch on: results and six checks;
  * "count" / "operator": rank n - 1 passes 4100 elements against 4099, or calls AllGather against AllReduce;
  * "graph": a checked AllReduce captured once and replayed three times: the sequence number lives on the device.
"""
import datetime
import multiprocessing as mp
import os
import socket
import tempfile
import time
import traceback

import pytest

pytestmark = pytest.mark.gpu

LOGS = os.environ.get("HCCL_AMD_TEST_LOG_DIR") or tempfile.gettempdir()
REPLAYS = 3
CHILD_LIMIT_S = 120
_failed = []  # a spawn that failed: no later test of this module starts processes


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, n, port, q, mode):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"  # a lost peer shows as a status bit, never a hang
    os.environ["HCCL_DFS_CONFIG"] = "inconsistent_check:on"
    os.makedirs(LOGS, exist_ok=True)
    log = open(os.path.join(LOGS, f"check_ranks_{mode}_n{n}_r{rank}.log"), "w")
    try:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n,
                                timeout=datetime.timedelta(seconds=CHILD_LIMIT_S))
        torch.cuda.set_device(0)
        import hccl_amd as H

        def all_gather(b):
            out = [None] * n
            dist.all_gather_object(out, b)
            return out

        comm = H.comm_init_host_exchange(n, rank, all_gather)
        assert comm.get_config(H.Config.INCONSISTENT_CHECK) == 1  # read from the environment
        stream = torch.cuda.Stream()
        SUM = int(H.HcclReduceOp.SUM)
        x = torch.full((4100,), float(rank + 1), device="cuda")
        y = torch.zeros(n * 4100, device="cuda")
        want = float(n * (n + 1) // 2)
        res = {}
        # The collective set-ups, and two checks that pass. The staging tier too, which the AllGather of the "operator"
        # mode needs and the AllReduce it meets (LL form) does not: a set-up is a host exchange of all ranks, which
        # ranks that disagree about the operator would not enter together.
        comm.all_gather(x[:4099], y[:n * 4099], stream)
        comm.all_reduce(x[:4099], y[:4099], SUM, stream)
        stream.synchronize()
        res["first"] = (comm.async_error(), comm.check_launches(), bool((y[:4099] == want).all()))
        if mode == "consistent":
            b = torch.full((33,), rank, dtype=torch.uint8, device="cuda")
            z = torch.zeros(16, device="cuda")
            comm.broadcast(b, n - 1, stream)
            comm.all_gather(x[:7], y[:7 * n], stream)
            comm.barrier(stream)
            comm.reduce_scatter(x[:16 * n], z, SUM, stream)
            stream.synchronize()
            res["ok"] = bool((b == n - 1).all()) and bool((z == want).all()) and \
                y[:7 * n].tolist() == [float(q + 1) for q in range(n) for _ in range(7)]
        elif mode in ("count", "operator"):
            odd = rank == n - 1
            dist.barrier()
            t0 = time.monotonic()
            if mode == "count":
                k = 4100 if odd else 4099
                comm.all_reduce(x[:k], y[:k], SUM, stream)
            elif odd:
                comm.all_gather(x[:4099], y[:n * 4099], stream)
            else:
                comm.all_reduce(x[:4099], y[:4099], SUM, stream)
            stream.synchronize()
            res["error"] = comm.async_error()
            res["report"] = comm.inconsistency()
            res["wall"] = time.monotonic() - t0
            res["later"] = []
            for _ in range(2):
                try:
                    comm.all_reduce(x[:4099], y[:4099], SUM, stream)
                    res["later"].append(0)
                except H.HcclError as e:
                    res["later"].append(e.code)
        else:
            out = torch.zeros(4099, device="cuda")
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            dist.barrier()
            before = comm.check_launches()
            with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
                comm.all_reduce(x[:4099], out, SUM, torch.cuda.current_stream())
            res["replays"] = []
            for i in range(REPLAYS):
                x.fill_(float(rank + 1 + i))
                out.zero_()
                torch.cuda.synchronize()
                dist.barrier()
                with torch.cuda.stream(stream):
                    graph.replay()
                stream.synchronize()
                res["replays"].append(bool((out == want + n * i).all()))
            res["replay_checks"] = comm.check_launches() - before
        res["status"] = comm.ipc_status()
        res["launches"] = comm.check_launches()
        res["error_end"] = comm.async_error()
        print(res, file=log, flush=True)
        dist.barrier()
        comm.destroy()  # collective: no rank unmaps while a peer's kernel may still store into it
        dist.destroy_process_group()
        q.put((rank, "ok", res))
    except Exception:  # noqa: BLE001
        print(traceback.format_exc(), file=log, flush=True)
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)  # peers' kernels are bounded: let them drain before this process's memory goes away


def spawn(n, mode):
    if _failed:
        pytest.fail(f"not started: {_failed[0]} failed before")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, n, port, q, mode)) for r in range(n)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in procs:
            rank, msg, res = q.get(timeout=CHILD_LIMIT_S)
            got[rank] = (msg, res)
    except Exception:  # noqa: BLE001  (a child past its limit)
        _failed.append((n, mode))
        raise
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(n):
        if got[r][0] != "ok":
            _failed.append((n, mode))
        assert got[r][0] == "ok", f"rank {r}:\n{got[r][0]}"
    return [got[r][1] for r in range(n)]


@pytest.mark.parametrize("n", [2, 4])
def test_consistent_sequence(n):
    res = spawn(n, "consistent")
    for r in range(n):
        assert res[r]["first"] == (0, 2, True), (r, res[r])
        assert res[r]["ok"] and res[r]["launches"] == 6 and res[r]["status"] & 3 == 0 and res[r]["error_end"] == 0


@pytest.mark.parametrize("mode", ["count", "operator"])
@pytest.mark.parametrize("n", [2, 4])
def test_one_rank_differs(n, mode):
    import hccl_amd as H

    res = spawn(n, mode)
    usual, other = (4099, 4100) if mode == "count" else (int(H.OpType.ALLREDUCE), int(H.OpType.ALLGATHER))
    name = "DataCount" if mode == "count" else "OpType"
    for r in range(n):
        print(f"n={n} {mode} rank {r}: {res[r]['wall']:.3f} s, {res[r]['report']}")
        assert res[r]["first"] == (0, 2, True)
        assert res[r]["error"] == H.HcclResult.HCCL_E_PARA, (r, res[r])
        rep = res[r]["report"]
        want = (0, name, other, usual) if r == n - 1 else (n - 1, name, usual, other)
        assert rep is not None and (rep["peer"], rep["name"], rep["local"], rep["remote"]) == want, (r, rep)
        assert res[r]["wall"] < 5.0
        assert res[r]["status"] & 3 == 3
        assert res[r]["later"] == [H.HcclResult.HCCL_E_PARA, H.HcclResult.HCCL_E_SUSPENDING]


def test_captured_check_replays():
    n = 2
    res = spawn(n, "graph")
    for r in range(n):
        assert res[r]["replays"] == [True] * REPLAYS, (r, res[r])
        assert res[r]["replay_checks"] == REPLAYS  # the capture launched none, each replay one
        assert res[r]["status"] & 3 == 0 and res[r]["error_end"] == 0
