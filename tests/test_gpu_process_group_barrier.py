"""dist.barrier() over the "hccl" backend: HcclBarrier, with no tensor allocated and nothing reduced.

Worlds of 1 process (the RCCL-backed communicator, which returns at once) and of 2 processes sharing the GPU (the
backend's IPC transport, as tests/test_gpu_process_group.py). Before the operator existed the backend allocated a
one-element tensor per barrier and ran a SUM AllReduce on it; here Comm.barrier is called once per dist.barrier(),
Comm.all_reduce not at all, and torch's allocator holds the same bytes before and after.
"""
import datetime
import multiprocessing as mp
import os
import socket
import time
import traceback

import pytest

pytestmark = pytest.mark.gpu

BARRIERS = 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, n, port, transport, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"
    if transport:
        os.environ["HCCL_AMD_PG_TRANSPORT"] = transport
    try:
        import torch
        import torch.distributed as dist
        import hccl_amd as H
        import hccl_amd.process_group  # noqa: F401  (registers backend "hccl")

        calls = {"barrier": 0, "all_reduce": 0}

        def counted(name):
            inner = getattr(H.Comm, name)

            def wrapper(self, *a, **kw):
                calls[name] += 1
                return inner(self, *a, **kw)

            setattr(H.Comm, name, wrapper)

        counted("barrier")
        counted("all_reduce")
        torch.cuda.set_device(0)
        dist.init_process_group(backend="hccl", rank=rank, world_size=n, init_method=f"tcp://127.0.0.1:{port}",
                                timeout=datetime.timedelta(seconds=120))
        checks, stamps = {}, None
        keep = torch.ones(16, device="cuda")  # the allocator is initialised before the first measurement
        torch.cuda.synchronize()
        held, peak = [], []
        for _ in range(BARRIERS):
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            dist.barrier()
            held.append(torch.cuda.memory_allocated() - before)
            peak.append(torch.cuda.max_memory_allocated() - before)
        checks["returned"] = True
        checks["no_allocation"] = held == [0] * BARRIERS and peak == [0] * BARRIERS
        checks["barrier_calls"] = calls["barrier"] == BARRIERS
        checks["no_all_reduce"] = calls["all_reduce"] == 0
        work = dist.barrier(async_op=True)
        work.wait()
        checks["async_work"] = work.is_completed() and work.is_success() and calls["barrier"] == BARRIERS + 1
        # a late rank holds the others: the host returns from dist.barrier only when every rank has arrived
        if n > 1:
            dist.barrier()
            if rank == n - 1:
                time.sleep(0.3)
            entered = time.monotonic()
            dist.barrier()
            left = time.monotonic()
            stamps = (entered, left)  # compared by the parent: the monotonic clock is one for the host's processes
        del keep
        dist.destroy_process_group()
        q.put((rank, "ok", (checks, stamps)))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)


@pytest.mark.parametrize("n,transport", [(1, ""), (2, "ipc")])
def test_dist_barrier_calls_hccl_barrier_and_allocates_nothing(n, transport):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, n, port, transport, q)) for r in range(n)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in procs:
            rank, msg, res = q.get(timeout=240)
            got[rank] = (msg, res)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(n):
        msg, res = got[r]
        assert msg == "ok", f"rank {r}: {msg}"
        assert all(res[0].values()), f"rank {r}: {res[0]}"
    if n > 1:
        late_entered = got[n - 1][1][1][0]
        for r in range(n):
            assert got[r][1][1][1] >= late_entered, (r, got[r][1][1], late_entered)
