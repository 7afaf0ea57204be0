"""HcclBarrier in RANK mode: 2 and 4 processes sharing the GPU, each one rank with its own launch of k_ipc_barrier, the
peers' flag words opened from IPC handles (the harness of tests/test_gpu_ipc_ranks.py).

One rank sleeps 0.3 s on the host before it calls HcclBarrier. No rank's stream may pass its barrier before that rank
has called its own, so every rank's completion time is at or after the late rank's enqueue time (time.monotonic() is
one clock for every process of a host). A barrier that did nothing would complete 0.3 s earlier on the other ranks.

The same worker serves tests/test_gpu_barrier.py's graph replay (mode "graph"), which is in rank mode because a
loopback world cannot be captured.
"""
import datetime
import multiprocessing as mp
import os
import socket
import time
import traceback

import pytest

pytestmark = pytest.mark.gpu

HOST_DELAY_S = 0.3
REPLAYS = 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def sleep_cycles(torch, target_ms=30.0):
    """The argument of torch.cuda._sleep for a device delay of about target_ms. _sleep spins until a device counter has
    advanced by its argument, and how fast that counter runs is a property of the device (the shader clock on some, a
    constant 100 MHz clock on others), so its rate is measured here: a probe sleep sized for 1 ms at the reported shader
    clock (at most 1 ms, since no counter runs faster) is timed with events, and the count is scaled from that."""
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    khz = int(getattr(props, "clock_rate", 0)) or 100000  # cycles per ms at the shader clock
    probe = khz
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(probe)  # the first launch pays the kernel's load
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(probe)
    e1.record()
    torch.cuda.synchronize()
    per_ms = probe / max(e0.elapsed_time(e1), 1e-3)
    return int(per_ms * target_ms)


def _rank_main(rank, n, port, q, mode):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"  # a lost peer shows as a status bit, never a hang
    try:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)
        import hccl_amd as H

        def all_gather(b):
            out = [None] * n
            dist.all_gather_object(out, b)
            return out

        comm = H.comm_init_host_exchange(n, rank, all_gather)
        stream = torch.cuda.Stream()
        before = comm.device_bytes()
        comm.barrier(stream)  # the collective set-up of the one-sided path: flags and status words only
        stream.synchronize()
        res = {"first_algo": comm.last_algo, "bytes_before": before, "bytes_after": comm.device_bytes()}
        if mode == "host_delay":
            late = n - 1
            dist.barrier()  # every rank starts the timed call together
            if rank == late:
                time.sleep(HOST_DELAY_S)
            res["enqueued"] = time.monotonic()
            comm.barrier(stream)
            stream.synchronize()
            res["completed"] = time.monotonic()
            res["algo"] = comm.last_algo
        else:
            res["replays"] = _graph_replays(torch, dist, H, comm, stream, rank, n)
        res["status"] = comm.ipc_status()
        dist.barrier()
        comm.destroy()  # collective: no rank unmaps while a peer's kernel may still store into it
        dist.destroy_process_group()
        q.put((rank, "ok", res))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)  # peers' kernels are bounded: let them drain before this process's memory goes away


def _graph_replays(torch, dist, H, comm, stream, rank, n):
    """HcclBarrier and the marker copy captured once, replayed REPLAYS times with the rotating device delay outside the
    graph. The marker array is rank 0's, mapped by every process (torch's IPC handle of the tensor)."""
    from torch.multiprocessing.reductions import reduce_tensor

    marks = torch.full((n,), -1, dtype=torch.int64, device="cuda") if rank == 0 else None
    box = [reduce_tensor(marks)[1] if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    if rank != 0:
        from torch.multiprocessing.reductions import rebuild_cuda_tensor
        marks = rebuild_cuda_tensor(*box[0])
    seen = torch.full((n,), -2, dtype=torch.int64, device="cuda")
    cycles = sleep_cycles(torch)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    dist.barrier()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        comm.barrier(torch.cuda.current_stream())
        seen.copy_(marks)
    captured_algo = comm.last_algo
    out = []
    for i in range(REPLAYS):
        delayed = i % n
        pre, post = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d0, d1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dist.barrier()  # every rank's copy of the previous replay has ended before a marker changes
        t0 = time.monotonic()
        with torch.cuda.stream(stream):
            if rank == delayed:
                d0.record()
                torch.cuda._sleep(cycles)
                d1.record()
            pre.record()
            marks[rank:rank + 1].fill_(i)
            graph.replay()
            post.record()
        stream.synchronize()
        done = time.monotonic()
        out.append({"seen": seen.tolist(), "own_order_ms": pre.elapsed_time(post), "start": t0, "done": done,
                    "delay_s": d0.elapsed_time(d1) / 1e3 if rank == delayed else None, "algo": captured_algo})
    if rank != 0:
        del marks  # the mapping goes before its owner's tensor does
    torch.cuda.synchronize()
    dist.barrier()
    return out


def spawn(n, mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, n, port, q, mode)) for r in range(n)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in procs:
            rank, msg, res = q.get(timeout=300)
            got[rank] = (msg, res)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(n):
        assert got[r][0] == "ok", f"rank {r}:\n{got[r][0]}"
    return [got[r][1] for r in range(n)]


@pytest.mark.parametrize("n", [2, 4])
def test_no_rank_passes_before_the_late_rank_has_called(n):
    import hccl_amd as H

    res = spawn(n, "host_delay")
    late = n - 1
    for r in range(n):
        print(f"rank {r}: enqueued {res[r]['enqueued'] - res[late]['enqueued']:+.4f} s, completed "
              f"{res[r]['completed'] - res[late]['enqueued']:+.4f} s relative to the late rank's enqueue")
    for r in range(n):
        assert res[r]["completed"] >= res[late]["enqueued"], (r, res[r], res[late])
        assert res[r]["algo"] == res[r]["first_algo"] == int(H.Algo.IPC)
        assert res[r]["status"] & 1 == 0
        # the first barrier set up what every one-sided call needs, alike on every rank (tests/test_gpu_barrier.py
        # compares the amount with a staging tier's)
        assert res[r]["bytes_before"] == 0 < res[r]["bytes_after"] == res[0]["bytes_after"]
    # the stagger was real: the other ranks had enqueued well before the late one
    assert all(res[late]["enqueued"] - res[r]["enqueued"] > HOST_DELAY_S / 2 for r in range(n - 1))
