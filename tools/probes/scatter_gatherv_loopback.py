#!/usr/bin/env python3
"""Scatter and AllGatherV on one GPU: their one-sided kernel against their mesh schedule and against the same traffic
expressed as HcclAlltoAllV.

Two stand-ins for a node, both on one GPU (no figure here crosses xGMI): an 8-rank loopback world (one process, one
launch for all ranks) and a 2-process rank-mode pair (peers' staging opened from IPC handles; it has no send/recv
transport, so only the one-sided kernels run there). Blocks of 1 KiB, 1 MiB and 64 MiB; per size, operator and variant,
`--runs` runs of up to `--calls` calls after a warm-up run (fewer calls at the large sizes), the variants taken in turn
inside every run so that drift hits them alike. Operators (root 1 for the Scatter):
  scatter   every rank receives one block of `bytes` from the root
  gatherv   every rank contributes `bytes`, except rank 0, which contributes a sixteenth of it
Variants:
  one_sided  HcclScatter / HcclAllGatherV under HCCL_AMD_ALGO_IPC (k_ipc_sg)
  schedule   the same calls on the mesh schedule, one transport group (loopback world only)
  a2av       the same bytes through the public HcclAlltoAllV under HCCL_AMD_ALGO_IPC (k_ipc_a2a): for the Scatter only
             the root's row is non-zero; for the AllGatherV every peer is sent the same block (equal sdispls)
A row per (mode, op, bytes, variant): the runs' per-call times in microseconds, their median, minimum and maximum.

    python tools/probes/scatter_gatherv_loopback.py --out profiles/scatter_gatherv_loopback_one_gpu.jsonl
"""
import argparse
import datetime
import json
import multiprocessing as mp
import os
import socket
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = [1 << 10, 1 << 20, 64 << 20]
OPS = ("scatter", "gatherv")
SROOT = 1


def gather_counts(n, nbytes):
    return [max(1, nbytes // 16) if q == 0 else nbytes for q in range(n)]


def buffers(torch, op, n, r, nbytes):
    """(send, recv) of rank r, bytes."""
    if op == "scatter":
        send = torch.full((n * nbytes,), r, dtype=torch.uint8, device="cuda") if r == SROOT else None
        return send, torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = gather_counts(n, nbytes)
    return (torch.full((counts[r],), r, dtype=torch.uint8, device="cuda"),
            torch.empty(sum(counts), dtype=torch.uint8, device="cuda"))


def issue(H, comm, op, variant, n, r, nbytes, send, recv, stream):
    if op == "scatter":
        if variant != "a2av":
            comm.scatter(send, recv, SROOT, stream)
            return
        sc = [nbytes] * n if r == SROOT else [0] * n
        rc = [nbytes if q == SROOT else 0 for q in range(n)]
        comm.alltoall_v(send, sc, [q * nbytes if r == SROOT else 0 for q in range(n)], recv, rc, [0] * n, stream,
                        dtype=H.HcclDataType.UINT8)
        return
    counts = gather_counts(n, nbytes)
    displs = [sum(counts[:q]) for q in range(n)]
    if variant != "a2av":
        comm.all_gather_v(send, recv, counts, displs, stream)
    else:
        comm.alltoall_v(send, [counts[r]] * n, [0] * n, recv, counts, displs, stream, dtype=H.HcclDataType.UINT8)


def calls_for(calls, n, nbytes):
    return max(3, min(calls, (1 << 29) // (n * n * nbytes)))


def row(mode, op, nbytes, variant, per_call_us):
    return {"mode": mode, "op": op, "bytes": nbytes, "variant": variant,
            "median_us": round(statistics.median(per_call_us), 2), "min_us": round(min(per_call_us), 2),
            "max_us": round(max(per_call_us), 2), "runs_us": [round(x, 2) for x in per_call_us]}


def loopback(n, runs, calls, emit):
    import torch
    import hccl_amd as H
    comms = H.loopback_world(n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    variants = {"one_sided": H.Algo.IPC, "schedule": H.Algo.MESH_ONESHOT, "a2av": H.Algo.IPC}
    for nbytes in SIZES:
        for op in OPS:
            bufs = [buffers(torch, op, n, r, nbytes) for r in range(n)]
            k = calls_for(calls, n, nbytes)
            times = {v: [] for v in variants}
            for run in range(runs + 1):  # run 0 warms up
                for v, algo in variants.items():
                    for c in comms:
                        c.set_algo(int(algo))
                    torch.cuda.synchronize()
                    gate = threading.Barrier(n + 1)

                    def body(r):
                        gate.wait()
                        for _ in range(k):
                            issue(H, comms[r], op, v, n, r, nbytes, bufs[r][0], bufs[r][1], streams[r])
                        streams[r].synchronize()

                    th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
                    for t in th:
                        t.start()
                    gate.wait()
                    t0 = time.perf_counter()
                    for t in th:
                        t.join()
                    dt = time.perf_counter() - t0
                    if run > 0:
                        times[v].append(dt / k * 1e6)
            for v in variants:
                emit(row(f"loopback{n}", op, nbytes, v, times[v]))
            del bufs
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()


def _pair_main(rank, n, port, runs, calls, q):
    os.environ.setdefault("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    import torch
    import torch.distributed as dist
    import hccl_amd as H
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n,
                            timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)

    def all_gather(b):
        out = [None] * n
        dist.all_gather_object(out, b)
        return out

    comm = H.comm_init_host_exchange(n, rank, all_gather)
    comm.set_algo(int(H.Algo.IPC))
    stream = torch.cuda.Stream()
    rows = []
    variants = ("one_sided", "a2av")
    for nbytes in SIZES:
        for op in OPS:
            send, recv = buffers(torch, op, n, rank, nbytes)
            k = calls_for(calls, n, nbytes)
            times = {v: [] for v in variants}
            for run in range(runs + 1):
                for v in variants:
                    torch.cuda.synchronize()
                    dist.barrier()
                    t0 = time.perf_counter()
                    for _ in range(k):
                        issue(H, comm, op, v, n, rank, nbytes, send, recv, stream)
                    stream.synchronize()
                    dt = time.perf_counter() - t0
                    if run > 0:
                        times[v].append(dt / k * 1e6)
            for v in variants:
                rows.append(row(f"rank{n}", op, nbytes, v, times[v]))
    dist.barrier()
    comm.destroy()
    dist.destroy_process_group()
    q.put((rank, rows))


def pair(runs, calls, emit):
    n = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_pair_main, args=(r, n, port, runs, calls, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in got[0]:  # rank 0's clock: a receiver of the Scatter
        emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scatter_gatherv_loopback_one_gpu.jsonl"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ranks", type=int, default=8)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            f.write(json.dumps(r) + "\n")
            f.flush()
            print(json.dumps({k: r[k] for k in ("mode", "op", "bytes", "variant", "median_us", "min_us", "max_us")}))

        pair(a.runs, a.calls, emit)  # before this process opens the GPU
        loopback(a.ranks, a.runs, a.calls, emit)


if __name__ == "__main__":
    main()
