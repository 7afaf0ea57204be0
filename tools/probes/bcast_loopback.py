#!/usr/bin/env python3
"""Broadcast on one GPU: the AllGather-based method it replaces against the two one-sided kinds and the schedule.

Two stand-ins for a node, both on one GPU (no figure here crosses xGMI): an 8-rank loopback world (one process, one
launch for all ranks) and a 2-process rank-mode pair (peers' staging opened from IPC handles). Sizes 1 KiB .. 64 MiB in
powers of four; per size and variant, `--runs` runs of `--calls` calls after a warm-up run, the variants taken in turn
inside every run so that drift hits them alike. Variants:
  parent    HcclAllGather of every rank's bytes into a world_size x bytes temporary, then a copy of the root's block
            (what ProcessGroupHCCL.broadcast did), the AllGather on the one-sided kernel
  parent_schedule  the same with the AllGather as its mesh schedule, which is what HCCL_AMD_ALGO_AUTO gave that method
            on a communicator with a send/recv transport (loopback world only)
  two_shot HcclBroadcast, kIpcBroadcast
  one_shot  HcclBroadcast, kIpcBroadcastOneShot
  schedule  HcclBroadcast, the mesh two-shot schedule (loopback world only: the pair has no send/recv transport)
A row per (mode, bytes, variant): the runs' per-call times in microseconds, their median, minimum and maximum.

    python tools/probes/bcast_loopback.py --out profiles/bcast_loopback_one_gpu.jsonl
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

SIZES = [1 << s for s in range(10, 27, 2)]
BCAST_ROOT = 1


def issue(comm, variant, buf, temp, stream, H):
    import torch
    if variant.startswith("parent"):
        m = buf.numel()
        comm.all_gather(buf, temp, stream)
        with torch.cuda.stream(stream):
            buf.copy_(temp[BCAST_ROOT * m:(BCAST_ROOT + 1) * m])
    else:
        comm.broadcast(buf, BCAST_ROOT, stream)


def configure(comm, variant, H):
    algo = {"schedule": H.Algo.MESH_TWOSHOT, "parent_schedule": H.Algo.MESH_ONESHOT}.get(variant, H.Algo.IPC)
    comm.set_algo(int(algo))
    comm.set_broadcast_kind({"two_shot": 1, "one_shot": 2}.get(variant, 0))


def row(mode, nbytes, variant, per_call_us):
    return {"mode": mode, "bytes": nbytes, "variant": variant, "median_us": round(statistics.median(per_call_us), 2),
            "min_us": round(min(per_call_us), 2), "max_us": round(max(per_call_us), 2),
            "runs_us": [round(x, 2) for x in per_call_us]}


def loopback(n, runs, calls, emit):
    import torch
    import hccl_amd as H
    comms = H.loopback_world(n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    variants = ["parent", "parent_schedule", "two_shot", "one_shot", "schedule"]
    for nbytes in SIZES:
        bufs = [torch.full((nbytes,), r, dtype=torch.uint8, device="cuda") for r in range(n)]
        temps = [torch.empty(nbytes * n, dtype=torch.uint8, device="cuda") for _ in range(n)]
        times = {v: [] for v in variants}
        for run in range(runs + 1):  # run 0 warms up
            for v in variants:
                for c in comms:
                    configure(c, v, H)
                torch.cuda.synchronize()
                gate = threading.Barrier(n + 1)

                def body(r, v=v):
                    gate.wait()
                    for _ in range(calls):
                        issue(comms[r], v, bufs[r], temps[r], streams[r], H)
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
                    times[v].append(dt / calls * 1e6)
        for v in variants:
            emit(row(f"loopback{n}", nbytes, v, times[v]))
        del bufs, temps
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
    stream = torch.cuda.Stream()
    variants = ["parent", "two_shot", "one_shot"]
    rows = []
    for nbytes in SIZES:
        buf = torch.full((nbytes,), rank, dtype=torch.uint8, device="cuda")
        temp = torch.empty(nbytes * n, dtype=torch.uint8, device="cuda")
        times = {v: [] for v in variants}
        for run in range(runs + 1):
            for v in variants:
                configure(comm, v, H)
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(calls):
                    issue(comm, v, buf, temp, stream, H)
                stream.synchronize()
                dt = time.perf_counter() - t0
                if run > 0:
                    times[v].append(dt / calls * 1e6)
        rows += [row(f"rank{n}", nbytes, v, times[v]) for v in variants]
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
    for r in got[0]:  # rank 0's clock: the non-root side, which ends with the data in place
        emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcast_loopback_one_gpu.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--ranks", type=int, default=8)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            f.write(json.dumps(r) + "\n")
            f.flush()
            print(json.dumps({k: r[k] for k in ("mode", "bytes", "variant", "median_us", "min_us", "max_us")}))

        pair(a.runs, a.calls, emit)  # before this process opens the GPU
        loopback(a.ranks, a.runs, a.calls, emit)


if __name__ == "__main__":
    main()
