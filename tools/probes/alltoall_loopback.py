#!/usr/bin/env python3
"""All-to-all on one GPU: the one-sided kernel against the mesh schedule, for even and skewed count matrices.

Two stand-ins for a node, both on one GPU (no figure here crosses xGMI): an 8-rank loopback world (one process, one
launch for all ranks) and a 2-process rank-mode pair (peers' staging opened from IPC handles; it has no send/recv
transport, so only the one-sided kernel runs there). Sizes 1 KiB .. 64 MiB per pair in powers of four; per size, matrix
and variant, `--runs` runs of up to `--calls` calls after a warm-up run (fewer calls at the large sizes), the variants
taken in turn inside every run so that drift hits them alike. Matrices:
  even    every pair moves `bytes`: HcclAlltoAll (every rank knows the counts: the host sets tier, blocks and rounds)
  skewed  pair (0, n - 1) moves `bytes`, every other pair a sixteenth of it: HcclAlltoAllV (count-free host decisions:
          the small staging tier, blocks from its capacity, the round count agreed on the device)
Variants: one_sided (HCCL_AMD_ALGO_IPC), schedule (the mesh schedule, one transport group).
A row per (mode, matrix, bytes, variant): the runs' per-call times in microseconds, their median, minimum and maximum.

    python tools/probes/alltoall_loopback.py --out profiles/alltoall_loopback_one_gpu.jsonl
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
MATRICES = ("even", "skewed")


def matrix(kind, n, nbytes):
    if kind == "even":
        return [[nbytes] * n for _ in range(n)]
    m = [[max(1, nbytes // 16)] * n for _ in range(n)]
    m[0][n - 1] = nbytes
    return m


def layout(m, r):
    n = len(m)
    sc = [m[r][q] for q in range(n)]
    rc = [m[q][r] for q in range(n)]
    return sc, [sum(sc[:q]) for q in range(n)], rc, [sum(rc[:q]) for q in range(n)]


def issue(comm, kind, send, recv, lay, stream):
    if kind == "even":
        comm.alltoall(send, recv, stream)
    else:
        comm.alltoall_v(send, lay[0], lay[1], recv, lay[2], lay[3], stream)


def calls_for(calls, n, nbytes):
    return max(3, min(calls, (1 << 29) // (n * n * nbytes)))


def row(mode, kind, nbytes, variant, per_call_us):
    return {"mode": mode, "matrix": kind, "bytes": nbytes, "variant": variant,
            "median_us": round(statistics.median(per_call_us), 2), "min_us": round(min(per_call_us), 2),
            "max_us": round(max(per_call_us), 2), "runs_us": [round(x, 2) for x in per_call_us]}


def loopback(n, runs, calls, emit):
    import torch
    import hccl_amd as H
    comms = H.loopback_world(n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    variants = {"one_sided": H.Algo.IPC, "schedule": H.Algo.MESH_ONESHOT}
    for nbytes in SIZES:
        for kind in MATRICES:
            m = matrix(kind, n, nbytes)
            lays = [layout(m, r) for r in range(n)]
            sends = [torch.full((sum(lays[r][0]),), r, dtype=torch.uint8, device="cuda") for r in range(n)]
            recvs = [torch.empty(sum(lays[r][2]), dtype=torch.uint8, device="cuda") for r in range(n)]
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
                            issue(comms[r], kind, sends[r], recvs[r], lays[r], streams[r])
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
                emit(row(f"loopback{n}", kind, nbytes, v, times[v]))
            del sends, recvs
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
    for nbytes in SIZES:
        for kind in MATRICES:
            lay = layout(matrix(kind, n, nbytes), rank)
            send = torch.full((sum(lay[0]),), rank, dtype=torch.uint8, device="cuda")
            recv = torch.empty(sum(lay[2]), dtype=torch.uint8, device="cuda")
            k = calls_for(calls, n, nbytes)
            times = []
            for run in range(runs + 1):
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(k):
                    issue(comm, kind, send, recv, lay, stream)
                stream.synchronize()
                dt = time.perf_counter() - t0
                if run > 0:
                    times.append(dt / k * 1e6)
            rows.append(row(f"rank{n}", kind, nbytes, "one_sided", times))
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
    for r in got[1]:  # rank 1's clock: the receiver of the skewed matrix's large pair
        emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alltoall_loopback_one_gpu.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--ranks", type=int, default=8)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            f.write(json.dumps(r) + "\n")
            f.flush()
            print(json.dumps({k: r[k] for k in ("mode", "matrix", "bytes", "variant", "median_us", "min_us", "max_us")}))

        pair(a.runs, a.calls, emit)  # before this process opens the GPU
        loopback(a.ranks, a.runs, a.calls, emit)


if __name__ == "__main__":
    main()
