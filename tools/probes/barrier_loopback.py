#!/usr/bin/env python3
"""HcclBarrier on one GPU: the one-sided kernel against the NHR token schedule and against the barrier the torch backend
used before the operator existed, a one-element int32 SUM AllReduce.

Loopback worlds of 2, 4 and 8 ranks (one process, every rank on its own thread and stream; the world's one-sided calls
are one launch for all ranks, issued behind every rank's stream). No figure here crosses xGMI: the flag words, the
tokens and the AllReduce's words all travel inside one device's memory, so these are enqueue and launch costs and say
nothing about link latency. Variants:
  one_sided  HcclBarrier under HCCL_AMD_ALGO_AUTO: k_ipc_barrier, one workgroup per rank
  nhr        HcclBarrier under HCCL_AMD_ALGO_NHR: ceil(log2 n) transport groups of one token each way
  allreduce  HcclAllReduce of one int32 under HCCL_AMD_ALGO_AUTO with the small-call rule on: the one-sided kernel's
             LL form, which is what a barrier cost before
Per world, `--runs` runs of `--calls` back-to-back calls per variant after a warm-up run, the variants taken in turn
inside every run so that drift hits them alike; the time is the host clock around all ranks' calls and their streams'
synchronisation, divided by the calls. A row per (world, variant): the runs' per-call microseconds, their median,
minimum and maximum. --trace adds the phase stamps of one one-sided call (HCCL_AMD_IPC_TRACE).

    python tools/probes/barrier_loopback.py --out profiles/barrier_loopback_one_gpu.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WORLDS = (2, 4, 8)
VARIANTS = ("one_sided", "nhr", "allreduce")


def row(n, variant, per_call_us, algo):
    return {"mode": f"loopback{n}", "variant": variant, "last_algo": algo,
            "median_us": round(statistics.median(per_call_us), 2), "min_us": round(min(per_call_us), 2),
            "max_us": round(max(per_call_us), 2), "runs_us": [round(x, 2) for x in per_call_us]}


def world(n, runs, calls, trace, emit):
    import torch
    import hccl_amd as H
    comms = H.loopback_world(n)
    for c in comms:
        c.set_config(H.Config.SMALL_IPC_BYTES, 1 << 20)  # the default, whatever the caller's environment says
    streams = [torch.cuda.Stream() for _ in range(n)]
    ones = [torch.ones(1, dtype=torch.int32, device="cuda") for _ in range(n)]
    algo_of = {"one_sided": H.Algo.AUTO, "nhr": H.Algo.NHR, "allreduce": H.Algo.AUTO}

    def issue(v, r):
        if v == "allreduce":
            comms[r].all_reduce(ones[r], ones[r], H.HcclReduceOp.SUM, streams[r])
        else:
            comms[r].barrier(streams[r])

    times = {v: [] for v in VARIANTS}
    used = {}
    for run in range(runs + 1):  # run 0 warms up
        for v in VARIANTS:
            for c in comms:
                c.set_algo(int(algo_of[v]))
            for o in ones:
                o.fill_(0)  # SUM of zeros: the values never grow
            torch.cuda.synchronize()
            gate = threading.Barrier(n + 1)

            def body(r):
                gate.wait()
                for _ in range(calls):
                    issue(v, r)
                streams[r].synchronize()

            th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
            for t in th:
                t.start()
            gate.wait()
            t0 = time.perf_counter()
            for t in th:
                t.join()
            dt = time.perf_counter() - t0
            used[v] = int(comms[0].last_algo)
            if run > 0:
                times[v].append(dt / calls * 1e6)
    for v in VARIANTS:
        emit(row(n, v, times[v], used[v]))
    if trace:
        for c in comms:
            c.set_algo(int(H.Algo.AUTO))
        torch.cuda.synchronize()
        th = [threading.Thread(target=lambda r=r: comms[r].barrier(streams[r])) for r in range(n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        stamps, blocks = comms[0].ipc_trace()
        # the slots k_ipc_barrier stamps (the others keep what an earlier launch of another kind left there)
        slots = {"entry": 0, "round": 1, "barrier1": 3, "exit": 7}
        for r in range(n):
            t = [int(x) for x in stamps[r][0]]
            emit({"mode": f"loopback{n}", "variant": "one_sided_trace", "rank": r, "blocks": blocks,
                  "ticks_100mhz_from_entry": {k: t[i] - t[0] for k, i in slots.items()}})
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "barrier_loopback_one_gpu.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    if a.trace:
        os.environ["HCCL_AMD_IPC_TRACE"] = "1"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            f.write(json.dumps(r) + "\n")
            f.flush()
            print(json.dumps({k: v for k, v in r.items() if k != "runs_us"}))

        for n in WORLDS:
            world(n, a.runs, a.calls, a.trace, emit)


if __name__ == "__main__":
    main()
