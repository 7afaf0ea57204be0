"""Cost of the cross-rank argument check (HCCL_DFS_CONFIG=inconsistent_check) in a 2-rank loopback world.

  HCCL_AMD_HOST_PROFILE=1 python tools/probes/check_cost.py [--calls 1000] [--repeats 5] [--bytes 4096]

For the switch off and on, on worlds built from the same library: `repeats` times, every rank enqueues `calls`
back-to-back AllReduces (fp32 sum, one-sided family) with no host synchronisation in between; rank 0's stream is timed
with events around the batch. Prints one JSON line per switch value: the median and all repeats of the time per call,
and the host time per collective entry (the ENTRY category of HcclAmdHostProfile, all ranks' calls together).
One-GPU loopback figures: both ranks share the device, the round trip is not an xGMI one, and every call of a loopback
world pays host rendezvous between the rank threads, two more with the check on.
"""
import argparse
import json
import os
import statistics
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import hccl_amd as H  # noqa: E402


def run(mode, calls, repeats, nbytes):
    n = 2
    comms = H.loopback_world(n)
    for c in comms:
        c.set_algo(int(H.Algo.IPC))
        c.set_config(H.Config.INCONSISTENT_CHECK, mode)
    streams = [torch.cuda.Stream() for _ in range(n)]
    x = [torch.ones(nbytes // 4, device="cuda") for _ in range(n)]
    y = [torch.zeros(nbytes // 4, device="cuda") for _ in range(n)]
    times = []

    def batch(r, k, e0=None, e1=None):
        with torch.cuda.stream(streams[r]):
            if e0 is not None and r == 0:
                e0.record()
            for _ in range(k):
                comms[r].all_reduce(x[r], y[r], int(H.HcclReduceOp.SUM), streams[r])
            if e1 is not None and r == 0:
                e1.record()

    def all_ranks(*args):
        th = [threading.Thread(target=batch, args=(r,) + args) for r in range(n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()

    all_ranks(20)  # set-up and warm-up
    H.host_profile(reset=True)
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        all_ranks(calls, e0, e1)
        times.append(e0.elapsed_time(e1) * 1e3 / calls)
    ns, entries = H.host_profile(reset=True)["entry"]
    ok = all(c.async_error() == 0 for c in comms) and bool((y[0] == n).all())
    launches = comms[0].check_launches()
    for c in comms:
        c.destroy()
    return {"inconsistent_check": mode, "ranks": n, "bytes": nbytes, "calls": calls,
            "us_per_call_median": round(statistics.median(times), 3), "us_per_call": [round(t, 3) for t in times],
            "host_entry_us_per_call": round(ns / max(1, entries) / 1e3, 3) if entries else None,
            "check_launches": launches, "ok": ok}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=4096)
    a = ap.parse_args()
    for mode in (-1, 1):
        print(json.dumps(run(mode, a.calls, a.repeats, a.bytes)), flush=True)
