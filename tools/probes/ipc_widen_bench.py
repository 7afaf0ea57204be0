"""The one-sided widening FP8 AllReduce (k_ipc_widen, k_ipc_widen2) and the one-shot mesh schedule, one GPU.

  python tools/probes/ipc_widen_bench.py [--n 8] [--rounds 5] [--launches 10] [--paths ipc schedule] [--sizes BYTES ..]
                                         [--rev REV] [--label TEXT]

An n-rank loopback world, one thread per rank. For E4M3 -> FP32 and E4M3 -> BF16 at 64 KiB, 1 MiB and 16 MiB of input
per rank (--sizes), `rounds` rounds that alternate the chosen paths (--paths) of HcclAmdAllReduceWiden:
  ipc       HCCL_AMD_ALGO_IPC: one launch of the one-sided one-shot kernel per call;
  twoshot   HCCL_AMD_ALGO_IPC_TWOSHOT: one launch of the one-sided two-shot kernel per call;
  schedule  HCCL_AMD_ALGO_AUTO: the one-shot mesh schedule (transport groups and k_reduce_widen folds).
Every rank issues `launches` back-to-back calls between two device events on its stream; a round's time is the slowest
rank's, per call. One JSON line per case: the median and every round of each path, and the later paths' medians over the
first's. The one-shot kernel's load
width is fixed when the library is built (HCCL_AMD_IPC_WIDEN_LOAD_BYTES): run the probe once per library, candidates
in turn, and tell them apart by `label`. `rev` (the source revision) and `label` are copied into every line.
HBM stands in for xGMI here: the one-shot pushes n - 1 copies of every input, which costs bandwidth only on one GPU.
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


def timed(comms, sends, recvs, streams, launches):
    """us per call: `launches` calls on every rank, the slowest rank's span between its two events."""
    n = len(comms)
    spans, errs = [0.0] * n, []
    gate = threading.Barrier(n)

    def body(r):
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            gate.wait()
            e0.record(streams[r])
            for _ in range(launches):
                comms[r].all_reduce_widen(sends[r], recvs[r], streams[r])
            e1.record(streams[r])
            e1.synchronize()
            spans[r] = e0.elapsed_time(e1) * 1e3 / launches
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            gate.abort()

    threads = [threading.Thread(target=body, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    return max(spans)


PATHS = {"ipc": H.Algo.IPC, "twoshot": H.Algo.IPC_TWOSHOT, "schedule": H.Algo.AUTO}


def case(comms, odt, nbytes, rounds, launches, paths, extra):
    n = len(comms)
    g = torch.Generator(device="cuda").manual_seed(nbytes)
    # finite E4M3 bytes (exponent field below 15): exact sums, so every path must give the same bits
    sends = [(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g) & 0xF7)
             .view(torch.float8_e4m3fn) for _ in range(n)]
    recvs = [torch.empty(nbytes, dtype=odt, device="cuda") for _ in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    torch.cuda.synchronize()
    times, outs, ran = {name: [] for name in paths}, {}, {}
    for k in range(rounds + 1):  # round 0 warms every path up (set-up, compiled schedule) and is not kept
        for name in paths:
            for c in comms:
                c.set_algo(PATHS[name])
            t = timed(comms, sends, recvs, streams, launches)
            if k == 0:
                outs[name], ran[name] = recvs[0].clone(), H.Algo(comms[0].last_algo).name
            else:
                times[name].append(t)
    m = {name: statistics.median(ts) for name, ts in times.items()}
    row = {"probe": "ipc_widen_bench", **extra, "n": n, "in": "e4m3", "out": str(odt).split(".")[-1],
           "bytes_per_rank": nbytes, "ran": ran}
    for name in paths:
        row[f"{name}_us_median"], row[f"{name}_us"] = round(m[name], 1), [round(t, 1) for t in times[name]]
    for name in paths[1:]:
        row[f"{name}_over_{paths[0]}"] = round(m[name] / m[paths[0]], 2)
    row["bits_equal"] = all(bool(torch.equal(outs[paths[0]], outs[name])) for name in paths[1:])
    row["ipc_status"] = comms[0].ipc_status() & 1
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64 << 10, 1 << 20, 16 << 20])
    ap.add_argument("--paths", nargs="+", choices=sorted(PATHS), default=["ipc", "schedule"])
    ap.add_argument("--rev", default="")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ipc_widen_bench: no GPU; nothing is measured without one")
    comms = H.loopback_world(a.n)
    for c in comms:
        c.set_config(H.Config.IPC_TIMEOUT_MS, 20000)  # a stuck barrier ends the kernel with a status bit, never a hang
    try:
        for odt in (torch.float32, torch.bfloat16):
            for nbytes in a.sizes:
                case(comms, odt, nbytes, a.rounds, a.launches, a.paths, {"rev": a.rev, "label": a.label})
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


if __name__ == "__main__":
    main()
