"""The widening FP8 sum (HcclAmdLocalReduceNWiden) against what a caller had before it.

  python tools/probes/widen_fold_bench.py [--mi 256] [--rounds 5] [--launches 20] [--rev REV] [--label TEXT]

For E4M3 -> FP32 and E4M3 -> BF16, nsrc in {2, 8}, `mi` Mi elements per operand, `rounds` rounds that alternate:
  new       `launches` back-to-back folds between two device events;
  baseline  torch decodes every operand to FP32 (x.to(torch.float32)), then HcclAmdLocalReduceN folds the FP32 copies
            (and, for BF16, torch narrows the result), repeated until at least `launches` kernels ran.
One JSON line per case: the median and every round of both times, the new kernel's algorithmic bytes
(nsrc + outSize) x count over its time and as a share of the 8 TB/s HBM peak, and baseline / new. The project's measured
rate of a same-type FP32 fold with the same stream count is in profiles/r02_stream_count_probe.jsonl (8 reads + 1 write:
5.71 TB/s). `rev` (the source revision) and `label` are copied into every line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import hccl_amd as H  # noqa: E402

PEAK_BPS = 8e12


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def case(odt, nsrc, count, rounds, launches, extra):
    g = torch.Generator(device="cuda").manual_seed(nsrc)
    # finite E4M3 bytes (exponent field below 15): the decode's speed does not depend on them, the check below does
    srcs = [(torch.randint(0, 256, (count,), dtype=torch.uint8, device="cuda", generator=g) & 0xF7)
            .view(torch.float8_e4m3fn) for _ in range(nsrc)]
    out = torch.empty(count, dtype=odt, device="cuda")
    base_out = torch.empty(count, dtype=torch.float32, device="cuda")

    def new():
        H.local_reduce_n_widen(out, srcs)

    def baseline():
        wide = [s.to(torch.float32) for s in srcs]
        H.local_reduce_n(base_out, wide)
        return base_out if odt == torch.float32 else base_out.to(odt)

    new()
    want = baseline()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out, want))  # exact sums: any order gives the same bits
    base_reps = max(1, -(-launches // (nsrc + 1)))
    t_new, t_base = [], []
    for _ in range(rounds):
        t_new.append(timed(new, launches))
        t_base.append(timed(baseline, base_reps))
    nbytes = (nsrc + out.element_size()) * count
    m_new, m_base = statistics.median(t_new), statistics.median(t_base)
    print(json.dumps({"probe": "widen_fold_bench", **extra, "in": "e4m3", "out": str(odt).split(".")[-1], "nsrc": nsrc,
                      "count": count, "bytes": nbytes, "new_us_median": round(m_new, 1),
                      "new_us": [round(t, 1) for t in t_new], "new_TBps": round(nbytes / m_new / 1e6, 3),
                      "new_share_of_8TBps": round(nbytes / (m_new * 1e-6) / PEAK_BPS, 3),
                      "baseline_us_median": round(m_base, 1), "baseline_us": [round(t, 1) for t in t_base],
                      "baseline_over_new": round(m_base / m_new, 2), "bits_equal": ok}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mi", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rev", default="")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("widen_fold_bench: no GPU; nothing is measured without one")
    extra = {"rev": a.rev, "label": a.label}
    for odt in (torch.float32, torch.bfloat16):
        for nsrc in (2, 8):
            case(odt, nsrc, a.mi << 20, a.rounds, a.launches, extra)


if __name__ == "__main__":
    main()
