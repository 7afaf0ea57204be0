"""The batched folds (LaunchReduceNBatch: k_reduceN_batch_rows, k_reduceN_batch) driven directly: fold-only IR programs
through HcclAmdCommExecute on a one-rank communicator. Consecutive REDUCE records with one operand count and
non-overlapping outputs are one batch (executor.cc, BatchRun), so each case below is one batched launch.

Every segment is head + 16-B vectors (full tiles + leftover vectors) + tail: all its operands and its output start one
element past a 16-B boundary, so the head is 3 elements for fp32 and 15 for int8. Each segment is compared bit for bit
with oracle.reduce_n, and every byte of the output buffer outside the segments' windows must keep its sentinel.

Which layout a case takes (RunBatch, reduce_kernels.hip): rows when totalVec * 16 / nseg < 4 MiB, that is when the
average segment has fewer than 262,144 vectors, flat otherwise.
  rows, 3 operands (tile 4 * 256 = 1024 vectors): nvec 2*1024+300 = 2348, 1024, 37      average 1136   -> rows
  rows, 2 operands (tile 256 vectors):            nvec 3*256+100 = 868, 5               average 436    -> rows
  mixed phase: the 3-operand rows shapes; the middle output one element off its sources' phase, so that segment takes
               the scalar kernel and the other two are batched                          average 1192   -> rows
  flat: nvec 257*1024+300 = 263,468 and 254*1024+904 = 261,000                          average 262,234 -> flat
        (524,468 * 16 / 2 = 4,195,744 B >= 4,194,304 B)
  flat, 8 segments (kMaxBatchSegs): the two flat shapes alternated, 4 * 524,468 / 8     average 262,234 -> flat
"""
import multiprocessing as mp
import os
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAT_MIN_AVG_VEC = (4 << 20) // 16
_ROWS3 = [(2 * 1024 + 300, 2), (1024, 0), (37, 3)]
_ROWS2 = [(3 * 256 + 100, 1), (5, 0)]
_FLAT = [(257 * 1024 + 300, 2), (254 * 1024 + 904, 1)]
# name -> (operands, [(vectors, tail elements)], index of the segment whose output is off phase or None, flat?)
CASES = {
    "rows3": (3, _ROWS3, None, False),
    "rows2": (2, _ROWS2, None, False),
    "rows3_mixed_phase": (3, _ROWS3, 1, False),
    "flat3": (3, _FLAT, None, True),
    "flat2": (2, _FLAT, None, True),
    "flat3_8seg": (3, _FLAT * 4, None, True),
}
DTYPES = ("fp32", "int8")


def _layout(nsrc, segs, off_phase, V):
    """Element offsets: per segment its count, operand starts in IN and output start in OUT, each one element past a
    16-B boundary (the off-phase output two past), with unused elements between neighbours."""
    head = V - 1
    plan, cin, cout = [], 0, 0

    def place(cur, extra=0):
        return (cur + V - 1) // V * V + 1 + extra

    for g, (nvec, tail) in enumerate(segs):
        count = head + nvec * V + tail
        srcs = []
        for _ in range(nsrc):
            s = place(cin)
            srcs.append(s)
            cin = s + count + 5
        d = place(cout, 1 if g == off_phase else 0)
        cout = d + count + 7
        plan.append((count, srcs, d))
    return plan, cin, cout + V


def test_cases_sit_on_the_intended_side_of_the_flat_threshold():
    """RunBatch's condition, from the batched segments' vector counts (the off-phase segment is not in the batch)."""
    for name, (_, segs, off, flat) in CASES.items():
        batched = [nvec for g, (nvec, _) in enumerate(segs) if g != off]
        assert len(segs) <= 8
        assert (sum(batched) * 16 // len(batched) >= 4 << 20) == flat, name
        assert (sum(batched) / len(batched) >= FLAT_MIN_AVG_VEC) == flat, name


def _worker(q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        import torch
        import hccl_amd as H
        from oracle import oracle as O
        from tests import _util as U
        from tests.test_gpu_rccl import _ir
        torch.cuda.set_device(0)
        comm = H.comm_init_root_info(1, H.get_root_info(), 0)
        stream = torch.cuda.Stream()
        IN, OUT = 0, 1
        results = {}
        for dname in DTYPES:
            dt = {"fp32": O.FP32, "int8": O.INT8}[dname]
            es = np.dtype(O.NP_STORAGE[dt]).itemsize
            V = 16 // es
            plans = {name: _layout(c[0], c[1], c[2], V) for name, c in CASES.items()}
            host_in = O.random_operands(dt, max(p[1] for p in plans.values()), seed=7 + es)
            dev_in = U.to_device(dt, host_in)
            for name, (nsrc, _, _, _) in CASES.items():
                plan, _, out_len = plans[name]
                prog = [_ir(H.IrKind.REDUCE, count, dst=(OUT, d), srcs=[(IN, s) for s in srcs])
                        for count, srcs, d in plan]
                arr = (H.HcclAmdIrOp * len(prog))(*prog)
                out = torch.empty(out_len, dtype=U.torch_dtype(dt), device="cuda")
                out.view(torch.uint8).fill_(0xA5)
                torch.cuda.synchronize()
                comm.execute(arr, len(prog), dev_in, out, H.HcclReduceOp.SUM, False, stream)
                torch.cuda.synchronize()
                got = U.to_host(dt, out)
                untouched = np.ones(out_len, dtype=bool)
                bad = []
                for g, (count, srcs, d) in enumerate(plan):
                    want = O.reduce_n(dt, O.SUM, [host_in[s:s + count] for s in srcs])
                    if not O.equal_bits(dt, got[d:d + count], want):
                        bad.append(g)
                    untouched[d:d + count] = False
                outside = got[untouched].view(np.uint8)
                results[(name, dname)] = (bad, int(np.count_nonzero(outside != 0xA5)), len(prog))
        comm.destroy()
        q.put(("ok", results))
    except Exception as e:  # noqa: BLE001
        q.put(("err", f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))


@pytest.fixture(scope="module")
def fold_results():
    """Every case on one communicator in one child process."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(q,))
    p.start()
    try:
        status, results = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert status == "ok", results
    return results


@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_batched_fold_segments_bit_exact_and_nothing_else_written(fold_results, name, dname):
    bad, overwritten, nseg = fold_results[(name, dname)]
    assert nseg == len(CASES[name][1])
    assert bad == [], f"segments differing from oracle.reduce_n: {bad}"
    assert overwritten == 0, f"{overwritten} bytes outside the segments' windows lost their sentinel"
