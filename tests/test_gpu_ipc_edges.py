"""Misaligned, tiny and guarded buffers on the one-sided reducing kernel, and guards on the executor path.

The staged kernel takes 16-byte vectors for a chunk only when every buffer of the launch is 16-byte aligned
(IpcArgs::aligned: this rank's pair in rank mode, the AND over every rank's pair in a loopback world) and the chunk
starts on the vector grid (ipc_kernel_body.h ChunkVec); the LL form reads its input words bytewise when a block's base
is not 4-byte aligned or a word straddles the end (LoadWord), and unpacks and folds through the same vector decision.
Here every rank's send buffer is a view some elements into a larger tensor and every receive buffer a view into an
allocation filled with 0xA5 (64 bytes of guard on each side, tests/test_gpu_reduce_edges.py Placed). After each call:
the family that ran, no barrier timeout, the LL launch counter, the output against the oracle replaying the twin
schedule on the shifted slices (the AIV engine: its closed forms), the guards, the send buffers, and a non-root Reduce
output still holding its fill.

Shift patterns, in elements (send, recv), V = 16 / itemsize: every rank (1, 1); every rank (0, V - 1); every rank
(V - 1, 0); only the last rank (1, 1) (the world's `aligned` is false while most pointers are aligned); INT8 in the LL
form at (2, 2) (2-byte but not 4-byte aligned: LoadWord's bytewise branch); and, at n = 3 and 4, every rank (0, 0):
the only pattern in which a loopback world's `aligned` is true, so the only one in which ChunkVec's second condition
(the chunk's start on the vector grid) decides anything, with the guards around the vector stores.
Counts (per rank; per block for a ReduceScatter): 1, V - 1, V + 1, n V + 1 (chunks of about one vector whose starts
leave the vector grid), 4099; the LL form also 3 and 21 (= 4 k + 1). The dtype sweep adds one vector more than the
blockElems HcclAmdIpcPlan reports at 4099 and, in the LL form, the largest LL count, 65536 / itemsize.

Pruning of operation x family x n x dtype x op x shift x count to what the code distinguishes:
* shift sweep: every (operation, family) pair, LL forms included, meets every shift pattern in FP32 and INT8 (SUM) at
  n = 2, 3, 4 (RHD: 2, 4; the aligned pattern: 3, 4), the counts above looped inside the case;
* dtype sweep: INT8, BFP16 (SUM and MAX each), FP32, FP64 meet every count, the two extra ones included, on one family
  of each kernel form: the staged one-shot (AllReduce, family 9), the staged two-shot (AllReduce, family 7), RHD
  (family 12) and the LL form (AllReduce, auto), every rank shifted (1, 1), n = 3 (RHD: 4);
* the AIV engine has no FP64 (SelectAivAlgo does not match it), so its pairs run FP32 and INT8 only.
The staged cases run with HCCL_AMD_IPC_LL_BYTES = 0: with the default, 64 KiB, every one-shot AllReduce and every
ReduceScatter of these sizes would take the LL form whatever family is asked for.
"""
import datetime
import multiprocessing as mp
import os
import socket
import time
import traceback

import numpy as np
import pytest
import torch

import hccl_amd as H
from oracle import oracle as O
from tests import sched_ref as R
from tests.test_gpu_collectives import AG, AR, RED, RS, _ipc_twin, aiv_expected, oracle_replay, run_ranks
from tests.test_gpu_reduce_edges import FILL, GUARD, Placed, check_window

pytestmark = pytest.mark.gpu

CORE_LIMIT = 48  # the AIV engine's default vector-core count (HCCL_AMD_AIV_CORE_LIMIT)
LL_BYTES = 64 << 10
SMALL_BYTES = 1 << 20
TWOSHOT, AUTO9, AIV, RHD12 = int(H.Algo.IPC_TWOSHOT), int(H.Algo.IPC), int(H.Algo.AIV), int(H.Algo.IPC_RHD)
KIND_NAMES = {AR: "allreduce", RS: "reducescatter", RED: "reduce", AG: "allgather"}

# (operation, family) on the staged kernel, and (operation, family asked for, family that runs) in the LL form
STAGED_PAIRS = [(AR, TWOSHOT), (AR, AUTO9), (RS, TWOSHOT), (RS, AUTO9), (RED, TWOSHOT), (RED, AUTO9), (AR, RHD12),
                (AR, AIV), (RS, AIV), (AG, AUTO9)]
LL_PAIRS = [(AR, int(H.Algo.AUTO), AUTO9), (AR, int(H.Algo.RHD), RHD12), (RS, int(H.Algo.AUTO), AUTO9)]
PATTERNS = ["all", "recv", "send", "last"]


def _es(dtype):
    return np.dtype(O.NP_STORAGE[dtype]).itemsize


def shifts_of(pattern, n, dtype):
    v = 16 // _es(dtype)
    if pattern == "last":
        return [(0, 0)] * (n - 1) + [(1, 1)]
    return [{"all": (1, 1), "recv": (0, v - 1), "send": (v - 1, 0), "two": (2, 2), "aligned": (0, 0)}[pattern]] * n


def counts_of(n, dtype, ll):
    v = 16 // _es(dtype)
    c = [1, v - 1, v + 1, n * v + 1, 4099] + ([3, 21] if ll else [])
    return sorted({x for x in c if x > 0})


def _cases():
    out = []
    for pattern in PATTERNS + ["aligned"]:
        for dtype in (O.FP32, O.INT8):
            for n in ((3, 4) if pattern == "aligned" else (2, 3, 4)):
                for kind, fam in STAGED_PAIRS:
                    if fam != RHD12 or n != 3:
                        out.append(("staged", kind, fam, fam, n, dtype, O.SUM, pattern, False))
                for kind, ask, fam in LL_PAIRS:
                    if fam != RHD12 or n != 3:
                        out.append(("ll", kind, ask, fam, n, dtype, O.SUM, pattern, False))
    for dtype, op in ((O.INT8, O.SUM), (O.INT8, O.MAX), (O.BFP16, O.SUM), (O.BFP16, O.MAX), (O.FP32, O.SUM),
                      (O.FP64, O.SUM)):
        out.append(("staged", AR, AUTO9, AUTO9, 3, dtype, op, "all", True))
        out.append(("staged", AR, TWOSHOT, TWOSHOT, 3, dtype, op, "all", True))
        out.append(("staged", AR, RHD12, RHD12, 4, dtype, op, "all", True))
        out.append(("ll", AR, int(H.Algo.AUTO), AUTO9, 3, dtype, op, "all", True))
    for n in (2, 3, 4):
        for kind, ask, fam in LL_PAIRS:
            if fam != RHD12 or n != 3:
                out.append(("ll", kind, ask, fam, n, O.INT8, O.SUM, "two", False))
    return out


def _case_id(c):
    form, kind, ask, fam, n, dtype, op, pattern, full = c
    return (f"{form}-{KIND_NAMES[kind]}-f{fam}-n{n}-{O.DTYPE_NAMES[dtype]}-{O.OP_NAMES[op]}-{pattern}"
            + ("-allcounts" if full else ""))


@pytest.fixture(scope="module")
def edge_worlds():
    cache = {}

    def get(n):
        if n not in cache:
            comms = H.loopback_world(n)
            for c in comms:
                c.set_config(H.Config.IPC_TIMEOUT_MS, 20000)  # a stuck barrier fails the test, never hangs the box
                c.set_config(H.Config.AIV_CORE_LIMIT, CORE_LIMIT)
            cache[n] = (comms, [torch.cuda.Stream() for _ in range(n)])
        return cache[n]

    yield get
    torch.cuda.synchronize()
    for comms, _ in cache.values():
        for c in comms:
            c.destroy()


def configure(comms, small, ll):
    for c in comms:
        c.set_config(H.Config.SMALL_IPC_BYTES, small)
        c.set_config(H.Config.IPC_LL_BYTES, ll)


def run_shifted(world, kind, algo, dtype, op, xs, count, shifts, root):
    """collective() of test_gpu_collectives.py with per-rank element shifts (send, recv) and guarded allocations.
    Returns (family that ran, LL launches of the call, sends, recvs) as Placed allocations."""
    comms, streams = world
    n = len(comms)
    sends = [Placed(dtype, shifts[r][0], len(xs[r]), xs[r]) for r in range(n)]
    recvs = [Placed(dtype, shifts[r][1], count * n if kind == AG else count) for r in range(n)]
    for c in comms:
        c.set_algo(algo)
    torch.cuda.synchronize()
    before = comms[0].ipc_ll_launches()

    def body(r):
        if kind == AR:
            comms[r].all_reduce(sends[r].win, recvs[r].win, op, streams[r])
        elif kind == RS:
            comms[r].reduce_scatter(sends[r].win, recvs[r].win, op, streams[r])
        elif kind == AG:
            comms[r].all_gather(sends[r].win, recvs[r].win, streams[r])
        else:
            comms[r].reduce(sends[r].win, recvs[r].win, root, op, streams[r])

    try:
        run_ranks(n, body)
        torch.cuda.synchronize()
        used = comms[0].last_algo
    finally:
        for c in comms:
            c.set_algo(0)
    return used, comms[0].ipc_ll_launches() - before, sends, recvs


def expected(kind, fam, n, count, dtype, op, xs, root):
    """The oracle's outputs for family `fam` of the one-sided kernel (or a schedule family of the executor)."""
    if fam == AIV:
        variant, want = aiv_expected(kind, dtype, op, xs, count, n, CORE_LIMIT)
        assert variant != R.AIV_NOT_MATCHED
        return want
    twin = _ipc_twin(kind, fam, n, count, dtype, op) if fam in (TWOSHOT, AUTO9, RHD12) else fam
    return oracle_replay(kind, twin, n, count, dtype, op, xs, root, 0)


def check_call(what, kind, n, dtype, root, want, sends, recvs):
    for r in range(n):
        if kind == RED and r != root:
            assert recvs[r].unchanged(), f"{what}: non-root rank {r} output (or its guard) written"
        else:
            recvs[r].check_output(want[r], f"{what} rank {r}")
        assert sends[r].unchanged(), f"{what}: rank {r} send buffer (or its guard) written"


def _special(dtype, op):
    return dtype in (O.INT64, O.UINT64, O.FP64) or op == O.PROD


def window_count(kind, fam, n, dtype, op, ll):
    """One vector more than the blockElems of the plan at 4099 elements: more than one block window."""
    es = _es(dtype)
    sched = {TWOSHOT: R.ALGO_TWOSHOT, RHD12: RHD12}.get(fam)
    if sched is None:
        sched = H.select_algo(kind, n, 4099 * es, _special(dtype, op))
    _, launches = H.ipc_plan(kind, n, 4099, dtype, family=sched, sharedDevice=1, llBytes=LL_BYTES if ll else 0)
    count = int(launches[0].blockElems) + 16 // es
    res, launches = H.ipc_plan(kind, n, count, dtype, family=sched, sharedDevice=1, llBytes=LL_BYTES if ll else 0)
    assert res.ll == (1 if ll else 0) and launches[0].blockElems < count, (count, launches[0].blockElems)
    return count


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_one_sided_edges(edge_worlds, case):
    form, kind, ask, fam, n, dtype, op, pattern, full = case
    ll = form == "ll"
    world = edge_worlds(n)
    configure(world[0], SMALL_BYTES if ll else 0, LL_BYTES if ll else 0)
    shifts = shifts_of(pattern, n, dtype)
    root = n - 1
    counts = counts_of(n, dtype, ll)
    if full:
        counts.append(window_count(kind, fam, n, dtype, op, ll))
        if ll:
            counts.append(LL_BYTES // _es(dtype))
    for count in counts:
        what = f"{_case_id(case)} count {count}"
        in_count = count * n if kind == RS else count
        xs = [O.random_operands(dtype, in_count, seed=7000 + 31 * count + r) for r in range(n)]
        used, ll_launches, sends, recvs = run_shifted(world, kind, ask, dtype, op, xs, count, shifts, root)
        assert used == fam, f"{what}: ran {H.Algo(used).name}"
        assert world[0][0].ipc_status() & 1 == 0, f"{what}: barrier timeout"
        assert ll_launches == (1 if ll else 0), f"{what}: {ll_launches} LL launches"
        want = expected(kind, fam, n, count, dtype, op, xs, root)
        check_call(what, kind, n, dtype, root, want, sends, recvs)


# ------------------------------------------------------------------------------------------------ the executor path

@pytest.mark.parametrize("dtype", [O.FP32, O.INT8], ids=lambda v: O.DTYPE_NAMES[v])
@pytest.mark.parametrize("kind,fam", [(AR, R.ALGO_ONESHOT), (AR, R.ALGO_TWOSHOT), (AR, R.ALGO_NHR),
                                      (RS, R.ALGO_ONESHOT)])
def test_executor_path_guards(edge_worlds, kind, fam, dtype):
    """The schedules (executor, LaunchReduceN, the copy kernels) into misaligned, guarded receive buffers."""
    n = 4
    world = edge_worlds(n)
    configure(world[0], 0, LL_BYTES)
    for pattern in ("all", "recv"):
        shifts = shifts_of(pattern, n, dtype)
        for count in (16 // _es(dtype) + 1, 4099):
            what = f"{KIND_NAMES[kind]} family {fam} {O.DTYPE_NAMES[dtype]} {pattern} count {count}"
            xs = [O.random_operands(dtype, count * n if kind == RS else count, seed=7600 + 31 * count + r)
                  for r in range(n)]
            used, ll_launches, sends, recvs = run_shifted(world, kind, fam, dtype, O.SUM, xs, count, shifts, 0)
            assert used == fam and ll_launches == 0, f"{what}: ran {H.Algo(used).name}"
            check_call(what, kind, n, dtype, 0, expected(kind, fam, n, count, dtype, O.SUM, xs, 0), sends, recvs)


# ------------------------------------------------------------------------------------------------ rank mode

RANK_N, RANK_ROOT = 2, 1


def _rank_cases():
    out = []
    for dtype in (O.INT8, O.FP32):
        for count in (16 // _es(dtype) + 1, 4099):
            for kind, ll in ((AR, False), (RS, False), (RED, False), (AG, False), (AR, True), (RS, True)):
                out.append((kind, ll, dtype, count))
    return out


def _rank_inputs(i, case):
    kind, _, dtype, count = case
    return [O.random_operands(dtype, count * RANK_N if kind == RS else count, seed=7800 + 13 * i + r)
            for r in range(RANK_N)]


def _rank_shift(rank, dtype):
    return (1, 16 // _es(dtype) - 1) if rank == 1 else (0, 0)  # only rank 1 is misaligned


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"  # a lost peer shows as a status bit, never a hang
    try:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=RANK_N,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)

        def all_gather(b):
            out = [None] * RANK_N
            dist.all_gather_object(out, b)
            return out

        comm = H.comm_init_host_exchange(RANK_N, rank, all_gather)
        comm.set_algo(AUTO9)
        stream = torch.cuda.Stream()
        results = []
        for i, case in enumerate(_rank_cases()):
            kind, ll, dtype, count = case
            comm.set_config(H.Config.IPC_LL_BYTES, LL_BYTES if ll else 0)
            si, so = _rank_shift(rank, dtype)
            x = _rank_inputs(i, case)[rank]
            send = Placed(dtype, si, len(x), x)
            recv = Placed(dtype, so, count * RANK_N if kind == AG else count)
            torch.cuda.synchronize()
            before = comm.ipc_ll_launches()
            if kind == AR:
                comm.all_reduce(send.win, recv.win, O.SUM, stream=stream)
            elif kind == RS:
                comm.reduce_scatter(send.win, recv.win, O.SUM, stream=stream)
            elif kind == AG:
                comm.all_gather(send.win, recv.win, stream=stream)
            else:
                comm.reduce(send.win, recv.win, RANK_ROOT, O.SUM, stream=stream)
            stream.synchronize()
            status = comm.ipc_status()
            results.append((i, status, comm.last_algo, comm.ipc_ll_launches() - before, recv.bytes_now(), recv.lo,
                            recv.hi, send.unchanged()))
            if max(all_gather(status & 1)) != 0:  # every rank stops together after a barrier timeout anywhere
                break
        dist.barrier()
        comm.destroy()  # collective: no rank unmaps while a peer's kernel may still store into it
        dist.destroy_process_group()
        q.put((rank, "ok", results))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)  # peers' kernels are bounded: let them drain before this process's memory goes away


def test_rank_mode_one_rank_misaligned():
    """Two processes on the one GPU, rank 1's buffers at (1, V - 1) and rank 0's aligned: the only place where
    IpcArgs::aligned differs between the ranks of one call. Family 9 on the staged kernel (AllReduce, ReduceScatter,
    Reduce, AllGather) and in the LL form (AllReduce, ReduceScatter), INT8 and FP32, V + 1 and 4099 elements."""
    cases = _rank_cases()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, port, q)) for r in range(RANK_N)]
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
    for r in range(RANK_N):
        assert got[r][0] == "ok", f"rank {r}:\n{got[r][0]}"
        assert len(got[r][1]) == len(cases), f"rank {r} stopped after case {len(got[r][1]) - 1}"
    for i, case in enumerate(cases):
        kind, ll, dtype, count = case
        xs = _rank_inputs(i, case)
        want = expected(kind, AUTO9, RANK_N, count, dtype, O.SUM, xs, RANK_ROOT)
        for r in range(RANK_N):
            what = f"rank {r} {KIND_NAMES[kind]} ll {ll} {O.DTYPE_NAMES[dtype]} count {count}"
            _, status, algo, ll_launches, out, lo, hi, send_ok = got[r][1][i]
            assert status & 1 == 0, f"{what}: barrier timeout (status {status:#x})"
            assert algo == AUTO9, f"{what}: ran {algo}"
            assert ll_launches == (1 if ll else 0), f"{what}: {ll_launches} LL launches"
            assert send_ok, f"{what}: send buffer (or its guard) written"
            if kind == RED and r != RANK_ROOT:
                assert np.all(out == FILL), f"{what}: non-root output written"
            else:
                assert lo >= GUARD and len(out) - hi >= GUARD
                check_window(dtype, out, lo, hi, want[r], what)
