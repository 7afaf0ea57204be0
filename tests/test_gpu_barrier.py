"""HcclBarrier on the GPU: the one-sided kernel (k_ipc_barrier, kind kIpcBarrier) and the token schedules.

The staggered check, which tells a barrier from a no-op: n ranks of a loopback world, each on its own stream and host
thread. In iteration i one rank (rotating) first enqueues a device delay of some tens of milliseconds; then every rank
records pre[r], writes i into its word of a shared device array, calls HcclBarrier, records post[r] and copies the
whole array into seen[r]. After synchronising, seen[r] must be all i for every r (every rank's write, the delayed one's
included, came before any rank's copy), and pre[q] must not be later than post[r] for any pair. Without a barrier the
undelayed ranks copy the array tens of milliseconds before the delayed rank writes its word.
"""
import multiprocessing as mp
import os
import traceback

import pytest
import torch

import hccl_amd as H
from oracle import oracle as O
from test_gpu_barrier_ranks import REPLAYS, sleep_cycles, spawn
from tests._util import to_device, to_host
from tests.test_gpu_collectives import oracle_replay, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, IPC, NHR, MESH = (int(H.Algo[k]) for k in ("AUTO", "IPC", "NHR", "MESH_ONESHOT"))
ITERS = 3
SMALL_IPC = 1 << 20  # the small-call rule's default bound (the suite's environment turns the rule off)


@pytest.fixture(autouse=True)
def bounded_waits(monkeypatch):
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")  # a stuck barrier fails the test, never hangs the box


@pytest.fixture(scope="module")
def cycles():
    return sleep_cycles(torch)


def destroy(comms):
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()


def staggered(comms, cycles, iters=ITERS):
    """The check of the module's docstring; returns nothing, asserts everything."""
    n = len(comms)
    streams = [torch.cuda.Stream() for _ in range(n)]
    marks = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    seen = [torch.full((n,), -2, dtype=torch.int64, device="cuda") for _ in range(n)]
    for i in range(iters):
        pre = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        post = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        d0, d1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()  # every copy of the previous iteration has ended before a word changes

        def body(r):
            with torch.cuda.stream(streams[r]):
                if r == i % n:
                    d0.record()
                    torch.cuda._sleep(cycles)
                    d1.record()
                pre[r].record()
                marks[r:r + 1].fill_(i)
                comms[r].barrier(streams[r])
                post[r].record()
                seen[r].copy_(marks)

        run_ranks(n, body)
        torch.cuda.synchronize()
        assert d0.elapsed_time(d1) > 5.0  # the delay was there: milliseconds, against a barrier's microseconds
        for r in range(n):
            assert seen[r].tolist() == [i] * n, (n, i, r, seen[r].tolist())
        for q in range(n):
            for r in range(n):
                assert pre[q].elapsed_time(post[r]) >= 0, (n, i, q, r)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_one_sided_barrier_in_a_loopback_world(monkeypatch, n, cycles):
    """AUTO takes the one-sided kernel although the suite turns the small-call rule off: a barrier has no bytes. A fresh
    world's first barrier sets up the flags and status words and no staging tier: the communicator then holds less than
    the smallest tier alone would take (the small tier under the default configuration, n x 1 MiB per area)."""
    monkeypatch.setenv("HCCL_AMD_SMALL_IPC_BYTES", str(SMALL_IPC))
    comms = H.loopback_world(n)
    try:
        assert [c.device_bytes() for c in comms] == [0] * n
        streams = [torch.cuda.Stream() for _ in range(n)]
        run_ranks(n, lambda r: comms[r].barrier(streams[r]))
        torch.cuda.synchronize()
        tier, _ = H.ipc_plan(H.OpType.ALLREDUCE, n, 70001, O.FP32, family=int(H.Algo.MESH_TWOSHOT))
        tier_bytes = 2 * tier.areaBytes + 2 * tier.altBytes
        assert tier.areaBytes == n * SMALL_IPC  # the plan names the small tier
        held = [c.device_bytes() for c in comms]
        print(f"n={n}: {held[0]} B held after the first barrier, smallest tier {tier_bytes} B")
        assert all(0 < b < tier_bytes for b in held), (held, tier_bytes)
        assert all(c.last_algo == IPC for c in comms)
        staggered(comms, cycles)
        assert all(c.last_algo == IPC for c in comms)
        assert [c.device_bytes() for c in comms] == held  # no later barrier allocates
        assert all(c.scratch() == (0, 0) for c in comms)
        assert comms[0].ipc_status() & 1 == 0
    finally:
        destroy(comms)


def test_epochs_between_other_one_sided_calls():
    """LL AllReduce of 1 KiB, Barrier, AllReduce of 1 MiB (many workgroups), Barrier, Barrier, Scatter of 64 KiB,
    Barrier, ReduceScatter of 256 KiB on one world, every rank enqueueing the whole sequence with no host
    synchronisation in between: the barrier's epoch is one that workgroups b >= 1 never see, and it flips the parity of
    the single-barrier kinds' alternate areas. Every result bit-exact against the oracle's replay of the auto schedule."""
    n, root = 4, 2
    comms = H.loopback_world(n)
    try:
        for c in comms:
            c.set_config(H.Config.SMALL_IPC_BYTES, SMALL_IPC)
        ar_small, ar_big, sc_count, rs_count = 256, 1 << 18, (64 << 10) // 4 // n, (256 << 10) // 4 // n
        xs_small = [O.random_operands(O.FP32, ar_small, seed=9100 + r) for r in range(n)]
        xs_big = [O.random_operands(O.FP32, ar_big, seed=9200 + r) for r in range(n)]
        xs_rs = [O.random_operands(O.FP32, rs_count * n, seed=9300 + r) for r in range(n)]
        sc_src = torch.randint(-2**31, 2**31 - 1, (n * sc_count,), dtype=torch.int32, device="cuda")
        d_small, d_big, d_rs = ([to_device(O.FP32, x) for x in xs] for xs in (xs_small, xs_big, xs_rs))
        o_small = [torch.zeros_like(t) for t in d_small]
        o_big = [torch.zeros_like(t) for t in d_big]
        o_rs = [torch.zeros(rs_count, dtype=d_rs[0].dtype, device="cuda") for _ in range(n)]
        o_sc = [torch.zeros(sc_count, dtype=torch.int32, device="cuda") for _ in range(n)]
        streams = [torch.cuda.Stream() for _ in range(n)]
        algos = [[] for _ in range(n)]
        ll_before = comms[0].ipc_ll_launches()
        torch.cuda.synchronize()

        def body(r):
            c, s = comms[r], streams[r]
            steps = [
                lambda: c.all_reduce(d_small[r], o_small[r], O.SUM, s),
                lambda: c.barrier(s),
                lambda: c.all_reduce(d_big[r], o_big[r], O.SUM, s),
                lambda: c.barrier(s),
                lambda: c.barrier(s),
                lambda: c.scatter(sc_src if r == root else None, o_sc[r], root, s),
                lambda: c.barrier(s),
                lambda: c.reduce_scatter(d_rs[r], o_rs[r], O.SUM, s),
            ]
            for step in steps:
                step()
                algos[r].append(c.last_algo)

        run_ranks(n, body)
        torch.cuda.synchronize()
        assert all(a == [IPC] * 8 for a in algos), algos
        assert comms[0].ipc_ll_launches() > ll_before  # the 1 KiB AllReduce ran in the LL form
        want_small = oracle_replay(0, AUTO, n, ar_small, O.FP32, O.SUM, xs_small, 0, 0)
        want_big = oracle_replay(0, AUTO, n, ar_big, O.FP32, O.SUM, xs_big, 0, 0)
        want_rs = oracle_replay(1, AUTO, n, rs_count, O.FP32, O.SUM, xs_rs, 0, 0)
        for r in range(n):
            assert O.equal_bits(O.FP32, to_host(O.FP32, o_small[r]), want_small[r]), r
            assert O.equal_bits(O.FP32, to_host(O.FP32, o_big[r]), want_big[r]), r
            assert O.equal_bits(O.FP32, to_host(O.FP32, o_rs[r]), want_rs[r]), r
            assert torch.equal(o_sc[r], sc_src[r * sc_count:(r + 1) * sc_count]), r
        assert comms[0].ipc_status() & 1 == 0
    finally:
        destroy(comms)


def test_graph_replay_in_rank_mode():
    """HcclBarrier and the marker copy captured once by two processes sharing the GPU (a loopback world cannot be
    captured), replayed with the rotating delay outside the graph: the epoch lives on the device, so each replay takes
    the next one. The marker array is rank 0's, mapped by both. Events of different processes cannot be compared, so
    the order assertion across ranks uses the host clock around them: the delayed rank's sleep starts after it read
    the clock (start) and lasts delay_s by its own events, its barrier kernel starts after that, and no rank's stream
    may complete earlier (1 ms granted for the event timer's granularity)."""
    n = 2
    res = spawn(n, "graph")
    for i in range(REPLAYS):
        delayed = i % n
        d = res[delayed]["replays"][i]
        assert d["delay_s"] > 0.005, d  # the delay was there
        for r in range(n):
            rep = res[r]["replays"][i]
            assert rep["seen"] == [i] * n, (i, r, rep)
            assert rep["own_order_ms"] >= 0
            assert rep["done"] >= d["start"] + d["delay_s"] - 1e-3, (i, r, rep, d)
            assert rep["algo"] == IPC
    assert all(res[r]["status"] & 1 == 0 for r in range(n))


@pytest.mark.parametrize("algo", [NHR, MESH], ids=["nhr", "mesh"])
@pytest.mark.parametrize("n", [2, 4, 5])
def test_forced_schedule_in_a_loopback_world(n, algo, cycles):
    """The token schedules on the transport: the staggered check, the compiled-schedule cache on the later calls, and no
    executor staging (the tokens are 256 bytes of the communicator's own)."""
    comms = H.loopback_world(n)
    try:
        for c in comms:
            c.set_algo(algo)
        staggered(comms, cycles)
        for c in comms:
            hits, misses = c.compile_stats()
            assert hits >= 1 and misses == 1, (hits, misses)
            assert c.last_algo == algo
            assert c.scratch() == (0, 0)
            assert c.device_bytes() == 256
    finally:
        destroy(comms)


def _selfloop_worker(q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        import torch as T
        import hccl_amd as HH
        T.cuda.set_device(0)
        comm = HH.comm_init_selfloop(8, 3)
        stream = T.cuda.Stream()
        out = []
        for _ in range(2):  # eager, then captured and replayed from the executor's graph cache
            comm.barrier(stream)
            stream.synchronize()
            out.append((comm.last_algo, comm.graph_stats(), comm.compile_stats()))
        out.append((comm.scratch(), comm.device_bytes()))
        comm.destroy()
        q.put(("ok", out))
    except Exception as e:  # noqa: BLE001
        q.put(("err", f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))


def test_self_loop_stand_in():
    """Rank 3 of 8 over the one-rank RCCL stand-in: the one-sided path is unavailable there, so AUTO runs the NHR
    schedule (3 groups of one send and one receive of equal size, which the stand-in pairs), eagerly the first time and
    as one graph launch the second."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_selfloop_worker, args=(q,))
    p.start()
    try:
        status, out = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert status == "ok", out
    (algo1, graphs1, _), (algo2, graphs2, compiled2), (scratch, held) = out
    assert algo1 == algo2 == NHR
    assert graphs1 == (0, 0) and graphs2 == (1, 1), (graphs1, graphs2)
    assert compiled2 == (1, 1)
    assert scratch == (0, 0) and held == 256


def test_one_rank_enqueues_nothing():
    """A one-rank communicator returns HCCL_SUCCESS and the stream has nothing new to wait for. Shown by a capture around
    the call, which records an empty graph: the call put no node on the stream. (An event recorded on a drained stream
    cannot be asked for completion "at once" on this runtime: the record is itself a stream command, and query() right
    behind it reports not-ready for some microseconds with or without a barrier call before it; measured on the MI355X,
    the first such query failed. So the event is only required to complete, and the stream to be idle after it.)"""
    import ctypes

    comms = H.loopback_world(1)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            torch.zeros(1, device="cuda").fill_(1)  # the stream has run something, and drained
        s.synchronize()
        comms[0].barrier(s)
        done = torch.cuda.Event()
        done.record(s)
        done.synchronize()
        assert done.query() and s.query()
        assert comms[0].last_algo == AUTO
        hip = ctypes.CDLL("libamdhip64.so")
        handle, graph, nodes = ctypes.c_void_p(s.cuda_stream), ctypes.c_void_p(), ctypes.c_size_t(99)
        assert hip.hipStreamBeginCapture(handle, 1) == 0  # hipStreamCaptureModeThreadLocal
        try:
            comms[0].barrier(s)
        finally:
            assert hip.hipStreamEndCapture(handle, ctypes.byref(graph)) == 0
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0
        assert nodes.value == 0
        assert hip.hipGraphDestroy(graph) == 0
        assert comms[0].device_bytes() == 0
    finally:
        destroy(comms)
