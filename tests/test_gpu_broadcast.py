"""HcclBroadcast on the GPU: the one-sided kernel (k_ipc_bcast, both kinds) and the mesh two-shot schedule, in loopback
worlds (n ranks in one process on the one GPU) and in rank mode (two processes sharing the GPU).

The operator moves data only, so every comparison is on raw bytes: the inputs are random bytes (NaN payloads included),
every rank's buffer must equal the root's, the root's must be unchanged, and the 64 guard bytes of 0xA5 on each side of
every buffer must be untouched.
"""
import datetime
import multiprocessing as mp
import os
import random
import socket
import threading
import time
import traceback

import pytest
import torch

import hccl_amd as H

pytestmark = pytest.mark.gpu

IPC, SCHED, AUTO = int(H.Algo.IPC), int(H.Algo.MESH_TWOSHOT), int(H.Algo.AUTO)
BY_BOUND, TWO_SHOT, ONE_SHOT = 0, 1, 2
GUARD = 64
SMALL_IPC = 1 << 20    # the small-call rule's bound in these worlds (the suite's environment turns the rule off)
ONE_SHOT_MAX = 64 << 20  # kIpcBcastOneShotMaxBytes (ipc_plan.h)
DTYPES = [torch.int8, torch.uint8, torch.float8_e4m3fn, torch.float16, torch.uint32, torch.float64]


def _esize(dt):
    return torch.empty(0, dtype=dt).element_size()


@pytest.fixture(scope="module")
def worlds():
    cache = {}
    mp_ = pytest.MonkeyPatch()
    mp_.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")  # a stuck barrier fails the test, never hangs the box

    def get(n):
        if n not in cache:
            cache[n] = H.loopback_world(n)
            for c in cache[n]:
                c.set_config(H.Config.SMALL_IPC_BYTES, SMALL_IPC)
        return cache[n]

    yield get
    torch.cuda.synchronize()
    for comms in cache.values():
        for c in comms:
            c.destroy()
    mp_.undo()


def run_ranks(n, fn):
    errs = []

    def body(r):
        try:
            fn(r)
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))

    th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs


def guarded(nbytes, shift_bytes, seed):
    """(whole allocation, the buffer's byte view): random bytes between two guards of 0xA5."""
    whole = torch.full((GUARD + shift_bytes + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    view = whole[GUARD + shift_bytes:GUARD + shift_bytes + nbytes]
    view.copy_(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g))
    return whole, view


def broadcast_and_check(comms, root, count, dt, algo, kind=BY_BOUND, shift=0, seed=0, want_algo=None):
    n, es = len(comms), _esize(dt)
    nbytes, sb = count * es, shift * es
    made = [guarded(nbytes, sb, seed * 64 + r) for r in range(n)]
    bufs = [v.view(dt) for _, v in made]
    want = made[root][1].clone()
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(algo)
        c.set_broadcast_kind(kind)
    torch.cuda.synchronize()
    run_ranks(n, lambda r: comms[r].broadcast(bufs[r], root, streams[r]))
    torch.cuda.synchronize()
    used = comms[0].last_algo
    for c in comms:
        c.set_algo(AUTO)
        c.set_broadcast_kind(BY_BOUND)
    what = (n, root, count, dt, algo, kind, shift)
    for r in range(n):
        whole, view = made[r]
        assert torch.equal(view, want), (what, r)
        assert bool((whole[:GUARD + sb] == 0xA5).all()) and bool((whole[GUARD + sb + nbytes:] == 0xA5).all()), (what, r)
    if want_algo is not None:
        assert used == want_algo, (what, used)
    return used


@pytest.mark.parametrize("path", [IPC, SCHED, AUTO], ids=["ipc", "schedule", "auto"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_broadcast_delivers_the_roots_bytes(worlds, n, path):
    """Roots first / middle / last, every element size, ragged counts, a count whose ceil(count / n) chunks end off
    the 16-byte grid, and the two counts around the one-shot bound; under AUTO also a call above the small-call bound,
    which takes the schedule."""
    comms = worlds(n)
    seed = 0
    for root in sorted({0, n // 2, n - 1}):
        for dt in DTYPES:
            es = _esize(dt)
            counts = [1, max(1, n - 1), n + 1, 1000, 4099, ONE_SHOT_MAX // es, ONE_SHOT_MAX // es + 1]
            if path == AUTO and dt == torch.uint8:
                counts.append(SMALL_IPC + 3)
            for count in counts:
                seed += 1
                want = SCHED if path == SCHED or (path == AUTO and count * es > SMALL_IPC) else IPC
                broadcast_and_check(comms, root, count, dt, path, seed=seed, want_algo=want)
    assert comms[0].ipc_status() & 1 == 0


@pytest.mark.parametrize("kind", [TWO_SHOT, ONE_SHOT], ids=["two_shot", "one_shot"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_buffers(worlds, kind, shift):
    """A buffer that starts 1, 2 or 3 elements of a 2-byte type off the 16-byte grid takes the element-wise path."""
    for n in (2, 3, 8):  # 8: the element-wise copy beside the pushes to six result areas
        for count in (7, 5001, 70001):
            broadcast_and_check(worlds(n), n - 1, count, torch.float16, IPC, kind, shift, seed=shift, want_algo=IPC)


def test_multi_round(monkeypatch):
    """The large staging tier at its smallest size (1 MiB areas): 3.5 MiB on 3 ranks needs 4 rounds of either kind."""
    monkeypatch.setenv("HCCL_AMD_IPC_STAGING_MIB", "1")
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    comms = H.loopback_world(3)
    try:
        for dt, count in ((torch.uint8, (7 << 19) + 5), (torch.float64, (7 << 16) + 3)):
            for kind in (TWO_SHOT, ONE_SHOT):  # the two-shot, then the one-shot forced on the same data
                broadcast_and_check(comms, 1, count, dt, IPC, kind, seed=77, want_algo=IPC)
        assert comms[0].ipc_status() & 1 == 0
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


def test_back_to_back_with_other_kinds(worlds):
    """AllReduce two-shot -> Broadcast -> Reduce -> Broadcast (another root) -> AllGather, 20 times on one world with no
    host synchronisation in between: the two-barrier kinds share their staging from call to call with no barrier in
    between (the invariant of ipc_k_bcast.hip, on hardware). Integer data, checked at the end."""
    n, iters, count = 4, 20, 300001
    comms = worlds(n)
    S = H.HcclReduceOp.SUM
    dev = "cuda"
    ramp = torch.arange(count, dtype=torch.int32, device=dev) % 1009
    ar_in = [[ramp + (r + 1 + i) for i in range(iters)] for r in range(n)]
    ar_out = [[torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(iters)] for _ in range(n)]
    b1 = [[ramp * (r + 2) + i for i in range(iters)] for r in range(n)]
    red_out = [[torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(iters)] for _ in range(n)]
    b2 = [[ramp * (r + 3) - i for i in range(iters)] for r in range(n)]
    ag_out = [[torch.zeros(n * 5003, dtype=torch.int32, device=dev) for _ in range(iters)] for _ in range(n)]
    want_b1 = [b1[i % n][i].clone() for i in range(iters)]
    want_b2 = [b2[(i + 1) % n][i].clone() for i in range(iters)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(int(H.Algo.IPC_TWOSHOT))
        c.set_broadcast_kind(TWO_SHOT)
    torch.cuda.synchronize()

    def body(r):
        c, s = comms[r], streams[r]
        for i in range(iters):
            c.all_reduce(ar_in[r][i], ar_out[r][i], S, s)
            c.broadcast(b1[r][i], i % n, s)
            c.reduce(ar_in[r][i], red_out[r][i], (i + 2) % n, S, s)
            c.broadcast(b2[r][i], (i + 1) % n, s)
            c.all_gather(ar_in[r][i][:5003], ag_out[r][i], s)

    run_ranks(n, body)
    torch.cuda.synchronize()
    for c in comms:
        c.set_algo(AUTO)
        c.set_broadcast_kind(BY_BOUND)
    assert comms[0].ipc_status() & 1 == 0
    for i in range(iters):
        total = ramp * n + sum(q + 1 + i for q in range(n))
        gathered = torch.cat([ar_in[q][i][:5003] for q in range(n)])
        for r in range(n):
            assert torch.equal(ar_out[r][i], total), (i, r)
            assert torch.equal(b1[r][i], want_b1[i]), (i, r)
            assert torch.equal(b2[r][i], want_b2[i]), (i, r)
            assert torch.equal(ag_out[r][i], gathered), (i, r)
        assert torch.equal(red_out[(i + 2) % n][i], total), i


def test_random_draws(worlds):
    rng = random.Random(20240611)
    for draw in range(200):
        n = rng.choice((2, 3, 8))
        dt = rng.choice(DTYPES)
        path, kind = rng.choice(((IPC, BY_BOUND), (IPC, TWO_SHOT), (IPC, ONE_SHOT), (SCHED, BY_BOUND)))
        count = rng.choice((rng.randint(1, 300), rng.randint(1, 20000), rng.randint(1, 300000)))
        broadcast_and_check(worlds(n), rng.randrange(n), count, dt, path, kind, shift=rng.randrange(4), seed=1000 + draw,
                            want_algo=path)


# ------------------------------------------------------------------------------------------------ rank mode

RANK_CASES = [  # (dtype name, count, kind, shift)
    ("uint8", 1, BY_BOUND, 0), ("uint8", 4099, ONE_SHOT, 3), ("float16", 70001, TWO_SHOT, 1),
    ("float64", 300001, TWO_SHOT, 0), ("uint32", 300001, ONE_SHOT, 0), ("float16", 33333, BY_BOUND, 0),
    ("uint8", (36 << 20) + 11, TWO_SHOT, 0),
]
RANK_ROOT = 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, n, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"
    try:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)

        def all_gather(b):
            out = [None] * n
            dist.all_gather_object(out, b)
            return out

        comm = H.comm_init_host_exchange(n, rank, all_gather)
        comm.set_algo(IPC)
        stream = torch.cuda.Stream()
        results = []
        for i, (name, count, kind, shift) in enumerate(RANK_CASES):
            dt = getattr(torch, name)
            es = _esize(dt)
            # every rank builds every rank's bytes from the seeds, so each knows the root's
            made = [guarded(count * es, shift * es, 7000 + i * 8 + r) for r in range(n)]
            whole, view = made[rank]
            want = made[RANK_ROOT][1]
            comm.set_broadcast_kind(kind)
            torch.cuda.synchronize()
            comm.broadcast(view.view(dt), RANK_ROOT, stream)
            stream.synchronize()
            lo = GUARD + shift * es
            ok = bool(torch.equal(view, want)) and bool((whole[:lo] == 0xA5).all()) and \
                bool((whole[lo + count * es:] == 0xA5).all())
            results.append((i, ok, comm.last_algo, comm.ipc_status() & 1))
            del made, whole, view, want
        # HIP graph: both kinds captured once (1000 B one-shot, 300001 fp32 two-shot), replayed three times with the
        # root's data changed in between; the barrier epochs live on the device, so each replay takes new ones
        small = torch.zeros(1000, dtype=torch.uint8, device="cuda")
        large = torch.zeros(300001, dtype=torch.float32, device="cuda")
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            comm.set_broadcast_kind(ONE_SHOT)
            comm.broadcast(small, RANK_ROOT, cs)
            comm.set_broadcast_kind(TWO_SHOT)
            comm.broadcast(large, RANK_ROOT, cs)
        graph_ok = []
        for rep in range(3):
            small.fill_(rank * 50 + rep)
            large.fill_(float(rank * 1000 + rep))
            torch.cuda.synchronize()
            dist.barrier()
            graph.replay()
            torch.cuda.synchronize()
            graph_ok.append(bool((small == RANK_ROOT * 50 + rep).all()) and
                            bool((large == float(RANK_ROOT * 1000 + rep)).all()))
            dist.barrier()
        results.append(("graph", graph_ok, comm.ipc_status() & 1))
        dist.barrier()
        comm.destroy()
        dist.destroy_process_group()
        q.put((rank, "ok", results))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)  # peers' kernels are bounded: let them drain before this process's memory goes away


def test_rank_mode_and_graph_replay():
    """Two processes sharing the GPU, root 1, both kinds, unaligned buffers and a 36 MiB call; then both kinds
    captured into a HIP graph and replayed with new data."""
    n = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, n, port, q)) for r in range(n)]
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
    for r in range(n):
        assert got[r][0] == "ok", f"rank {r}:\n{got[r][0]}"
    for r in range(n):
        res = got[r][1]
        assert res[-1] == ("graph", [True] * 3, 0), (r, res[-1])
        assert res[:-1] == [(i, True, IPC, 0) for i in range(len(RANK_CASES))], (r, res)
