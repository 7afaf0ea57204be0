"""HcclAllGatherV on the GPU: the one-sided kernel (k_ipc_sg, kind kIpcAllGatherV) and the mesh schedule, in loopback
worlds (n ranks in one process on the one GPU); then HcclScatter and HcclAllGatherV in rank mode (two processes sharing
the GPU), eager and replayed from a HIP graph.

The operator moves data only, so every comparison is on raw bytes: the inputs are random bytes (NaN payloads included),
block q of every rank's output must equal rank q's input, the bytes between and around the blocks must keep their fill,
the inputs must be unchanged, and the 64 guard bytes of 0xA5 on each side of every buffer must be untouched.
"""
import datetime
import multiprocessing as mp
import os
import time
import traceback

import pytest
import torch

import hccl_amd as H
from test_gpu_broadcast import GUARD, _free_port, guarded, run_ranks

pytestmark = pytest.mark.gpu

IPC, SCHED, AUTO = int(H.Algo.IPC), int(H.Algo.MESH_ONESHOT), int(H.Algo.AUTO)
SMALL_IPC = 1 << 20  # the small-call rule's bound in these worlds (the suite's environment turns the rule off)
DTYPES = [torch.uint8, torch.float16, torch.uint32, torch.float64]  # element sizes 1, 2, 4, 8


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


def count_vectors(n):
    ragged = [(1, 4099, 0, 77, 1000, 3, 2048, 5)[q % 8] for q in range(n)]
    return {
        "equal": [1000] * n,
        "ragged": ragged,
        "one_zero": [0 if q == n // 2 else 300 + 7 * q for q in range(n)],
        "only_one": [4099 if q == n - 1 else 0 for q in range(n)],
    }


def layouts(counts):
    n = len(counts)
    packed = [sum(counts[:q]) for q in range(n)]
    gaps = [sum(counts[:q]) + 5 * (q + 1) for q in range(n)]
    desc = [sum(counts[q + 1:]) + 2 * (n - 1 - q) for q in range(n)]
    off = [sum(counts[:q]) + q + 1 for q in range(n)]  # blocks 1, 2, 3, .. elements off the packed places
    return {"packed": packed, "gaps": gaps, "descending": desc, "off_grid": off}


def gather_and_check(comms, counts, displs, dt, algo, shift=0, seed=0, want_algo=None, in_place=False):
    n, es = len(comms), _esize(dt)
    sb = shift * es
    out_bytes = max(displs[q] + counts[q] for q in range(n)) * es + 3 * es
    outs = [guarded(out_bytes, sb, seed * 64 + 32 + r) for r in range(n)]
    ins = [guarded(counts[r] * es, sb, seed * 64 + r) for r in range(n)]
    data = [v.clone() for _, v in ins]
    fills = [v.clone() for _, v in outs]
    sends = []
    for r in range(n):
        lo = displs[r] * es
        if in_place:
            outs[r][1][lo:lo + counts[r] * es] = data[r]
            fills[r][lo:lo + counts[r] * es] = data[r]
            sends.append(outs[r][1][lo:lo + counts[r] * es].view(dt) if counts[r] else None)
        else:
            sends.append(ins[r][1].view(dt) if counts[r] else None)
    recvs = [v.view(dt) for _, v in outs]
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(algo)
    torch.cuda.synchronize()
    run_ranks(n, lambda r: comms[r].all_gather_v(sends[r], recvs[r], counts, displs, streams[r]))
    torch.cuda.synchronize()
    used = comms[0].last_algo
    for c in comms:
        c.set_algo(AUTO)
    what = (n, counts, displs, dt, algo, shift, in_place)
    for r in range(n):
        want = fills[r]
        for q in range(n):
            want[displs[q] * es:(displs[q] + counts[q]) * es] = data[q]
        assert torch.equal(outs[r][1], want), (what, r)
        assert torch.equal(ins[r][1], data[r]), (what, r)
        for whole, nbytes in ((outs[r][0], out_bytes), (ins[r][0], counts[r] * es)):
            lo = GUARD + sb
            assert bool((whole[:lo] == 0xA5).all()) and bool((whole[lo + nbytes:] == 0xA5).all()), (what, r)
    if want_algo is not None:
        assert used == want_algo, (what, used)
    return [v for _, v in outs]


@pytest.mark.parametrize("path", [IPC, SCHED, AUTO], ids=["ipc", "schedule", "auto"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_all_gather_v_delivers_every_block(worlds, n, path):
    """Every count vector in every layout, the element sizes in turn; under AUTO also a call whose output lies above the
    small-call bound, which takes the schedule."""
    comms = worlds(n)
    seed = 0
    for name, counts in count_vectors(n).items():
        for lname, displs in layouts(counts).items():
            for dt in DTYPES if lname in ("packed", "off_grid") else DTYPES[1:3]:
                seed += 1
                gather_and_check(comms, counts, displs, dt, path, seed=seed, want_algo=IPC if path == AUTO else path)
    if path == AUTO:
        counts = [SMALL_IPC // n + 5] * n
        gather_and_check(comms, counts, layouts(counts)["packed"], torch.uint8, path, seed=999, want_algo=SCHED)
    assert comms[0].ipc_status() & 1 == 0


@pytest.mark.parametrize("path", [IPC, SCHED], ids=["ipc", "schedule"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_buffers(worlds, path, shift):
    for n in (2, 3, 8):
        counts = count_vectors(n)["ragged"]
        for lname in ("packed", "off_grid"):
            gather_and_check(worlds(n), counts, layouts(counts)[lname], torch.float16, path, shift, seed=shift,
                             want_algo=path)


@pytest.mark.parametrize("path", [IPC, SCHED], ids=["ipc", "schedule"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_in_place(worlds, n, path):
    """sendBuf == recvBuf + recvDispls[rank]: the own block is where it belongs and is not copied."""
    seed = 300
    for name, counts in count_vectors(n).items():
        for lname in ("packed", "gaps"):
            seed += 1
            gather_and_check(worlds(n), counts, layouts(counts)[lname], torch.uint32, path, seed=seed, want_algo=path,
                             in_place=True)


@pytest.mark.parametrize("path", [IPC, SCHED], ids=["ipc", "schedule"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_equal_counts_match_all_gather(worlds, n, path):
    comms = worlds(n)
    for dt, count in ((torch.uint8, 4099), (torch.float16, 1000), (torch.float64, 333)):
        counts = [count] * n
        got = gather_and_check(comms, counts, layouts(counts)["packed"], dt, path, seed=42, want_algo=path)
        es = _esize(dt)
        # the same inputs (the same seeds) through HcclAllGather
        ins = [guarded(count * es, 0, 42 * 64 + r)[1].view(dt) for r in range(n)]
        outs = [torch.zeros(n * count * es + 3 * es, dtype=torch.uint8, device="cuda") for _ in range(n)]
        streams = [torch.cuda.Stream() for _ in range(n)]
        for c in comms:
            c.set_algo(IPC if path == IPC else SCHED)
        torch.cuda.synchronize()
        run_ranks(n, lambda r: comms[r].all_gather(ins[r], outs[r][:n * count * es].view(dt), streams[r]))
        torch.cuda.synchronize()
        for c in comms:
            c.set_algo(AUTO)
        for r in range(n):
            assert torch.equal(got[r][:n * count * es], outs[r][:n * count * es]), (n, dt, r)


def test_multi_round(monkeypatch):
    """The large staging tier at its smallest accepted size (16 MiB areas, so 8 MiB slots on two ranks): a block of
    17 MiB beside a short one needs 3 rounds, asserted from the planner before anything runs."""
    monkeypatch.setenv("HCCL_AMD_IPC_STAGING_MIB", "16")
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    n = 2
    counts = [(17 << 20) + 3, 4099]
    displs = [7, (17 << 20) + 64]
    res, launches = H.ipc_plan(H.OpType.ALLGATHER_V, n, counts[0], H.HcclDataType.UINT8, family=0, counts=counts,
                               displs=displs, sharedDevice=1)
    assert res.altBytes == 16 << 20 and len(launches) == 1 and launches[0].rounds >= 3, (res.altBytes, launches[0].rounds)
    comms = H.loopback_world(n)
    try:
        gather_and_check(comms, counts, displs, torch.uint8, IPC, seed=77, want_algo=IPC)
        assert comms[0].ipc_status() & 1 == 0
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


# ------------------------------------------------------------------------------------------------ rank mode

RANK_SCATTER = [  # (dtype name, count, root, shift)
    ("uint8", 1, 0, 0), ("uint8", 4099, 1, 3), ("float16", 70001, 1, 1), ("float64", 300001, 0, 0),
]
RANK_GATHER = [  # (dtype name, counts, displs, shift)
    ("uint8", [1, 4099], [0, 1], 0), ("float16", [70001, 0], [5, 0], 1), ("float64", [1000, 300001], [300003, 1], 0),
]


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
        for i, (name, count, root, shift) in enumerate(RANK_SCATTER):
            dt = getattr(torch, name)
            es = _esize(dt)
            # every rank builds the root's bytes from the seed, so each knows its block
            _, src = guarded(n * count * es, shift * es, 9000 + i)
            whole, view = guarded(count * es, shift * es, 9100 + i * 8 + rank)
            torch.cuda.synchronize()
            comm.scatter(src.view(dt) if rank == root else None, view.view(dt), root, stream)
            stream.synchronize()
            lo = GUARD + shift * es
            ok = bool(torch.equal(view, src[rank * count * es:(rank + 1) * count * es])) and \
                bool((whole[:lo] == 0xA5).all()) and bool((whole[lo + count * es:] == 0xA5).all())
            results.append(("scatter", i, ok, comm.last_algo, comm.ipc_status() & 1))
        for i, (name, counts, displs, shift) in enumerate(RANK_GATHER):
            dt = getattr(torch, name)
            es = _esize(dt)
            ins = [guarded(counts[r] * es, shift * es, 9500 + i * 8 + r)[1] for r in range(n)]
            nbytes = (max(displs[r] + counts[r] for r in range(n)) + 2) * es
            whole, view = guarded(nbytes, shift * es, 9600 + i * 8 + rank)
            want = view.clone()
            for r in range(n):
                want[displs[r] * es:(displs[r] + counts[r]) * es] = ins[r]
            torch.cuda.synchronize()
            comm.all_gather_v(ins[rank].view(dt) if counts[rank] else None, view.view(dt), counts, displs, stream)
            stream.synchronize()
            lo = GUARD + shift * es
            ok = bool(torch.equal(view, want)) and bool((whole[:lo] == 0xA5).all()) and \
                bool((whole[lo + nbytes:] == 0xA5).all())
            results.append(("gather", i, ok, comm.last_algo, comm.ipc_status() & 1))
        # HIP graph: both operators captured once and replayed four times with fresh inputs; the barrier epochs live on
        # the device, so each replay takes new ones
        sc_src = torch.zeros(n * 5001, dtype=torch.float32, device="cuda")
        sc_dst = torch.zeros(5001, dtype=torch.float32, device="cuda")
        counts, displs = [3001, 777], [2, 3010]
        gv_src = torch.zeros(counts[rank], dtype=torch.int32, device="cuda")
        gv_dst = torch.zeros(3800, dtype=torch.int32, device="cuda")
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            comm.scatter(sc_src if rank == 1 else None, sc_dst, 1, cs)
            comm.all_gather_v(gv_src, gv_dst, counts, displs, cs)
        graph_ok = []
        ramp = torch.arange(n * 5001, dtype=torch.float32, device="cuda")
        for rep in range(4):
            sc_src.copy_(ramp * (rep + 2))
            sc_dst.fill_(-1.0)
            gv_src.fill_(rank * 100 + rep)
            gv_dst.fill_(-1)
            torch.cuda.synchronize()
            dist.barrier()
            graph.replay()
            torch.cuda.synchronize()
            want = torch.full((3800,), -1, dtype=torch.int32, device="cuda")
            for r in range(n):
                want[displs[r]:displs[r] + counts[r]] = r * 100 + rep
            graph_ok.append(bool(torch.equal(sc_dst, ramp[rank * 5001:(rank + 1) * 5001] * (rep + 2))) and
                            bool(torch.equal(gv_dst, want)))
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
    """Two processes sharing the GPU: both operators eager (roots 0 and 1, unaligned buffers, a zero count), then both
    captured into one HIP graph and replayed four times with fresh inputs."""
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
        assert res[-1] == ("graph", [True] * 4, 0), (r, res[-1])
        want = [("scatter", i, True, IPC, 0) for i in range(len(RANK_SCATTER))] + \
               [("gather", i, True, IPC, 0) for i in range(len(RANK_GATHER))]
        assert res[:-1] == want, (r, res)
