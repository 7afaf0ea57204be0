"""HcclAlltoAll, HcclAlltoAllV and HcclAlltoAllVC on the GPU: the one-sided kernel (k_ipc_a2a) and the mesh schedule, in
loopback worlds (n ranks in one process on the one GPU) and in rank mode (two processes sharing the GPU).

The operators move data only, so every comparison is on raw bytes: the inputs are random bytes (NaN payloads included),
the receive buffer starts as random bytes too and must end as those bytes with every pair's region replaced by the
sender's block (so the gaps between regions are untouched), the send buffer must be unchanged, and the 64 guard bytes of
0xA5 on each side of both buffers must be untouched.
"""
import datetime
import multiprocessing as mp
import os
import socket
import threading
import time
import traceback

import pytest
import torch

import hccl_amd as H

pytestmark = pytest.mark.gpu

IPC, SCHED, AUTO = int(H.Algo.IPC), int(H.Algo.MESH_ONESHOT), int(H.Algo.AUTO)
GUARD = 64
SMALL_IPC = 1 << 20  # the small-call rule's bound in these worlds (the suite's environment turns the rule off)
A2A = int(H.OpType.ALLTOALL)
DTYPES = [torch.uint8, torch.float16, torch.uint32, torch.float64]


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
    if nbytes:
        view.copy_(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g))
    return whole, view


def packed(matrix):
    """Per rank (send counts, sdispls, recv counts, rdispls) as HcclAlltoAllVC lays them out."""
    n = len(matrix)
    lay = []
    for r in range(n):
        sc = [matrix[r][q] for q in range(n)]
        rc = [matrix[q][r] for q in range(n)]
        lay.append((sc, [sum(sc[:q]) for q in range(n)], rc, [sum(rc[:q]) for q in range(n)]))
    return lay


def gapped(matrix, off):
    """The same counts with gaps between the blocks: block q starts `off + q` elements after block q - 1 ends, so with
    2-byte elements and off = 1, 2, 3 the blocks start 1, 2, 3, ... elements off the 16-byte grid."""
    lay = []
    for sc, sd, rc, rd in packed(matrix):
        n = len(sc)
        shift = [(q + 1) * off + q * (q - 1) // 2 for q in range(n)]
        lay.append((sc, [sd[q] + shift[q] for q in range(n)], rc, [rd[q] + shift[q] + 1 for q in range(n)]))
    return lay


class Case:
    """One call's buffers on every rank and the bytes each receive buffer must end with."""

    def __init__(self, lay, dt, seed, ranks=None):
        self.lay, self.dt, self.es, self.n = lay, dt, _esize(dt), len(lay)
        es, n = self.es, self.n
        self.send, self.recv, self.keep, self.want = {}, {}, {}, {}
        made = {}
        for r in range(n):  # every rank's send bytes come from the seeds, so a process can build its peers' too
            sc, sd, _, _ = lay[r]
            made[r] = guarded(max(sd[q] + sc[q] for q in range(n)) * es, 0, seed * 64 + r)
        for r in (range(n) if ranks is None else ranks):
            _, _, rc, rd = lay[r]
            self.send[r] = made[r]
            self.keep[r] = made[r][0].clone()
            self.recv[r] = guarded(max(rd[q] + rc[q] for q in range(n)) * es, 0, seed * 64 + 32 + r)
            want = self.recv[r][0].clone()
            for q in range(n):
                sq = lay[q][1][r] * es
                lo = GUARD + rd[q] * es
                want[lo:lo + rc[q] * es] = made[q][1][sq:sq + rc[q] * es]
            self.want[r] = want

    def bufs(self, r):
        return self.send[r][1].view(self.dt), self.recv[r][1].view(self.dt)

    def check(self, what, ranks=None):
        for r in (range(self.n) if ranks is None else ranks):
            assert torch.equal(self.recv[r][0], self.want[r]), (what, r)    # regions, gaps and guards
            assert torch.equal(self.send[r][0], self.keep[r]), (what, r)    # sendBuf and its guards unchanged


def call(comm, case, r, form, matrix, stream):
    send, recv = case.bufs(r)
    if form == "a2a":
        comm.alltoall(send, recv, stream)
    elif form == "vc":
        comm.alltoall_vc(send, matrix, recv, stream, dtype=H.hccl_dtype(send))
    else:
        comm.alltoall_v(send, case.lay[r][0], case.lay[r][1], recv, case.lay[r][2], case.lay[r][3], stream,
                        dtype=H.hccl_dtype(send))


def run_and_check(comms, matrix, dt, algo, form, seed, off=0):
    n = len(comms)
    case = Case(gapped(matrix, off) if off else packed(matrix), dt, seed)
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(algo)
    torch.cuda.synchronize()
    run_ranks(n, lambda r: call(comms[r], case, r, form, matrix, streams[r]))
    torch.cuda.synchronize()
    used = comms[0].last_algo
    for c in comms:
        c.set_algo(AUTO)
    what = (n, form, str(dt), algo, off, seed)
    case.check(what)
    # last_algo: the one-sided path reports IPC, the schedule path MESH_ONESHOT. Under AUTO an AlltoAllV takes the
    # kernel whatever its size; the forms whose matrix every rank knows take it up to the small-call bound.
    largest = max(max(row) for row in matrix)
    one_sided = algo == IPC or (algo == AUTO and (form == "v" or n * largest * case.es <= SMALL_IPC))
    assert used == (IPC if one_sided else SCHED), (what, used)


def matrices(n):
    g = torch.Generator().manual_seed(100 + n)
    rnd = [[int(torch.randint(0, 6, (1,), generator=g)) * 37 % 151 for _ in range(n)] for _ in range(n)]
    rnd[n - 1][0] = 0
    zrow = [[0 if p == n // 2 else 3 + p + q for q in range(n)] for p in range(n)]
    zcol = [[0 if q == n - 1 else 2 + p * q for q in range(n)] for p in range(n)]
    zero = [[0] * n for _ in range(n)]
    skew = [[1] * n for _ in range(n)]
    skew[0][n - 1] = 70001  # the ranks' own round needs differ
    return {"random": rnd, "zero_row": zrow, "zero_col": zcol, "all_zero": zero, "skew": skew}


@pytest.mark.parametrize("path", [IPC, SCHED, AUTO], ids=["ipc", "schedule", "auto"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_alltoall(worlds, n, path):
    """Element sizes 1, 2, 4, 8 and per-pair counts 1, n + 1, 1000, 4099; under AUTO also one count just above the
    small-call bound, which takes the schedule."""
    comms = worlds(n)
    seed = 0
    for dt in DTYPES:
        counts = [1, n + 1, 1000, 4099]
        if path == AUTO and dt == torch.uint8:
            counts.append(SMALL_IPC // n + 1)
        for count in counts:
            seed += 1
            run_and_check(comms, [[count] * n for _ in range(n)], dt, path, "a2a", seed)
    assert comms[0].ipc_status() & 1 == 0


@pytest.mark.parametrize("path", [IPC, SCHED, AUTO], ids=["ipc", "schedule", "auto"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_alltoall_v_and_vc(worlds, n, path):
    """Random counts with zeros, a zero row, a zero column, all zero, and one pair of 70001 beside pairs of 1; the V form
    also with displacements that leave gaps and start 1, 2 or 3 two-byte elements off the 16-byte grid."""
    comms = worlds(n)
    seed = 100
    for name, m in matrices(n).items():
        for form in ("v", "vc"):
            seed += 1
            run_and_check(comms, m, torch.float16, path, form, seed)
        if name in ("random", "skew"):
            for off in (1, 2, 3):
                seed += 1
                run_and_check(comms, m, torch.float16, path, "v", seed, off=off)
    run_and_check(comms, matrices(n)["random"], torch.float64, path, "v", seed + 1, off=1)
    run_and_check(comms, matrices(n)["random"], torch.uint8, path, "vc", seed + 2)
    assert comms[0].ipc_status() & 1 == 0


def test_multi_round(monkeypatch):
    """Shrunken staging: the large tier at the smallest size the configuration accepts (16 MiB areas) and the small one
    at its smallest (3 x 64 KiB). AlltoAllV always runs in the small tier: a pair of 70001 8-byte elements takes 9 rounds
    of its 62 KiB slots while the other ranks need one, agreed on the device. AlltoAllVC of that matrix fits one round of
    the large tier; with a pair of 1500001 elements it takes the planner's round count, asserted here."""
    monkeypatch.setenv("HCCL_AMD_IPC_STAGING_MIB", "16")
    monkeypatch.setenv("HCCL_AMD_SMALL_IPC_BYTES", "0")
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    n, big = 3, 1500001
    m = matrices(n)["skew"]
    wide = [[1] * n for _ in range(n)]
    wide[0][n - 1] = big
    res, launches = H.ipc_plan(A2A, n, big, H.HcclDataType.INT64, family=AUTO, sharedDevice=1)
    assert res.altBytes == 16 << 20 and launches[0].piece == (16 << 20) // 8 // n // 2 * 2
    assert launches[0].rounds == -(-big // launches[0].piece) == 3
    res, launches = H.ipc_plan(A2A, n, 0, H.HcclDataType.INT64, family=-1, kind=8, geom=4, subMode=1, sharedDevice=1)
    assert launches[0].rounds == 0 and launches[0].piece == (65536 - 2048) // 8
    assert -(-70001 // launches[0].piece) == 9  # the V form's own need for the skewed matrix
    comms = H.loopback_world(n)
    try:
        for form in ("v", "vc", "v"):
            run_and_check(comms, m, torch.float64, IPC, form, seed=77)
            run_and_check(comms, m, torch.float64, IPC, form, seed=78, off=1 if form == "v" else 0)
        run_and_check(comms, wide, torch.float64, IPC, "vc", seed=79)  # three rounds of the large tier
        assert comms[0].ipc_status() & 1 == 0
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


def test_back_to_back_without_synchronisation(worlds):
    """Three AlltoAllV calls with different matrices on one world, nothing between them: each launch must read its own
    tables, and the alternate areas carry one call's slots while the next call already stores."""
    n = 3
    comms = worlds(n)
    ms = [matrices(n)["skew"], matrices(n)["random"], [[4099 + p - q for q in range(n)] for p in range(n)]]
    cases = [Case(gapped(m, 1), torch.float16, 300 + i) for i, m in enumerate(ms)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(IPC)
    torch.cuda.synchronize()

    def body(r):
        for i in range(3):
            call(comms[r], cases[i], r, "v", ms[i], streams[r])

    run_ranks(n, body)
    torch.cuda.synchronize()
    for c in comms:
        c.set_algo(AUTO)
    for i, case in enumerate(cases):
        case.check(("back_to_back", i))
    assert comms[0].last_algo == IPC and comms[0].ipc_status() & 1 == 0


# ------------------------------------------------------------------------------------------------ rank mode

RANK_MATRIX = [[3, 70001], [1, 5]]  # rank 0 needs several rounds of the shrunken slots, rank 1 one


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, n, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"
    os.environ["HCCL_AMD_IPC_STAGING_MIB"] = "16"
    os.environ["HCCL_AMD_SMALL_IPC_BYTES"] = "0"  # the small tier at its smallest: 64 KiB slots
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
        stream = torch.cuda.Stream()
        results = []
        for i, (dt, off) in enumerate(((torch.float64, 0), (torch.float16, 1), (torch.uint8, 3))):
            case = Case(gapped(RANK_MATRIX, off) if off else packed(RANK_MATRIX), dt, 500 + i, ranks=[rank])
            torch.cuda.synchronize()
            call(comm, case, rank, "v", RANK_MATRIX, stream)
            stream.synchronize()
            try:
                case.check(("rank", i), ranks=[rank])
                ok = True
            except AssertionError:
                ok = False
            results.append((i, ok, comm.last_algo, comm.ipc_status() & 1))
        # HIP graph: an AlltoAllV captured after the warm-up calls above and replayed three times with fresh inputs; the
        # tables travel in the kernel's arguments and the epochs live on the device, so each replay takes new ones
        lay = packed(RANK_MATRIX)
        sc, sd, rc, rd = lay[rank]
        send = torch.zeros(sum(sc), dtype=torch.float64, device="cuda")
        recv = torch.zeros(sum(rc), dtype=torch.float64, device="cuda")
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            comm.alltoall_v(send, sc, sd, recv, rc, rd, torch.cuda.current_stream())
        graph_ok = []
        for rep in range(3):
            for qq in range(n):  # the block for rank qq holds 1000 * me + 10 * qq + rep
                send[sd[qq]:sd[qq] + sc[qq]] = float(1000 * rank + 10 * qq + rep)
            recv.fill_(-1.0)
            torch.cuda.synchronize()
            dist.barrier()
            graph.replay()
            torch.cuda.synchronize()
            graph_ok.append(all(bool((recv[rd[qq]:rd[qq] + rc[qq]] == float(1000 * qq + 10 * rank + rep)).all())
                                for qq in range(n)))
            dist.barrier()
        results.append(("graph", graph_ok, comm.last_algo, comm.ipc_status() & 1))
        dist.barrier()
        comm.destroy()
        dist.destroy_process_group()
        q.put((rank, "ok", results))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)  # peers' kernels are bounded: let them drain before this process's memory goes away


def test_rank_mode_and_graph_replay():
    """Two processes sharing the GPU on an IPC-only communicator: AlltoAllV with unequal round needs (aligned and
    unaligned), then one captured into a HIP graph and replayed with new data."""
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
        assert res[-1] == ("graph", [True] * 3, IPC, 0), (r, res[-1])
        assert res[:-1] == [(i, True, IPC, 0) for i in range(3)], (r, res)
