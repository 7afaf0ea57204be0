"""HcclScatter on the GPU: the one-sided kernel (k_ipc_sg, kind kIpcScatter) and the mesh schedule, in loopback worlds
(n ranks in one process on the one GPU).

The operator moves data only, so every comparison is on raw bytes: the root's input is random bytes (NaN payloads
included), rank r's output must equal block r of it, the root's input must be unchanged (except in place), and the 64
guard bytes of 0xA5 on each side of every buffer must be untouched. Ranks other than the root pass no input at all.
Rank mode and graph replay of both new operators are in test_gpu_all_gather_v.py.
"""
import pytest
import torch

import hccl_amd as H
from test_gpu_broadcast import GUARD, guarded, run_ranks

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


def untouched(whole, lo, nbytes):
    return bool((whole[:lo] == 0xA5).all()) and bool((whole[lo + nbytes:] == 0xA5).all())


def scatter_and_check(comms, root, count, dt, algo, shift=0, seed=0, want_algo=None, in_place=False):
    n, es = len(comms), _esize(dt)
    blk, sb = count * es, shift * es
    swhole, sview = guarded(n * blk, sb, seed * 64 + 63)
    before = sview.clone()
    made = [guarded(blk, sb, seed * 64 + r) for r in range(n)]
    recvs = [v.view(dt) for _, v in made]
    if in_place:
        recvs[root] = sview[:blk].view(dt)
    sends = [sview.view(dt) if r == root else None for r in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(algo)
    torch.cuda.synchronize()
    run_ranks(n, lambda r: comms[r].scatter(sends[r], recvs[r], root, streams[r]))
    torch.cuda.synchronize()
    used = comms[0].last_algo
    for c in comms:
        c.set_algo(AUTO)
    what = (n, root, count, dt, algo, shift, in_place)
    for r in range(n):
        assert torch.equal(recvs[r].view(torch.uint8), before[r * blk:(r + 1) * blk]), (what, r)
        assert untouched(made[r][0], GUARD + sb, blk), (what, r)
    assert untouched(swhole, GUARD + sb, n * blk), what
    if in_place:
        assert torch.equal(sview[blk:], before[blk:]), what
    else:
        assert torch.equal(sview, before), what
    if want_algo is not None:
        assert used == want_algo, (what, used)
    return used


@pytest.mark.parametrize("path", [IPC, SCHED, AUTO], ids=["ipc", "schedule", "auto"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_scatter_delivers_the_roots_blocks(worlds, n, path):
    """Roots first / middle / last, element sizes 1, 2, 4, 8, counts 1, n + 1, 1000, 4099; under AUTO also a call whose
    n x count x es lies above the small-call bound, which takes the schedule."""
    comms = worlds(n)
    seed = 0
    for root in sorted({0, n // 2, n - 1}):
        for dt in DTYPES:
            es = _esize(dt)
            counts = [1, n + 1, 1000, 4099]
            if path == AUTO and dt == torch.uint8:
                counts.append(SMALL_IPC // n + 3)
            for count in counts:
                seed += 1
                want = SCHED if path == SCHED or (path == AUTO and n * count * es > SMALL_IPC) else IPC
                scatter_and_check(comms, root, count, dt, path, seed=seed, want_algo=want)
    assert comms[0].ipc_status() & 1 == 0


@pytest.mark.parametrize("path", [IPC, SCHED], ids=["ipc", "schedule"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_buffers(worlds, path, shift):
    """Buffers that start 1, 2 or 3 elements of a 2-byte type off the 16-byte grid; with an odd count the blocks of the
    root's input start anywhere."""
    for n in (2, 3, 8):
        for count in (7, 5001, 70001):
            scatter_and_check(worlds(n), n - 1, count, torch.float16, path, shift, seed=shift, want_algo=path)


@pytest.mark.parametrize("path", [IPC, SCHED], ids=["ipc", "schedule"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_in_place_on_the_root(worlds, n, path):
    """recvBuf == sendBuf on root 0 (nothing to copy) and on root n - 1 (block n - 1 lands where block 0 was, after
    block 0 has left)."""
    seed = 500
    for root in (0, n - 1):
        for dt, count in ((torch.uint8, 4099), (torch.float64, 1000), (torch.float16, 300001)):
            seed += 1
            scatter_and_check(worlds(n), root, count, dt, path, seed=seed, want_algo=path, in_place=True)


def test_multi_round(monkeypatch):
    """The large staging tier at its smallest accepted size (16 MiB areas; the Scatter's slot is a whole alternate
    area): blocks of 33 MiB need 3 rounds, asserted from the planner before anything runs."""
    monkeypatch.setenv("HCCL_AMD_IPC_STAGING_MIB", "16")
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    n, count = 2, (33 << 20) + 5
    res, launches = H.ipc_plan(H.OpType.SCATTER, n, count, H.HcclDataType.UINT8, family=0, sharedDevice=1)
    assert res.altBytes == 16 << 20 and len(launches) == 1 and launches[0].rounds >= 3, (res.altBytes, launches[0].rounds)
    comms = H.loopback_world(n)
    try:
        scatter_and_check(comms, 1, count, torch.uint8, IPC, seed=77, want_algo=IPC)
        scatter_and_check(comms, 1, count, torch.uint8, IPC, seed=78, want_algo=IPC, in_place=True)
        assert comms[0].ipc_status() & 1 == 0
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


def test_back_to_back_with_other_kinds(worlds):
    """Scatter -> AllGatherV -> Broadcast (one-shot) -> AlltoAll -> ReduceScatter, 8 times (40 calls) on one stream per
    rank with no host synchronisation in between, roots and counts varying: the single-barrier kinds share the two
    alternate areas from call to call. Integer data, checked at the end."""
    n, iters = 4, 8
    comms = worlds(n)
    dev = "cuda"
    S = H.HcclReduceOp.SUM
    cnt = [1000 + 777 * i for i in range(iters)]
    gv = [[(q * 131 + i * 17) % 5 * 1001 + (0 if (q + i) % 3 == 0 else 1) for q in range(n)] for i in range(iters)]
    gd = [[sum(gv[i][:q]) + 3 * q for q in range(n)] for i in range(iters)]
    ramp = torch.arange(n * 8000, dtype=torch.int32, device=dev)
    sc_in = [[ramp[:n * cnt[i]] * 3 + (r + i) for i in range(iters)] for r in range(n)]
    sc_out = [[torch.zeros(cnt[i], dtype=torch.int32, device=dev) for i in range(iters)] for _ in range(n)]
    gv_in = [[ramp[:gv[i][r]] * 5 + (r * 7 + i) for i in range(iters)] for r in range(n)]
    gv_out = [[torch.full((gd[i][-1] + gv[i][-1] + 2,), -1, dtype=torch.int32, device=dev) for i in range(iters)]
              for _ in range(n)]
    bc = [[ramp[:cnt[i]] * (r + 2) + i for i in range(iters)] for r in range(n)]
    want_bc = [bc[(i + 1) % n][i].clone() for i in range(iters)]
    a2a_in = [[ramp[:n * 301] * 7 + (r * 11 + i) for i in range(iters)] for r in range(n)]
    a2a_out = [[torch.zeros(n * 301, dtype=torch.int32, device=dev) for _ in range(iters)] for _ in range(n)]
    rs_in = [[ramp[:n * 257] % 1009 + (r + i) for i in range(iters)] for r in range(n)]
    rs_out = [[torch.zeros(257, dtype=torch.int32, device=dev) for _ in range(iters)] for _ in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    for c in comms:
        c.set_algo(IPC)
        c.set_broadcast_kind(2)
    torch.cuda.synchronize()

    def body(r):
        c, s = comms[r], streams[r]
        for i in range(iters):
            root = i % n
            c.scatter(sc_in[r][i] if r == root else None, sc_out[r][i], root, s)
            c.all_gather_v(gv_in[r][i] if gv[i][r] else None, gv_out[r][i], gv[i], gd[i], s)
            c.broadcast(bc[r][i], (i + 1) % n, s)
            c.alltoall(a2a_in[r][i], a2a_out[r][i], s)
            c.reduce_scatter(rs_in[r][i], rs_out[r][i], S, s)

    run_ranks(n, body)
    torch.cuda.synchronize()
    for c in comms:
        c.set_algo(AUTO)
        c.set_broadcast_kind(0)
    assert comms[0].ipc_status() & 1 == 0
    for i in range(iters):
        root = i % n
        want_gv = torch.full_like(gv_out[0][i], -1)
        for q in range(n):
            want_gv[gd[i][q]:gd[i][q] + gv[i][q]] = gv_in[q][i]
        for r in range(n):
            assert torch.equal(sc_out[r][i], sc_in[root][i][r * cnt[i]:(r + 1) * cnt[i]]), (i, r)
            assert torch.equal(gv_out[r][i], want_gv), (i, r)
            assert torch.equal(bc[r][i], want_bc[i]), (i, r)
            want_a2a = torch.cat([a2a_in[q][i][r * 301:(r + 1) * 301] for q in range(n)])
            assert torch.equal(a2a_out[r][i], want_a2a), (i, r)
            want_rs = sum(rs_in[q][i][r * 257:(r + 1) * 257] for q in range(n))
            assert torch.equal(rs_out[r][i], want_rs), (i, r)
