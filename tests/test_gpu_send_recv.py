"""HcclSend / HcclRecv on the GPU, on both data paths, in loopback worlds (n ranks in one process on the one GPU, one
thread and one stream per rank): the transport's group, and the one-sided kernel (k_ipc_p2p) after enable_p2p() with
the IPC override, where every message really travels through the slots and flag words of the p2p area.

Data is moved bit for bit, so every comparison is on raw bytes: random bytes (NaN payloads included), 64 guard bytes of
0xA5 on each side of every buffer. A lone Send meets its Recv on the host in a loopback world, so a ring shift posts
Send first on even ranks and Recv first on odd ones. No test leaves a message unmatched.
"""
import pytest
import torch

import hccl_amd as H
from test_gpu_broadcast import GUARD, guarded, run_ranks

pytestmark = pytest.mark.gpu

IPC, AUTO = int(H.Algo.IPC), int(H.Algo.AUTO)
SLOT = H.P2P_SLOT_BYTES_DEFAULT
PATHS = ["transport", "ipc"]
DTYPES = [torch.int8, torch.float16, torch.float32, torch.int64, torch.float8_e4m3fn]


def _esize(dt):
    return torch.empty(0, dtype=dt).element_size()


def counts_for(dt):
    """1, 3, slotElems - 1, slotElems + 1 and 2 slotElems + 5: the last needs a credit from the receiver."""
    se = SLOT // _esize(dt)
    return [1, 3, se - 1, se + 1, 2 * se + 5]


@pytest.fixture(scope="module")
def worlds():
    cache, grown = {}, {}
    mp_ = pytest.MonkeyPatch()
    mp_.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")  # a stuck wait fails the test, never hangs the box

    def get(n, path):
        if (n, path) not in cache:
            comms = cache[(n, path)] = H.loopback_world(n)
            for c in comms:
                c.set_algo(IPC)
            if path == "ipc":
                # a one-sided collective first, so that enable_p2p() adds the p2p allocations alone
                bufs = [torch.ones(64, dtype=torch.float32, device="cuda") for _ in range(n)]
                streams = [torch.cuda.Stream() for _ in range(n)]
                torch.cuda.synchronize()
                run_ranks(n, lambda r: comms[r].all_reduce(bufs[r], bufs[r], stream=streams[r]))
                torch.cuda.synchronize()
                before = [c.device_bytes() for c in comms]
                run_ranks(n, lambda r: comms[r].enable_p2p())
                run_ranks(n, lambda r: comms[r].enable_p2p())  # idempotent
                grown[n] = [c.device_bytes() - b for c, b in zip(comms, before)]
        return cache[(n, path)]

    get.grown = grown
    yield get
    torch.cuda.synchronize()
    for comms in cache.values():
        for c in comms:
            c.destroy()
    mp_.undo()


def untouched(whole, lo, nbytes):
    return bool((whole[:lo] == 0xA5).all()) and bool((whole[lo + nbytes:] == 0xA5).all())


def post_pair(comm, r, send, dst, recv, src, stream):
    """This rank's Send and Recv of a ring step, in the order that lets lone calls meet on the host."""
    if r % 2 == 0:
        comm.send(send, dst, stream)
        comm.recv(recv, src, stream)
    else:
        comm.recv(recv, src, stream)
        comm.send(send, dst, stream)


def ring_shift(comms, path, counts, dt, shift=0, seed=0):
    """Every rank sends len(counts) messages to its right neighbour and receives as many from its left one."""
    n, es = len(comms), _esize(dt)
    sb = shift * es
    sent = [[guarded(c * es, sb, seed * 256 + r * 16 + k) for k, c in enumerate(counts)] for r in range(n)]
    got = [[guarded(c * es, sb, seed * 256 + r * 16 + k + 8) for k, c in enumerate(counts)] for r in range(n)]
    want = [[v.clone() for _, v in row] for row in sent]
    streams = [torch.cuda.Stream() for _ in range(n)]
    torch.cuda.synchronize()

    def body(r):
        for k in range(len(counts)):
            post_pair(comms[r], r, sent[r][k][1].view(dt), (r + 1) % n, got[r][k][1].view(dt), (r - 1) % n, streams[r])

    run_ranks(n, body)
    torch.cuda.synchronize()
    for r in range(n):
        for k, c in enumerate(counts):
            what = (n, path, c, dt, shift, r, k)
            assert torch.equal(got[r][k][1], want[(r - 1) % n][k]), what
            assert torch.equal(sent[r][k][1], want[r][k]), what
            assert untouched(got[r][k][0], GUARD + sb, c * es), what
        assert comms[r].last_algo == (IPC if path == "ipc" else int(H.Algo.MESH_ONESHOT)), (n, path, r)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_ring_shift_is_bit_exact(worlds, n, path, dt):
    for k, count in enumerate(counts_for(dt)):
        ring_shift(worlds(n, path), path, [count], dt, seed=k)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dt", [torch.int8, torch.float16, torch.float32])
def test_buffers_shifted_by_one_element(worlds, path, dt):
    se = SLOT // _esize(dt)
    for k, count in enumerate([3, se + 1]):
        ring_shift(worlds(2, path), path, [count], dt, shift=1, seed=10 + k)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [2, 4])
def test_two_messages_on_one_pair_arrive_in_order(worlds, n, path):
    se = SLOT // 4
    ring_shift(worlds(n, path), path, [se + 7, 5], torch.float32, seed=20)
    ring_shift(worlds(n, path), path, [1, 2 * se + 1], torch.float32, seed=21)


@pytest.mark.parametrize("path", PATHS)
def test_p2p_between_collectives_leaves_the_epochs_alone(worlds, path):
    """Ranks 0 and 1 exchange messages, all four ranks run an AllReduce and a Scatter, then 0 and 1 exchange again:
    a point-to-point launch that touched the collectives' epochs or flags on two ranks only would end the collectives
    in their barrier."""
    comms, n, dt = worlds(4, path), 4, torch.float32
    se = SLOT // 4

    def exchange(seed, count):
        pair = comms[:2]
        sent = [guarded(count * 4, 0, seed + r) for r in range(2)]
        got = [guarded(count * 4, 0, seed + 8 + r) for r in range(2)]
        want = [v.clone() for _, v in sent]
        streams = [torch.cuda.Stream() for _ in range(2)]
        torch.cuda.synchronize()
        run_ranks(2, lambda r: post_pair(pair[r], r, sent[r][1].view(dt), 1 - r, got[r][1].view(dt), 1 - r, streams[r]))
        torch.cuda.synchronize()
        for r in range(2):
            assert torch.equal(got[r][1], want[1 - r]), (path, seed, r)

    exchange(300, 2 * se + 5)
    ins = [torch.full((1000,), float(r + 1), dtype=dt, device="cuda") for r in range(n)]
    outs = [torch.empty(1000, dtype=dt, device="cuda") for _ in range(n)]
    src = torch.arange(n * 333, dtype=dt, device="cuda")
    parts = [torch.empty(333, dtype=dt, device="cuda") for _ in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    torch.cuda.synchronize()

    def collectives(r):
        comms[r].all_reduce(ins[r], outs[r], stream=streams[r])
        comms[r].scatter(src if r == 2 else None, parts[r], 2, streams[r])

    run_ranks(n, collectives)
    torch.cuda.synchronize()
    for r in range(n):
        assert torch.equal(outs[r], torch.full((1000,), 10.0, dtype=dt, device="cuda")), (path, r)
        assert torch.equal(parts[r], src[r * 333:(r + 1) * 333]), (path, r)
    exchange(400, se + 1)
    exchange(500, 3)
    for c in comms:
        assert c.ipc_status() & 0xFF == 0  # the sticky bits; the bits above are the last collective's longest wait
        assert c.async_error() == 0


def test_count_zero_succeeds_with_no_peer_call(worlds):
    c = worlds(2, "transport")[0]
    L = H.lib
    assert L.HcclSend(None, 0, 99, 7, None, None) == 0  # before any other check
    assert L.HcclRecv(None, 0, 99, 7, None, None) == 0
    buf = torch.zeros(4, device="cuda")
    st = torch.cuda.Stream()
    c.send(buf[:0], 1, st)  # returns at once: rank 1 posts nothing
    c.recv(buf[:0], 1, st)


def test_argument_checks_and_their_codes(worlds):
    c = worlds(4, "transport")[1]  # rank 1 of 4
    L, E, FP32 = H.lib, H.HcclResult, int(H.HcclDataType.FP32)
    buf = torch.zeros(16, device="cuda")
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL)
    p, s, h = buf.data_ptr(), stream.cuda_stream, c.handle
    for fn in (L.HcclSend, L.HcclRecv):
        assert fn(p, 4, FP32, 0, None, s) == E.HCCL_E_PTR            # comm
        assert fn(None, 4, FP32, 0, h, s) == E.HCCL_E_PTR            # buffer
        assert fn(p, 4, FP32, 0, h, None) == E.HCCL_E_PTR            # stream
        assert fn(p, 0x7FFFFFFFF + 1, FP32, 0, h, s) == E.HCCL_E_PARA  # CheckCount before the data type
        assert fn(p, 0x7FFFFFFFF + 1, 12, 0, h, s) == E.HCCL_E_PARA
        assert fn(p, 4, int(H.HcclDataType.INT128), 0, h, s) == E.HCCL_E_NOT_SUPPORT
        assert fn(p, 4, 13, 0, h, s) == E.HCCL_E_NOT_SUPPORT         # the gap in the numbering
        assert fn(p, 4, 12, 1, h, s) == E.HCCL_E_NOT_SUPPORT         # the data type before the peer
        assert fn(p, 4, FP32, 1, h, s) == E.HCCL_E_NOT_SUPPORT       # the peer is this rank
        assert fn(p, 4, FP32, 4, h, s) == E.HCCL_E_PARA              # outside the communicator
    one = H.loopback_world(1)[0]
    try:  # a one-rank communicator: the only rank is self
        assert L.HcclSend(p, 4, FP32, 0, one.handle, s) == E.HCCL_E_NOT_SUPPORT
        assert L.HcclRecv(p, 4, FP32, 1, one.handle, s) == E.HCCL_E_PARA
    finally:
        one.destroy()
    assert c.async_error() == 0


def test_without_enable_p2p_the_transport_runs_and_holds_nothing_more(worlds):
    comms = worlds(2, "transport")  # the IPC override is set, but p2p was never enabled
    before = [c.device_bytes() for c in comms]
    ring_shift(comms, "transport", [1000], torch.float32, seed=30)
    assert [c.device_bytes() for c in comms] == before
    assert all(c.last_algo != IPC for c in comms)


@pytest.mark.parametrize("n", [2, 4])
def test_enable_p2p_grows_device_bytes_by_the_planned_area_and_counters(worlds, n):
    worlds(n, "ipc")
    plan = H.p2p_plan(0, 1, SLOT, n)
    assert worlds.grown[n] == [plan.areaBytes + plan.counterBytes] * n
