"""HcclBatchSendRecv on the GPU, on both data paths (the transport's group, and k_ipc_p2p after enable_p2p() with the
IPC override), in loopback worlds, bit-exact: the reference's three shapes (bidirectional ring, two neighbours as
batch_send_recv_testcase.cc:149-152 lists them, full mesh), duplicates to one peer listed in different orders on the two
sides, a self pair, the HCCL_E_PARA of an unmatched self item, itemNum == 0, and, on an RCCL self-loop communicator, a
batch whose receive gets this rank's own send."""
import pytest
import torch

import hccl_amd as H
from test_gpu_broadcast import run_ranks
from test_gpu_send_recv import PATHS, SLOT, worlds  # noqa: F401  (the module-scoped worlds fixture)

pytestmark = pytest.mark.gpu

SEND, RECV = H.SendRecvType.SEND, H.SendRecvType.RECV


def payload(src, dst, k, count, dt=torch.int32):
    g = torch.Generator().manual_seed(src * 1000 + dst * 10 + k)
    return torch.randint(0, 256, (count * torch.empty(0, dtype=dt).element_size(),), dtype=torch.uint8,
                         generator=g).cuda().view(dt)


def run_batches(comms, plan):
    """plan[r] = list of (type, peer, k, count, dtype): rank r's items, in its listing order. A send carries
    payload(r, peer, k); every receive is checked against the payload its sender made."""
    n = len(comms)
    bufs = [[payload(r, q, k, c, dt) if t == SEND else torch.zeros(
        c * torch.empty(0, dtype=dt).element_size(), dtype=torch.uint8, device="cuda").view(dt) for t, q, k, c, dt in plan[r]] for r in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    torch.cuda.synchronize()
    run_ranks(n, lambda r: comms[r].batch_send_recv([(t, b, q) for (t, q, _, _, _), b in zip(plan[r], bufs[r])],
                                                    streams[r]))
    torch.cuda.synchronize()
    for r in range(n):
        for (t, q, k, c, dt), b in zip(plan[r], bufs[r]):
            want = payload(r, q, k, c, dt) if t == SEND else payload(q, r, k, c, dt)
            assert torch.equal(b.view(torch.uint8), want.view(torch.uint8)), (r, t, q, k, c)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [2, 4])
def test_bidirectional_ring(worlds, n, path):
    c = SLOT // 4 + 3
    plan = [[(SEND, (r + 1) % n, 0, c, torch.int32), (RECV, (r - 1) % n, 0, c, torch.int32),
             (SEND, (r - 1) % n, 1, 7, torch.int32), (RECV, (r + 1) % n, 1, 7, torch.int32)] for r in range(n)]
    run_batches(worlds(n, path), plan)


@pytest.mark.parametrize("path", PATHS)
def test_two_neighbours(worlds, path):
    """Every rank sends to and receives from both neighbours, sends listed first (the reference's test case)."""
    n, c = 4, 2 * SLOT // 2 + 5  # fp16: more than two slots, so the senders need credits while they also receive
    plan = [[(SEND, (r - 1) % n, 0, c, torch.float16), (SEND, (r + 1) % n, 0, c, torch.float16),
             (RECV, (r - 1) % n, 0, c, torch.float16), (RECV, (r + 1) % n, 0, c, torch.float16)] for r in range(n)]
    run_batches(worlds(n, path), plan)


@pytest.mark.parametrize("path", PATHS)
def test_full_mesh_with_mixed_types(worlds, path):
    n = 4
    dts = [torch.int8, torch.float16, torch.int32, torch.int64]
    plan = [[(SEND, q, 0, 100 + r + q, dts[(r + q) % 4]) for q in range(n) if q != r] +
            [(RECV, q, 0, 100 + r + q, dts[(r + q) % 4]) for q in range(n) if q != r] for r in range(n)]
    run_batches(worlds(n, path), plan)


@pytest.mark.parametrize("path", PATHS)
def test_duplicates_listed_in_different_orders(worlds, path):
    """Three messages 0 -> 1 of different counts and types; rank 1 lists its receives in another order. The k of an
    item is its rank in the sort (count, then data type, descending), which is what pairs them."""
    msgs = [(0, 900, torch.int32), (1, 33, torch.int64), (2, 33, torch.int32)]
    plan = [[(SEND, 1, k, c, dt) for k, c, dt in (msgs[2], msgs[0], msgs[1])],
            [(RECV, 0, k, c, dt) for k, c, dt in (msgs[1], msgs[2], msgs[0])]]
    run_batches(worlds(2, path), plan)


@pytest.mark.parametrize("path", PATHS)
def test_self_pair_and_unmatched_self_item(worlds, path):
    comms = worlds(2, path)
    plan = [[(SEND, 0, 0, 50, torch.int32), (RECV, 0, 0, 50, torch.int32), (SEND, 1, 1, 9, torch.int32)],
            [(RECV, 0, 1, 9, torch.int32)]]
    run_batches(comms, plan)
    buf = torch.zeros(8, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()  # (the default stream's handle is NULL, which the entry refuses)
    with pytest.raises(H.HcclError) as e:
        comms[0].batch_send_recv([(SEND, buf, 0)], st)
    assert e.value.code == H.HcclResult.HCCL_E_PARA
    with pytest.raises(H.HcclError) as e:
        comms[0].batch_send_recv([(SEND, buf, 0), (RECV, buf[:4], 0)], st)
    assert e.value.code == H.HcclResult.HCCL_E_PARA
    with pytest.raises(H.HcclError) as e:
        comms[0].batch_send_recv([(SEND, buf, 2)], st)  # outside the communicator
    assert e.value.code == H.HcclResult.HCCL_E_PARA
    comms[0].batch_send_recv([], st)  # itemNum == 0
    assert H.lib.HcclBatchSendRecv(None, 0, None, None) == 0
    assert comms[0].async_error() == 0


def test_rccl_self_loop_returns_the_ranks_own_data():
    """The one-rank RCCL stand-in of a 4-rank world: {send to 1, recv from 3} of equal count runs and the receive gets
    this rank's own send; a lone Send or Recv cannot run there."""
    c = H.comm_init_selfloop(4, 0)
    try:
        src, dst = payload(0, 1, 0, 5000), torch.zeros(5000, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        c.batch_send_recv([(SEND, src, 1), (RECV, dst, 3)], st)
        torch.cuda.synchronize()
        assert torch.equal(dst, src)
        for call in (lambda: c.send(src, 1, st), lambda: c.recv(dst, 3, st)):
            with pytest.raises(H.HcclError) as e:
                call()
            assert e.value.code == H.HcclResult.HCCL_E_NOT_SUPPORT
    finally:
        c.destroy()
