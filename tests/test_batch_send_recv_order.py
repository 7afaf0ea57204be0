"""HcclBatchSendRecv's host list handling (HcclAmdBatchSendRecvOrder = hccl_amd/csrc/ipc_plan.cc BatchSendRecvOrder)
against the reference's rule (ins_v2_batch_send_recv_executor.cc:106-208), restated here: items of count 0 are dropped;
the sends are stably sorted from this rank downwards (cyclic, self first), the receives from it upwards, duplicates of a
pair by count, then data type, both descending; the leading self items pair up, and a self item left over, or a pair of
unequal counts, is HCCL_E_PARA. CPU only."""
import functools
import random

import pytest

import hccl_amd as H

SEND, RECV = int(H.SendRecvType.SEND), int(H.SendRecvType.RECV)
BUF = 0x1000  # never dereferenced


def reference_order(items, me, n):
    """The rule as the reference states it; items are (type, count, dtype, remote). Returns None for HCCL_E_PARA."""
    keep = [i for i, it in enumerate(items) if it[1] > 0]
    sends = [i for i in keep if items[i][0] == SEND]
    recvs = [i for i in keep if items[i][0] == RECV]

    def size_cmp(a, b):
        (_, ca, da, _), (_, cb, db, _) = items[a], items[b]
        return (cb > ca) - (cb < ca) or (db > da) - (db < da)

    def send_cmp(a, b):
        fa = items[a][3] + n if items[a][3] <= me else items[a][3]
        fb = items[b][3] + n if items[b][3] <= me else items[b][3]
        return (fb > fa) - (fb < fa) or size_cmp(a, b)

    def recv_cmp(a, b):
        fa = items[a][3] + n if items[a][3] < me else items[a][3]
        fb = items[b][3] + n if items[b][3] < me else items[b][3]
        return (fa > fb) - (fa < fb) or size_cmp(a, b)

    sends.sort(key=functools.cmp_to_key(send_cmp))  # list.sort is stable
    recvs.sort(key=functools.cmp_to_key(recv_cmp))
    pairs = []
    while sends and recvs and items[sends[0]][3] == me and items[recvs[0]][3] == me:
        pairs.append((sends.pop(0), recvs.pop(0)))
    if (sends and items[sends[0]][3] == me) or (recvs and items[recvs[0]][3] == me):
        return None
    if any(items[s][1] != items[r][1] for s, r in pairs):
        return None
    return sends, recvs, pairs


def library_order(items, me, n):
    try:
        return H.batch_send_recv_order([(t, (BUF, c, d), q) for t, c, d, q in items], me, n)
    except H.HcclError as e:
        assert e.code == H.HcclResult.HCCL_E_PARA
        return None


def test_duplicates_sort_by_count_then_type_so_two_listings_match():
    FP32, INT8, FP16 = 4, 0, 3
    a = [(SEND, 5, FP32, 1), (SEND, 9, INT8, 1), (SEND, 5, FP16, 1), (SEND, 5, FP32, 1)]
    b = [a[2], a[3], a[0], a[1]]
    oa, ob = library_order(a, 0, 2)[0], library_order(b, 0, 2)[0]
    assert [a[i][1:3] for i in oa] == [b[i][1:3] for i in ob] == [(9, INT8), (5, FP32), (5, FP32), (5, FP16)]
    assert oa == [1, 0, 3, 2]  # stable among equals
    # the receiver's listing of the same messages, in yet another order, sorts the same way
    r = [(RECV, 5, FP16, 0), (RECV, 5, FP32, 0), (RECV, 9, INT8, 0), (RECV, 5, FP32, 0)]
    assert [r[i][1:3] for i in library_order(r, 1, 2)[1]] == [a[i][1:3] for i in oa]


def test_zero_counts_are_dropped_even_with_a_null_buffer_or_a_bad_type():
    arr = H.send_recv_items([(SEND, (0, 0, 4), 1), (7, (0, 0, 4), 1), (RECV, (BUF, 3, 4), 1)])
    import ctypes
    order = (ctypes.c_uint32 * 3)()
    ns, nr, np_ = ctypes.c_uint32(9), ctypes.c_uint32(9), ctypes.c_uint32(9)
    assert H.lib.HcclAmdBatchSendRecvOrder(arr, 3, 0, 2, order, ns, nr, np_) == 0
    assert (ns.value, nr.value, np_.value, order[0]) == (0, 1, 0, 2)
    arr = H.send_recv_items([(SEND, (0, 4, 4), 1)])
    assert H.lib.HcclAmdBatchSendRecvOrder(arr, 1, 0, 2, order, ns, nr, np_) == H.HcclResult.HCCL_E_PTR
    arr = H.send_recv_items([(7, (BUF, 4, 4), 1)])
    assert H.lib.HcclAmdBatchSendRecvOrder(arr, 1, 0, 2, order, ns, nr, np_) == H.HcclResult.HCCL_E_PARA


def test_self_pairs_and_their_errors():
    assert library_order([(SEND, 4, 4, 2), (RECV, 4, 4, 2), (SEND, 8, 4, 2), (RECV, 8, 0, 2)], 2, 4) == \
        ([], [], [(2, 3), (0, 1)])
    assert library_order([(SEND, 4, 4, 2)], 2, 4) is None                      # no receive from self
    assert library_order([(RECV, 4, 4, 2), (SEND, 4, 4, 1)], 2, 4) is None     # no send to self
    assert library_order([(SEND, 4, 4, 2), (RECV, 5, 4, 2)], 2, 4) is None     # unequal counts
    assert library_order([(SEND, 4, 4, 0), (RECV, 4, 4, 0)], 0, 1) == ([], [], [(0, 1)])  # one rank: self pairs only


@pytest.mark.parametrize("seed", range(8))
def test_random_lists_match_the_restated_rule(seed):
    rng = random.Random(seed)
    for _ in range(300):
        n = rng.choice((1, 2, 3, 4, 8, 16))
        me = rng.randrange(n)
        items = [(rng.choice((SEND, RECV)), rng.choice((0, 1, 1, 2, 7)), rng.choice((0, 3, 4, 5)), rng.randrange(n))
                 for _ in range(rng.randrange(0, 10))]
        assert library_order(items, me, n) == reference_order(items, me, n), (items, me, n)
