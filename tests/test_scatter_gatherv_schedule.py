"""HcclScatter's and HcclAllGatherV's schedule path, host only.

Both mesh programs (schedule.cc ScatterMesh, AllGatherVMesh; ins_temp_scatter_mesh_1D.cc,
ins_temp_all_gather_v_mesh_1D.cc) move data only: COPY / SEND / RECV records on the caller's buffers, no staging and no
fold. Checked here: the oracle's replay of the n programs against numpy on raw bytes; the groups are live under RCCL's
rendezvous rule (test_group_liveness.check_live); with an explicit piece size both ends of every pair post the same
pieces; the executor's plan leaves no unordered conflict, in particular for the in-place Scatter on a root other than
0, whose own-block COPY writes where block 0's SEND reads (and the check is shown to fail once that dependency is taken
out of the plan).
"""
import ctypes
import random

import numpy as np
import pytest

import hccl_amd as H
from oracle import oracle as O
from test_executor_hazards import _conflict, _ranges
from test_group_liveness import check_live, groups_of

SCATTER, AGV = 7, 8
ONESHOT = 1
COPY, SEND, RECV = 0, 2, 3
NP_OF = {O.INT8: np.uint8, O.FP16: np.uint16, O.FP32: np.uint32, O.INT64: np.int64}  # element sizes 1, 2, 4, 8


def roots(n):
    return sorted({0, n // 2, n - 1})


def scatter_programs(n, root, count, dtype, piece, algo=0):
    progs = []
    for r in range(n):
        arr, nops, used, scratch = H.build_schedule(SCATTER, algo, n, r, count, dtype, root, piece)
        assert used == ONESHOT and scratch == 0
        assert all(arr[i].kind in (COPY, SEND, RECV) for i in range(nops))
        progs.append((arr, nops))
    return progs


def gather_programs(counts, displs, dtype, piece, in_place=False):
    n = len(counts)
    progs = []
    for r in range(n):
        arr, nops, scratch = H.build_schedule_all_gather_v(n, r, counts, displs, dtype, piece, in_place)
        assert scratch == 0
        assert all(arr[i].kind in (COPY, SEND, RECV) for i in range(nops))
        progs.append((arr, nops))
    return progs


def count_vectors(n):
    return {
        "equal": [40] * n,
        "ragged": [(1, 300, 0, 77, 64, 3, 129, 5)[q % 8] for q in range(n)],
        "one_zero": [0 if q == n // 2 else 30 + 7 * q for q in range(n)],
        "only_one": [300 if q == n - 1 else 0 for q in range(n)],
    }


def layouts(counts):
    n = len(counts)
    return {
        "packed": [sum(counts[:q]) for q in range(n)],
        "gaps": [sum(counts[:q]) + 5 * (q + 1) for q in range(n)],
        "descending": [sum(counts[q + 1:]) + 2 * (n - 1 - q) for q in range(n)],
    }


def replay_scatter(n, root, count, dtype, piece, seed, in_place=False):
    npdt = NP_OF[dtype]
    es = np.dtype(npdt).itemsize
    rng = np.random.default_rng(seed)
    progs = scatter_programs(n, root, count, dtype, piece)
    src = rng.integers(0, 256, (n * count + 3) * es, dtype=np.uint8).view(npdt)
    keep = src.copy()
    ins = [src if r == root else np.zeros(1, dtype=npdt) for r in range(n)]
    outs = [rng.integers(0, 256, (count + 3) * es, dtype=np.uint8).view(npdt) for _ in range(n)]
    if in_place:
        outs[root] = src
    tails = [o[count:].copy() for o in outs]
    scratch = np.zeros(1, dtype=npdt)
    assert O.replay(n, dtype, O.SUM, progs, [[ins[r], outs[r], scratch] for r in range(n)]) == 0
    what = (n, root, count, dtype, piece, in_place)
    for r in range(n):
        assert outs[r][:count].tobytes() == keep[r * count:(r + 1) * count].tobytes(), (what, r)
        if not (in_place and r == root):
            assert outs[r][count:].tobytes() == tails[r].tobytes(), (what, r)
    if in_place:
        assert src[count:].tobytes() == keep[count:].tobytes(), what
    else:
        assert src.tobytes() == keep.tobytes(), what


def replay_gather(counts, displs, dtype, piece, seed, in_place=False):
    n = len(counts)
    npdt = NP_OF[dtype]
    es = np.dtype(npdt).itemsize
    rng = np.random.default_rng(seed)
    progs = gather_programs(counts, displs, dtype, piece, in_place)
    out_len = max(displs[q] + counts[q] for q in range(n)) + 3
    data = [rng.integers(0, 256, counts[r] * es, dtype=np.uint8).view(npdt) for r in range(n)]
    outs = [rng.integers(0, 256, out_len * es, dtype=np.uint8).view(npdt) for _ in range(n)]
    wants = []
    for r in range(n):
        want = outs[r].copy()  # gaps between the blocks stay as they were
        for q in range(n):
            want[displs[q]:displs[q] + counts[q]] = data[q]
        wants.append(want)
    if in_place:
        for r in range(n):
            outs[r][displs[r]:displs[r] + counts[r]] = data[r]
        ins = [outs[r][displs[r]:] for r in range(n)]  # the input is the own block's place in the output
    else:
        ins = [np.concatenate([data[r], np.zeros(1, dtype=npdt)]) for r in range(n)]
    scratch = np.zeros(1, dtype=npdt)
    assert O.replay(n, dtype, O.SUM, progs, [[ins[r], outs[r], scratch] for r in range(n)]) == 0
    for r in range(n):
        assert outs[r].tobytes() == wants[r].tobytes(), (counts, displs, dtype, piece, in_place, r)
        if not in_place:
            assert ins[r][:counts[r]].tobytes() == data[r].tobytes(), (counts, displs, r)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_scatter_replay(n):
    for root in roots(n):
        for dtype in NP_OF:
            for count in (1, n + 1, 1000):
                for piece in (0, 128):
                    replay_scatter(n, root, count, dtype, piece, seed=n * 100 + root)
                    replay_scatter(n, root, count, dtype, piece, seed=n * 100 + root, in_place=True)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_all_gather_v_replay(n):
    seed = 0
    for counts in count_vectors(n).values():
        for displs in layouts(counts).values():
            for dtype in NP_OF:
                for piece in (0, 128):
                    seed += 1
                    replay_gather(counts, displs, dtype, piece, seed)
                    replay_gather(counts, displs, dtype, piece, seed, in_place=True)


def test_random_sweep():
    rng = random.Random(20241021)
    for draw in range(150):
        n = rng.randint(1, 16)
        dtype = rng.choice(list(NP_OF))
        piece = rng.choice((0, 128, 1024))
        replay_scatter(n, rng.randrange(n), rng.choice((1, n + 1, rng.randint(1, 3000))), dtype, piece, seed=draw,
                       in_place=rng.random() < 0.5)
        counts = [rng.choice((0, 1, rng.randint(0, 40), rng.randint(0, 700))) for _ in range(n)]
        order = list(range(n))
        rng.shuffle(order)
        displs, at = [0] * n, 0
        for q in order:  # blocks in any order, with gaps
            at += rng.randrange(3)
            displs[q] = at
            at += counts[q]
        replay_gather(counts, displs, dtype, piece, seed=draw, in_place=rng.random() < 0.5)


def test_records_and_selector():
    """One COPY on the root and one SEND per peer; one RECV on a peer. AllGatherV: a COPY unless in place, one SEND of
    the whole input and one RECV per peer with a non-zero count. One transport group by default. Every family is this
    one schedule."""
    n, count = 5, 300
    for root in roots(n):
        for r, (arr, nops) in enumerate(scatter_programs(n, root, count, O.FP16, 0)):
            kinds = [arr[i].kind for i in range(nops)]
            if r == root:
                assert kinds == [SEND] * (n - 1) + [COPY]
                assert sorted(arr[i].srcOff[0] for i in range(n - 1)) == [q * count for q in range(n) if q != root]
                assert (arr[n - 1].srcOff[0], arr[n - 1].dstOff, arr[n - 1].count) == (root * count, 0, count)
            else:
                assert kinds == [RECV] and (arr[0].peer, arr[0].dstOff, arr[0].count) == (root, 0, count)
            assert len(groups_of(arr, nops)) == 1
    counts = count_vectors(n)["one_zero"]
    displs = layouts(counts)["gaps"]
    for in_place in (False, True):
        for r, (arr, nops) in enumerate(gather_programs(counts, displs, O.FP16, 0, in_place)):
            ops = [arr[i] for i in range(nops)]
            copies = [o for o in ops if o.kind == COPY]
            assert len(copies) == (0 if in_place or counts[r] == 0 else 1)
            for o in copies:
                assert (o.srcOff[0], o.dstOff, o.count) == (0, displs[r], counts[r])
            sends = [o for o in ops if o.kind == SEND]
            assert len(sends) == (n - 1 if counts[r] else 0)
            assert all(o.srcOff[0] == 0 and o.count == counts[r] for o in sends)
            recvs = {o.peer: (o.dstOff, o.count) for o in ops if o.kind == RECV}
            assert recvs == {q: (displs[q], counts[q]) for q in range(n) if q != r and counts[q]}
            assert len(groups_of(arr, nops)) <= 1
    for arr, nops in gather_programs([0] * n, [0] * n, O.FP16, 0):
        assert nops == 0
    for op in (SCATTER, AGV):
        for nbytes in (1, 1 << 20, 1 << 30):
            assert H.select_algo(op, 8, nbytes) == ONESHOT
    base = scatter_programs(4, 1, 1000, O.FP16, 0)
    for algo in range(1, 13):
        for (a, na), (b, nb) in zip(base, scatter_programs(4, 1, 1000, O.FP16, 0, algo=algo)):
            assert na == nb and bytes(a) == bytes(b)
    n_ops = ctypes.c_uint64(0)
    assert H.lib.HcclAmdBuildSchedule(SCATTER, 0, 4, 0, 100, O.FP16, 4, 0, None, 0, ctypes.byref(n_ops), None,
                                      None) == H.HcclResult.HCCL_E_PARA  # root out of range
    # the generic export cannot carry AllGatherV's arrays: it refuses the op
    assert H.lib.HcclAmdBuildSchedule(AGV, 0, 4, 0, 100, O.FP16, 0, 0, None, 0, ctypes.byref(n_ops), None,
                                      None) == H.HcclResult.HCCL_E_PARA
    assert int(H.OpType.SCATTER) == SCATTER and int(H.OpType.ALLGATHER_V) == AGV


@pytest.mark.parametrize("n", [2, 3, 8])
def test_groups_are_live(n):
    for root in roots(n):
        for count, piece in [(1, 0), (n + 1, 0), (1000, 128), (65537, 4096)]:
            check_live([groups_of(*p) for p in scatter_programs(n, root, count, O.FP16, piece)])
    seen = set()
    vectors = count_vectors(n)
    vectors["skew"] = [70001] + [1] * (n - 1)  # rank 0's block takes many groups, the others' one
    for name, counts in vectors.items():
        for displs in layouts(counts).values():
            for piece in (0, 128, 4096):
                progs = [groups_of(*p) for p in gather_programs(counts, displs, O.FP16, piece)]
                check_live(progs)
                if name == "skew" and piece == 128:
                    seen |= {len(g) for g in progs}
    assert len(seen) == 1 and seen.pop() > 1  # every rank receives rank 0's pieces: all post the same groups


def pieces_by_pair(progs):
    """{(sender, receiver): [(group, count), ..]} as the senders post them, and the same as the receivers do."""
    sent, received = {}, {}
    for r, (arr, nops) in enumerate(progs):
        for i in range(nops):
            o = arr[i]
            if o.kind == SEND:
                sent.setdefault((r, o.peer), []).append((o.group, o.count))
            elif o.kind == RECV:
                received.setdefault((o.peer, r), []).append((o.group, o.count))
    return sent, received


@pytest.mark.parametrize("n", [2, 3, 8])
def test_both_ends_cut_alike(n):
    """With pieceBytes set, the sender and the receiver of every pair post the same pieces in groups of the same index,
    although the ranks' payloads differ (the root's is n times a peer's; every AllGatherV block has its own size)."""
    for piece in (128, 1024):
        for root in roots(n):
            sent, received = pieces_by_pair(scatter_programs(n, root, 3001, O.FP16, piece))
            assert sent == received and len(sent) == n - 1
            assert all(len(v) == -(-3001 * 2 // piece) for v in sent.values())
        for counts in count_vectors(n).values():
            sent, received = pieces_by_pair(gather_programs(counts, layouts(counts)["gaps"], O.FP16, piece))
            assert sent == received
            assert len(sent) == sum(1 for c in counts if c) * (n - 1)


def unordered_conflicts(arr, units, es, bases):
    """Pairs of units on different streams that touch the same bytes, one of them writing, and that the plan leaves
    unordered; and messages of one group that meet. The rule of test_executor_hazards."""
    rng = [_ranges(arr, u["first"], u["num"], es, bases) for u in units]
    before, last, bad = [], {0: -1, 1: -1}, []
    for k, u in enumerate(units):
        hb = 0
        for p in (last[u["stream"]], u["wait"]):
            if p >= 0:
                hb |= before[p] | (1 << p)
        before.append(hb)
        last[u["stream"]] = k
    for b, ub in enumerate(units):
        for a in range(b):
            if units[a]["stream"] != ub["stream"] and not (before[b] >> a) & 1 and _conflict(rng[a], rng[b]):
                bad.append((a, b))
        if not ub["comm"]:
            continue  # (in place on root 0 the own-block COPY reads and writes the same bytes: it changes nothing)
        for i, x in enumerate(rng[b]):
            for y in rng[b][i + 1:]:
                if _conflict([x], [y]):
                    bad.append((b, b))
    return bad


@pytest.mark.parametrize("n", [2, 3, 8])
def test_executor_hazards(n):
    es = 2
    apart = (1 << 40, 2 << 40, 3 << 40)
    aliased = (1 << 40, 1 << 40, 3 << 40)
    for count, piece in [(1, 0), (n + 1, 0), (1000, 128), (300001, 4096)]:
        for root in roots(n):
            for bases in (apart, aliased):  # aliased: recvBuf == sendBuf, legal on the root
                arr, nops = scatter_programs(n, root, count, O.FP16, piece)[root]
                assert unordered_conflicts(arr, H.executor_plan(arr, nops, es, bases), es, bases) == []
    for counts in count_vectors(n).values():
        for displs in layouts(counts).values():
            for in_place in (False, True):
                for r, (arr, nops) in enumerate(gather_programs(counts, displs, O.FP16, 128, in_place)):
                    base_in = (2 << 40) + displs[r] * es if in_place else 1 << 40
                    bases = (base_in, 2 << 40, 3 << 40)
                    assert unordered_conflicts(arr, H.executor_plan(arr, nops, es, bases), es, bases) == []


@pytest.mark.parametrize("piece", [0, 128])
def test_in_place_scatter_orders_the_copy_after_block_0s_send(piece):
    """Root 1, recvBuf == sendBuf: the own-block COPY writes bytes [0, count) of the buffer, which block 0's SEND
    reads. In program order (the single-stream executor) the COPY follows every SEND; in the two-stream plan the COPY's
    unit waits for the group that holds the last piece of block 0. Without that wait the checker above reports the
    conflict, so it does test the dependency."""
    n, root, count, es = 3, 1, 1000, 2
    bases = (1 << 40, 1 << 40, 3 << 40)
    arr, nops = scatter_programs(n, root, count, O.FP16, piece)[root]
    copies = [i for i in range(nops) if arr[i].kind == COPY]
    block0 = [i for i in range(nops) if arr[i].kind == SEND and arr[i].peer == 0]
    assert len(copies) == 1 and block0 and copies[0] > max(block0)
    units = H.executor_plan(arr, nops, es, bases)
    copy_unit = next(k for k, u in enumerate(units) if u["first"] <= copies[0] < u["first"] + u["num"])
    last_send = next(k for k, u in enumerate(units) if u["first"] <= max(block0) < u["first"] + u["num"])
    assert units[copy_unit]["stream"] == 1 and units[copy_unit]["wait"] == last_send
    assert unordered_conflicts(arr, units, es, bases) == []
    broken = [dict(u) for u in units]
    broken[copy_unit]["wait"] = -1
    assert (last_send, copy_unit) in unordered_conflicts(arr, broken, es, bases)
    # with distinct buffers there is nothing to wait for
    apart = (1 << 40, 2 << 40, 3 << 40)
    assert H.executor_plan(arr, nops, es, apart)[copy_unit]["wait"] == -1
