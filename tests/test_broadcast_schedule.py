"""HcclBroadcast's schedule path and entry checks, host only.

The mesh two-shot program (schedule.cc BroadcastTwoShot; ins_temp_broadcast_mesh_1D_two_shot.cc) moves data only, in
place: INPUT and OUTPUT are the caller's one buffer, there is no staging and no fold. Checked here: the oracle's replay
of the n programs delivers the root's bytes to every rank; the groups are live under RCCL's rendezvous rule
(test_group_liveness.check_live); the executor's plan leaves no unordered conflict on the aliased buffer
(the rule of test_executor_hazards, with equal bases for INPUT and OUTPUT); the entry checks that need no communicator.
Equality is on raw bytes throughout: nothing is computed.
"""
import ctypes
import random

import numpy as np
import pytest

import hccl_amd as H
from oracle import oracle as O
from test_executor_hazards import _conflict, _ranges
from test_group_liveness import check_live, groups_of

BCAST = 5
TWOSHOT = 2
SEND, RECV = 2, 3
NP_OF = {O.FP16: np.uint16, O.INT64: np.int64}


def _programs(n, root, count, dtype, piece, algo=0):
    progs = []
    for r in range(n):
        arr, nops, used, scratch = H.build_schedule(BCAST, algo, n, r, count, dtype, root, piece)
        assert used == TWOSHOT
        assert scratch == 0
        assert all(arr[i].kind in (SEND, RECV) for i in range(nops))
        progs.append((arr, nops))
    return progs


def _replay_and_check(n, root, count, dtype, piece, seed):
    progs = _programs(n, root, count, dtype, piece)
    es = np.dtype(NP_OF[dtype]).itemsize
    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, count * es, dtype=np.uint8).view(NP_OF[dtype]) for _ in range(n)]
    want = data[root].copy()
    scratch = np.zeros(1, dtype=NP_OF[dtype])
    bufs = [[data[r], data[r], scratch] for r in range(n)]  # INPUT and OUTPUT are the same array
    assert O.replay(n, dtype, O.SUM, progs, bufs) == 0
    for r in range(n):
        assert data[r].tobytes() == want.tobytes(), (n, root, count, dtype, piece, r)


@pytest.mark.parametrize("n", range(1, 9))
def test_every_rank_gets_the_roots_bytes(n):
    for root in range(n):
        for count in sorted({1, max(1, n - 1), n, n + 1, 1000}):
            for piece in (0, 128):
                for dtype in (O.FP16, O.INT64):
                    _replay_and_check(n, root, count, dtype, piece, seed=n * 1000 + root)


def test_random_sweep():
    rng = random.Random(20240607)
    for draw in range(300):
        n = rng.randint(1, 16)
        _replay_and_check(n, rng.randrange(n), rng.choice((1, max(1, n - 1), n, n + 1, 1000, rng.randint(1, 5000))),
                          rng.choice((O.FP16, O.INT64)), rng.choice((0, 128, 1024)), seed=draw)


def test_selector_and_family_overrides():
    """The selector answers the mesh two-shot, and every schedule family runs that one schedule."""
    for n in (2, 8):
        for nbytes in (1, 1 << 20, 1 << 30):
            assert H.select_algo(BCAST, n, nbytes) == TWOSHOT
    base = _programs(4, 1, 1000, O.FP16, 0)
    for algo in (1, 2, 3, 4, 5, 6, 7, 8, 9):
        got = _programs(4, 1, 1000, O.FP16, 0, algo=algo)
        for (a, na), (b, nb) in zip(base, got):
            assert na == nb and bytes(a) == bytes(b)
    n_ops = ctypes.c_uint64(0)
    assert H.lib.HcclAmdBuildSchedule(BCAST, 0, 4, 0, 100, O.FP16, 4, 0, None, 0, ctypes.byref(n_ops), None,
                                      None) == H.HcclResult.HCCL_E_PARA  # root out of range


@pytest.mark.parametrize("n", [2, 3, 8])
def test_groups_are_live(n):
    for root in (0, n // 2, n - 1):
        for count, piece in [(1, 0), (n - 1, 0), (1000, 128), (65537, 4096), (1 << 20, 0)]:
            progs = [groups_of(*p) for p in _programs(n, root, count, O.FP16, piece)]
            check_live(progs)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_no_unordered_conflict_on_the_aliased_buffer(n):
    """The executor's units of each rank's program with INPUT and OUTPUT at one base: two units on different streams
    that touch the same bytes (one of them writing) are ordered by the plan; and no group receives into bytes that
    another message of the same group reads or writes (one group's messages run concurrently)."""
    es, base = 2, 1 << 40
    bases = (base, base, 3 << 40)
    for root in (0, n // 2, n - 1):
        for count, piece in [(1, 0), (n + 1, 0), (1000, 128), (300001, 4096)]:
            for arr, nops in _programs(n, root, count, O.FP16, piece):
                units = H.executor_plan(arr, nops, es, bases)
                rng = [_ranges(arr, u["first"], u["num"], es, bases) for u in units]
                before, last = [], {0: -1, 1: -1}
                for k, u in enumerate(units):
                    hb = 0
                    for p in (last[u["stream"]], u["wait"]):
                        if p >= 0:
                            hb |= before[p] | (1 << p)
                    before.append(hb)
                    last[u["stream"]] = k
                for b, ub in enumerate(units):
                    for a in range(b):
                        if units[a]["stream"] != ub["stream"] and not (before[b] >> a) & 1:
                            assert not _conflict(rng[a], rng[b]), (n, root, count, piece, a, b)
                    for i, x in enumerate(rng[b]):
                        for y in rng[b][i + 1:]:
                            assert not _conflict([x], [y]), (n, root, count, piece, b)


def test_entry_checks_without_a_communicator():
    L, E = H.lib, H.HcclResult
    U8 = H.HcclDataType.UINT8
    p = 0x1000  # never dereferenced
    assert L.HcclBroadcast(None, 0, U8, 0, None, None) == E.HCCL_SUCCESS  # count 0 before anything else
    assert L.HcclBroadcast(p, 8, U8, 0, None, p) == E.HCCL_E_PTR          # comm
    assert L.HcclBroadcast(None, 8, U8, 0, None, None) == E.HCCL_E_PTR
    assert len(H.SIGNATURES["HcclBroadcast"][1]) == 6
