"""The all-to-all family's schedule path and entry checks, host only.

The mesh program (schedule.cc AllToAllMesh; ins_temp_all_to_all_v_mesh_1D.cc) moves data only: a copy of the own block,
then one send and one receive per peer at arbitrary offsets, no staging and no fold. Checked here: the oracle's replay of
the n programs against the numpy permutation on raw bytes; only COPY / SEND / RECV records and no staging; every family
gives the same records; the groups are live under RCCL's rendezvous rule (test_group_liveness.check_live), also when an
explicit piece size makes ranks post different numbers of groups; HcclAlltoAllVC's conversion equals the V form; the entry
checks that need no communicator. (The aliased-buffer conflict check of the Broadcast does not apply: send and receive
buffers are distinct.)
"""
import ctypes
import random

import numpy as np
import pytest

import hccl_amd as H
from oracle import oracle as O
from test_group_liveness import check_live, groups_of

A2A = 6
COPY, SEND, RECV = 0, 2, 3
NP_OF = {O.FP16: np.uint16, O.INT64: np.int64}


def packed(matrix, r):
    """HcclAlltoAllVC's conversion for rank r: (send counts, sdispls, recv counts, rdispls), packed prefix sums."""
    n = len(matrix)
    sc = [matrix[r][q] for q in range(n)]
    rc = [matrix[q][r] for q in range(n)]
    sd = [sum(sc[:q]) for q in range(n)]
    rd = [sum(rc[:q]) for q in range(n)]
    return sc, sd, rc, rd


def gapped(matrix, r, gap):
    """The same counts with `gap + q` unused elements before block q on both sides."""
    sc, sd, rc, rd = packed(matrix, r)
    n = len(matrix)
    sd = [sd[q] + (q + 1) * gap + q * (q - 1) // 2 for q in range(n)]
    rd = [rd[q] + (q + 1) * gap + q * (q - 1) // 2 for q in range(n)]
    return sc, sd, rc, rd


def matrices(n, rng):
    even = [[5] * n for _ in range(n)]
    rnd = [[rng.choice((0, 0, 1, 7, 64, 300)) for _ in range(n)] for _ in range(n)]
    zrow = [[0 if p == n // 2 else 3 + p + q for q in range(n)] for p in range(n)]
    zcol = [[0 if q == n - 1 else 2 + p * q for q in range(n)] for p in range(n)]
    zero = [[0] * n for _ in range(n)]
    return {"even": even, "random": rnd, "zero_row": zrow, "zero_col": zcol, "all_zero": zero}


def programs(matrix, dtype, piece, layout=packed, gap=0):
    n = len(matrix)
    progs = []
    for r in range(n):
        args = layout(matrix, r) if layout is packed else layout(matrix, r, gap)
        arr, nops, scratch = H.build_schedule_alltoall(n, r, *args, dtype, piece)
        assert scratch == 0
        assert all(arr[i].kind in (COPY, SEND, RECV) for i in range(nops))
        progs.append((arr, nops))
    return progs


def replay_and_check(matrix, dtype, piece, seed, gap=0):
    n = len(matrix)
    npdt = NP_OF[dtype]
    rng = np.random.default_rng(seed)
    lay = [gapped(matrix, r, gap) for r in range(n)]
    progs = programs(matrix, dtype, piece, gapped, gap)
    ins, outs, wants = [], [], []
    for r in range(n):
        sc, sd, rc, rd = lay[r]
        in_len = max([sd[q] + sc[q] for q in range(n)] + [1]) + 3
        out_len = max([rd[q] + rc[q] for q in range(n)] + [1]) + 3
        ins.append(rng.integers(0, 256, in_len * np.dtype(npdt).itemsize, dtype=np.uint8).view(npdt))
        outs.append(rng.integers(0, 256, out_len * np.dtype(npdt).itemsize, dtype=np.uint8).view(npdt))
    for r in range(n):
        want = outs[r].copy()  # gaps between the receive regions stay as they were
        _, _, rc, rd = lay[r]
        for q in range(n):
            sq = lay[q][1][r]
            want[rd[q]:rd[q] + rc[q]] = ins[q][sq:sq + matrix[q][r]]
        wants.append(want)
    keep = [x.copy() for x in ins]
    scratch = np.zeros(1, dtype=npdt)
    assert O.replay(n, dtype, O.SUM, progs, [[ins[r], outs[r], scratch] for r in range(n)]) == 0
    for r in range(n):
        assert outs[r].tobytes() == wants[r].tobytes(), (n, dtype, piece, r)
        assert ins[r].tobytes() == keep[r].tobytes(), (n, dtype, piece, r)


@pytest.mark.parametrize("n", range(1, 9))
def test_replay_is_the_permutation(n):
    rng = random.Random(100 + n)
    for name, m in matrices(n, rng).items():
        for dtype in (O.FP16, O.INT64):
            for piece in (0, 128):
                replay_and_check(m, dtype, piece, seed=n * 100 + len(name), gap=0 if name == "even" else 2)


def test_random_sweep():
    rng = random.Random(20241020)
    for draw in range(200):
        n = rng.randint(1, 16)
        m = [[rng.choice((0, 1, rng.randint(0, 40), rng.randint(0, 700))) for _ in range(n)] for _ in range(n)]
        replay_and_check(m, rng.choice((O.FP16, O.INT64)), rng.choice((0, 128, 1024)), seed=draw, gap=rng.randrange(3))


def test_every_family_gives_the_same_records():
    """HcclAmdBuildScheduleAlltoAll takes no family; through BuildSchedule's resolution every family is this schedule,
    and the selector answers it."""
    for n in (2, 8):
        for nbytes in (1, 1 << 20, 1 << 30):
            assert H.select_algo(A2A, n, nbytes) == int(H.Algo.MESH_ONESHOT)
    # the generic export cannot carry the four arrays: it refuses the op instead of building something else
    n_ops = ctypes.c_uint64(0)
    for algo in range(0, 13):
        assert H.lib.HcclAmdBuildSchedule(A2A, algo, 4, 0, 100, O.FP16, 0, 0, None, 0, ctypes.byref(n_ops), None,
                                          None) == H.HcclResult.HCCL_E_PARA
    m = matrices(4, random.Random(1))["random"]
    a = programs(m, O.FP16, 0)
    b = programs(m, O.FP16, 0)
    for (x, nx), (y, ny) in zip(a, b):
        assert nx == ny and bytes(x) == bytes(y)


def test_default_granule_is_one_group_and_zero_counts_post_nothing():
    n = 5
    m = matrices(n, random.Random(3))["zero_row"]
    for r, (arr, nops) in enumerate(programs(m, O.INT64, 0)):
        groups = groups_of(arr, nops)
        sc, _, rc, _ = packed(m, r)
        msgs = sum(1 for q in range(n) if q != r and sc[q]) + sum(1 for q in range(n) if q != r and rc[q])
        assert len(groups) == (1 if msgs else 0)
        assert sum(len(g) for g in groups) == msgs
    for arr, nops in programs(matrices(n, random.Random(3))["all_zero"], O.INT64, 0):
        assert nops == 0


@pytest.mark.parametrize("n", [2, 3, 8])
def test_groups_are_live(n):
    rng = random.Random(7 * n)
    ms = matrices(n, rng)
    skew = [[1] * n for _ in range(n)]
    skew[0][n - 1] = 70001  # rank 0 and rank n-1 post many groups, the others one
    ms["skew"] = skew
    counts = set()
    for name, m in ms.items():
        for piece in (0, 128, 4096):
            progs = [groups_of(*p) for p in programs(m, O.FP16, piece)]
            check_live(progs)
            if name == "skew" and piece == 128:
                counts = {len(g) for g in progs}
    assert len(counts) > 1 or n == 2  # ranks with different group counts were among the checked programs


def test_vc_equals_v_with_the_converted_arrays():
    """Row `rank` = send counts, column `rank` = receive counts, both displacements packed prefix sums
    (ConvertAlltoAllVCParam)."""
    m = [[0, 3, 5], [7, 11, 0], [2, 0, 13]]
    assert packed(m, 1) == ([7, 11, 0], [0, 7, 18], [3, 11, 0], [0, 3, 14])
    assert packed(m, 2) == ([2, 0, 13], [0, 2, 2], [5, 0, 13], [0, 5, 5])


def test_entry_checks_without_a_communicator():
    L, E = H.lib, H.HcclResult
    U8, I8 = H.HcclDataType.UINT8, H.HcclDataType.INT8
    p, p2 = 0x1000, 0x2000  # never dereferenced: every check below returns before the communicator is looked at
    arr = (ctypes.c_uint64 * 4)()
    # HcclAlltoAll
    assert L.HcclAlltoAll(None, 0, U8, None, 0, U8, None, None) == E.HCCL_SUCCESS  # both counts 0 before anything else
    assert L.HcclAlltoAll(p, 8, U8, p2, 8, U8, None, p) == E.HCCL_E_PTR            # comm
    assert L.HcclAlltoAll(None, 8, U8, p2, 8, U8, p, p) == E.HCCL_E_PTR            # sendBuf
    assert L.HcclAlltoAll(p, 8, U8, None, 8, U8, p, p) == E.HCCL_E_PTR             # recvBuf
    assert L.HcclAlltoAll(p, 8, U8, p2, 9, U8, p, p) == E.HCCL_E_PARA              # sendCount != recvCount
    assert L.HcclAlltoAll(p, 0, U8, p2, 9, U8, p, p) == E.HCCL_E_PARA
    assert L.HcclAlltoAll(p, 8, U8, p2, 8, I8, p, p) == E.HCCL_E_PARA              # sendType != recvType
    assert L.HcclAlltoAll(p, 8, U8, p2, 8, U8, p, None) == E.HCCL_E_PTR            # stream
    assert L.HcclAlltoAll(p, 8, U8, p, 8, U8, p, p) == E.HCCL_E_PARA               # in place
    big = (1 << 64) - 1
    assert L.HcclAlltoAll(p, big, H.HcclDataType.FP64, p2, big, H.HcclDataType.FP64, p, p) == E.HCCL_E_PARA  # overflow
    # HcclAlltoAllV
    assert L.HcclAlltoAllV(p, arr, arr, U8, p2, arr, arr, U8, None, p) == E.HCCL_E_PTR   # comm
    for hole in range(4):
        a = [arr, arr, arr, arr]
        a[hole] = None
        assert L.HcclAlltoAllV(p, a[0], a[1], U8, p2, a[2], a[3], U8, p, p) == E.HCCL_E_PTR
    assert L.HcclAlltoAllV(p, arr, arr, U8, p2, arr, arr, U8, p, None) == E.HCCL_E_PTR   # stream
    assert L.HcclAlltoAllV(p, arr, arr, U8, p, arr, arr, U8, p, p) == E.HCCL_E_PARA      # in place
    assert L.HcclAlltoAllV(p, arr, arr, U8, p2, arr, arr, I8, p, p) == E.HCCL_E_PARA     # sendType != recvType
    # HcclAlltoAllVC
    assert L.HcclAlltoAllVC(p, arr, U8, p2, U8, None, p) == E.HCCL_E_PTR                 # comm
    assert L.HcclAlltoAllVC(p, None, U8, p2, U8, p, p) == E.HCCL_E_PTR                   # matrix
    assert L.HcclAlltoAllVC(p, arr, U8, p2, U8, p, None) == E.HCCL_E_PTR                 # stream
    assert L.HcclAlltoAllVC(p, arr, U8, p, U8, p, p) == E.HCCL_E_PARA                    # in place
    assert L.HcclAlltoAllVC(p, arr, U8, p2, I8, p, p) == E.HCCL_E_PARA                   # sendType != recvType
    # the schedule export's own checks
    n_ops = ctypes.c_uint64(0)
    assert L.HcclAmdBuildScheduleAlltoAll(2, 0, arr, arr, arr, None, U8, 0, None, 0, ctypes.byref(n_ops),
                                          None) == E.HCCL_E_PTR
    assert L.HcclAmdBuildScheduleAlltoAll(2, 2, arr, arr, arr, arr, U8, 0, None, 0, ctypes.byref(n_ops),
                                          None) == E.HCCL_E_PARA
    assert len(H.SIGNATURES["HcclAlltoAll"][1]) == 8
    assert len(H.SIGNATURES["HcclAlltoAllV"][1]) == 10
    assert len(H.SIGNATURES["HcclAlltoAllVC"][1]) == 7
    assert len(H.SIGNATURES["HcclAmdBuildScheduleAlltoAll"][1]) == 12
    assert int(H.OpType.ALLTOALL) == A2A
