"""The one-sided Scatter's and AllGatherV's launch geometry through HcclAmdIpcPlan (the code RunIpcPlan runs,
ipc_plan.cc), host only: over rounds x workgroups every element of every block is covered exactly once, a round's
piece fits its slot, and for the same alternate area the Scatter's piece is n times the AllGatherV's (one slot per
area against n)."""
import pytest

import hccl_amd as H

SCATTER, AGV = int(H.OpType.SCATTER), int(H.OpType.ALLGATHER_V)
DT = {1: H.HcclDataType.UINT8, 2: H.HcclDataType.FP16, 4: H.HcclDataType.FP32, 8: H.HcclDataType.FP64}
KIND_SCATTER, KIND_AGV = 9, 10


def windows(g, blocks):
    """Piece coordinates [lo, hi) that block b handles, as ForBlockShare deals them (ipc_kernel_body.h)."""
    out = []
    for b in range(blocks):
        if g.tileElems == 0:
            out.append([(b * g.blockElems, (b + 1) * g.blockElems)])
        else:
            step = blocks * g.tileElems
            out.append([(lo, lo + g.tileElems) for lo in range(b * g.tileElems, g.piece, step)])
    return out


def cover(g, blocks, length):
    """How often each element of a block of `length` elements is touched over the launch's rounds and blocks."""
    seen = [0] * length
    for k in range(g.rounds):
        kp = k * g.piece
        part = 0 if kp >= length else min(g.piece, length - kp)
        for wins in windows(g, blocks):
            for lo, hi in wins:
                for e in range(min(lo, part), min(hi, part)):
                    seen[kp + e] += 1
    return seen


AREAS = [(1 << 16, 1 << 16), (1 << 12, 1 << 12)]  # one-round and many-round areas (bytes)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_scatter_covers_every_block_once(n, es):
    for area, alt in AREAS:
        for count in (1, n + 1, 1000, 4099):
            for blocks, tile in ((0, 0), (3, 0), (4, 256)):
                res, launches = H.ipc_plan(SCATTER, n, count, DT[es], family=0, areaBytes=area, altBytes=alt,
                                           blocks=blocks, tileBytes=tile, sharedDevice=1)
                assert res.ll == 0 and len(launches) == 1
                g = launches[0]
                assert g.piece * es <= alt and g.piece % (16 // es) == 0  # the slot is the whole alternate area
                assert g.epochSpan == g.rounds == -(-count // g.piece)
                assert g.blockElems * res.blocks >= g.piece
                assert (g.chunkStride, g.chunkLen, g.total) == (count, count, n * count)
                assert cover(g, res.blocks, count) == [1] * count, (n, es, count, blocks, tile)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_all_gather_v_covers_every_block_once(n, es):
    vectors = [[1000] * n, [(1, 4099, 0, 77, 1000, 3, 2048, 5)[q % 8] for q in range(n)],
               [4099 if q == n - 1 else 0 for q in range(n)]]
    for area, alt in AREAS:
        for counts in vectors:
            displs = [sum(counts[q + 1:]) + 2 * (n - 1 - q) for q in range(n)]  # descending, with gaps
            for blocks, tile in ((0, 0), (3, 0), (4, 256)):
                res, launches = H.ipc_plan(AGV, n, counts[0], DT[es], family=0, counts=counts, displs=displs,
                                           areaBytes=area, altBytes=alt, blocks=blocks, tileBytes=tile, sharedDevice=1)
                assert res.ll == 0 and len(launches) == 1
                g = launches[0]
                assert g.vgeom == 1 and list(g.vLen[:n]) == counts and list(g.vStart[:n]) == displs
                assert n * g.piece * es <= alt and g.piece % (16 // es) == 0  # n slots share the area
                assert g.epochSpan == g.rounds == -(-max(counts) // g.piece)  # from the largest block, known to all
                for q in range(n):
                    assert cover(g, res.blocks, counts[q]) == [1] * counts[q], (n, es, counts, q, blocks, tile)


@pytest.mark.parametrize("n", [2, 3, 8, 16])
def test_scatter_piece_is_n_times_the_all_gather_vs(n):
    """Same area, a count that fills it: one slot per area against n, so n times fewer rounds and barriers."""
    for es in (1, 2, 4, 8):
        alt = n * (1 << 14)
        count = 3 * alt // es
        _, sc = H.ipc_plan(SCATTER, n, count, DT[es], family=0, areaBytes=alt, altBytes=alt)
        _, gv = H.ipc_plan(AGV, n, count, DT[es], family=0, counts=[count] * n, displs=[q * count for q in range(n)],
                           areaBytes=alt, altBytes=alt)
        assert sc[0].piece == n * gv[0].piece == alt // es
        assert gv[0].rounds == n * sc[0].rounds == 3 * n


def test_explicit_plan_and_refusals():
    """The kinds are reachable as explicit plans too (kind 9 with the block layout, kind 10 with the V layout), and a
    kind beyond them is refused."""
    a, _ = H.ipc_plan(SCATTER, 4, 1000, DT[2], family=0)
    b, _ = H.ipc_plan(SCATTER, 4, 1000, DT[2], family=-1, kind=KIND_SCATTER, order=1, geom=3)
    assert (a.blocks, a.altBytes) == (b.blocks, b.altBytes)
    with pytest.raises(Exception):
        H.ipc_plan(SCATTER, 4, 1000, DT[2], family=-1, kind=KIND_AGV + 1, order=1, geom=3)
    with pytest.raises(Exception):
        H.ipc_plan(AGV, 4, 1000, DT[2], family=0)  # the V layout needs the two arrays
