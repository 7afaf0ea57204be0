"""The one-sided all-to-all's launch geometry through the planner export (HcclAmdIpcPlan, ipc_plan.cc), host only.

AlltoAll and AlltoAllVC (every rank knows the count matrix) are planned from n x (largest entry) x element size like the
other kinds. AlltoAllV's counts are not common knowledge, so nothing in its plan may depend on them: rounds 0 (agreed on
the device), the small staging tier, and workgroups from that tier's capacity.
"""
import pytest

import hccl_amd as H

A2A = int(H.OpType.ALLTOALL)
KIND_A2A, GEOM_WHOLE, AGREED = 8, 4, 1
HEADER_BYTES = 2048  # kIpcA2aHeaderBytes
DT = {1: H.HcclDataType.UINT8, 2: H.HcclDataType.FP16, 4: H.HcclDataType.FP32, 8: H.HcclDataType.INT64}


def known(n, count, es, **kw):
    res, launches = H.ipc_plan(A2A, n, count, DT[es], family=int(H.Algo.AUTO), **kw)
    assert res.numLaunches == 1 and res.ll == 0
    return res, launches[0]


def agreed(n, count, es, **kw):
    res, launches = H.ipc_plan(A2A, n, count, DT[es], family=-1, kind=KIND_A2A, geom=GEOM_WHOLE, subMode=AGREED, **kw)
    assert res.numLaunches == 1 and res.ll == 0
    return res, launches[0]


@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_a_call_that_fits_the_small_tier(monkeypatch, n, es):
    monkeypatch.setenv("HCCL_AMD_SMALL_IPC_BYTES", str(1 << 20))
    V = 16 // es
    for count in (1, n + 1, 1000, 4099):
        res, g = known(n, count, es, sharedDevice=1)
        assert res.altBytes == n << 20  # the small tier: n x HCCL_AMD_SMALL_IPC_BYTES per area
        assert g.piece == -(-count // V) * V and g.rounds == 1 and g.epochSpan == 1
        nbytes = n * count * es  # DefaultIpcBlocks of the call's bytes
        assert res.blocks == (4 if nbytes <= 64 << 10 else 16 if nbytes <= 512 << 10 else 32)
        assert g.blockElems % V == 0 and g.blockElems * res.blocks >= g.piece
        assert n * g.piece * es <= res.altBytes
    # one element more than a small-tier slot holds: the large tier
    res, g = known(n, (1 << 20) // es + 1, es, sharedDevice=1)
    assert res.altBytes > n << 20 and g.rounds == 1


def test_four_rounds_at_a_64_kib_alternate_area():
    """As test_ipc_layout's ReduceScatter case: 2 ranks, fp32, alternate areas of 64 KiB hold two 32 KiB slots."""
    n, es = 2, 4
    res, g = known(n, 4 * 8192 - 5, es, areaBytes=1 << 20, altBytes=64 << 10)
    assert (g.piece, g.rounds, g.epochSpan) == (8192, 4, 4)
    assert g.blockElems * res.blocks >= g.piece and n * g.piece * es <= 64 << 10
    res, g = known(n, 4 * 8192 + 1, es, areaBytes=1 << 20, altBytes=64 << 10)
    assert (g.piece, g.rounds) == (8192, 5)
    # the agreed form's slot gives up the header
    res, g = agreed(n, 123, es, areaBytes=1 << 20, altBytes=64 << 10)
    assert (g.piece, g.rounds, g.epochSpan) == (8192 - HEADER_BYTES // es, 0, 0)
    # an all-zero matrix still runs one round (the ranks meet at its barrier)
    res, g = known(3, 0, 2, sharedDevice=1)
    assert g.rounds == 1 and g.epochSpan == 1 and g.piece == 8


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("es", [1, 2, 8])
def test_the_v_form_does_not_depend_on_the_count(monkeypatch, n, es):
    monkeypatch.setenv("HCCL_AMD_SMALL_IPC_BYTES", str(1 << 20))
    plans = []
    for count in (0, 1, 3_000_000_000):
        res, g = agreed(n, count, es, sharedDevice=1, residentPerRank=96)
        assert g.rounds == 0 and g.epochSpan == 0
        assert res.altBytes == n << 20  # always the small tier
        assert g.piece == (1 << 20) // es - HEADER_BYTES // es
        assert g.blockElems * res.blocks >= g.piece
        plans.append((res.blocks, res.areaBytes, res.altBytes, g.piece, g.blockElems, g.tileElems))
    assert plans[0] == plans[1] == plans[2]
    # the blocks follow the tier's capacity: DefaultIpcBlocks(altBytes), capped by the residency
    assert plans[0][0] == {2: 32, 8: 64}[n]
    # the known form of the same large count takes the large tier and many rounds' worth of geometry instead
    res, g = known(n, 3_000_000_000, es, sharedDevice=1, residentPerRank=96)
    assert res.altBytes != n << 20 and g.rounds > 1


def test_rejections():
    with pytest.raises(H.HcclError):  # the header does not fit the slot
        agreed(16, 1, 1, areaBytes=1 << 20, altBytes=16 << 10)
    with pytest.raises(H.HcclError):  # no such sub-mode
        H.ipc_plan(A2A, 2, 1, DT[1], family=-1, kind=KIND_A2A, geom=GEOM_WHOLE, subMode=2)
