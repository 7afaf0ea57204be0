"""The host-side plan of the one-sided barrier (HcclAmdIpcPlan for HCCL_AMD_OP_BARRIER; ipc_plan.cc): one launch of
one workgroup per rank with one barrier epoch, no data and no staging tier, whatever family, count or data type the
query names."""
import pytest

import hccl_amd as H
from oracle import oracle as O

LENGTHS = ("total", "chunkStride", "chunkLen", "rem", "group", "piece", "blockElems", "tileElems")


@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("family", [int(H.Algo.AUTO), int(H.Algo.NHR), int(H.Algo.MESH_ONESHOT), int(H.Algo.IPC)])
def test_barrier_plan(n, family):
    res, launches = H.ipc_plan(H.OpType.BARRIER, n, 0, O.INT8, family=family)
    assert (res.blocks, res.ll, res.numLaunches) == (1, 0, 1)
    assert (res.areaBytes, res.altBytes) == (0, 0)  # the call needs no tier
    assert len(launches) == 1
    g = launches[0]
    assert (g.rounds, g.epochSpan, g.ll) == (1, 1, 0)
    assert [getattr(g, f) for f in LENGTHS] == [0] * len(LENGTHS)
    assert (g.balanced, g.vgeom) == (0, 0)
    assert list(g.vStart) == [0] * 16 and list(g.vLen) == [0] * 16


def test_barrier_plan_ignores_count_data_type_and_environment_of_the_call():
    """Neither a count, a data type without a one-sided element size, a loopback world, a block override nor given
    area sizes change the plan."""
    for dtype in (O.INT8, O.FP32, O.FP64, 99):
        res, launches = H.ipc_plan(H.OpType.BARRIER, 4, 1 << 30, dtype, family=int(H.Algo.AUTO), sharedDevice=1,
                                   blocks=64, residentPerRank=3, areaBytes=1 << 20, altBytes=1 << 16)
        assert (res.blocks, res.ll, res.numLaunches, res.areaBytes, res.altBytes) == (1, 0, 1, 0, 0)
        assert (launches[0].rounds, launches[0].epochSpan, launches[0].piece) == (1, 1, 0)


@pytest.mark.parametrize("n", [1, 17])
def test_rank_counts_outside_the_one_sided_path(n):
    with pytest.raises(H.HcclError) as e:
        H.ipc_plan(H.OpType.BARRIER, n, 0, O.INT8, family=int(H.Algo.AUTO))
    assert e.value.code == H.HcclResult.HCCL_E_PARA


def test_the_kind_is_not_an_explicit_plan():
    """Kind 11 is reached through the operator type only: the explicit-plan form keeps refusing what the data kinds'
    planner does not know."""
    with pytest.raises(H.HcclError) as e:
        H.ipc_plan(H.OpType.ALLREDUCE, 4, 1024, O.FP32, family=-1, kind=11, order=0, geom=4)
    assert e.value.code == H.HcclResult.HCCL_E_PARA
