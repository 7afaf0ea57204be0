"""Kernels against the reference's own recorded results, without the oracle in between (GPU).

tests/golden/ref_local_reduce.npz was written by the reference's AicpuReduce, compiled (tests/golden/make_ref_golden.py):
every ordered pair of edge values, quiet and signalling NaNs of both signs against finite numbers, infinities, zeros and
other NaNs in both roles, random bit patterns, and ordered folds of eight such operands. Every comparison here is
O.equal_bits_select: SUM and PROD bit for bit with any NaN matching any NaN, MAX and MIN byte for byte, so a MAX / MIN
result must carry the selected operand's exact bits, a signalling NaN's included. A converting move that quiets a
NaN, a hardware max / min in place of the select, or a canonicalising copy would fail here and nowhere else.

* HcclAmdLocalReduce2, seven dtypes x four ops: every pointer 16-byte aligned; every pointer one element past a
  boundary (head and tail lanes fall on other elements); the output one element off the sources' phase (the scalar
  kernel).
* HcclAmdLocalReduceN at 2, 3, 4, 7 and 8 operands against the recorded chain acc = in_j (op) acc, FP16, FP32, FP64
  and INT32, aligned and shifted by one element.
* The one-sided kernel in a 2-rank loopback world, where one application of the rule is the whole result: family 9
  staged (HCCL_AMD_IPC_LL_BYTES = 0) and in the LL form, AllReduce, MAX and MIN, FP16, FP32 and FP64.
  Direction, as tests/test_gpu_minmax_roles.py pins it: at this size family 9 follows the one-shot order O1, rank r
  computes acc = x_r; acc = x_peer (op) acc, so the peer's buffer is src and the rank's own is dst. Each case runs
  twice with the fixture's src and dst exchanged between the ranks, so each rank's output is once the recorded
  dst = src (op) dst. (Were the twin the two-shot order O2, both ranks compute x_1 (op) x_0; the test handles both and
  asserts which one it is.)
* The executor's one-shot family (1) at n = 2 through the fold kernel, MAX and MIN, FP32 and FP16; same direction.
* BFP16 MAX / MIN and INT16, which the reference routes nowhere: the same placements against the oracle, under
  equal_bits_select. Their ids say "unpinned by the reference".
"""
import os

import numpy as np
import pytest
import torch

import hccl_amd as H
from oracle import oracle as O
from tests import sched_ref as R
from tests.test_gpu_collectives import AR, _ipc_twin, collective
from tests.test_gpu_minmax_roles import diff_report
from tests.test_gpu_reduce_edges import FILL, Placed

pytestmark = pytest.mark.gpu

ROUTED = [O.INT8, O.INT32, O.FP16, O.FP32, O.INT64, O.UINT64, O.FP64]
CHAIN_STEPS = (2, 3, 4, 7, 8)
SELECT_OPS = (O.MAX, O.MIN)
LL_BYTES, SMALL_BYTES = 64 << 10, 1 << 20
AUTO9 = int(H.Algo.IPC)

_ids_dt = lambda v: O.DTYPE_NAMES[v]  # noqa: E731
_ids_op = lambda v: O.OP_NAMES[v]  # noqa: E731


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_local_reduce.npz"),
                allow_pickle=False)
    return {k: z[k] for k in z.files}


def check_placed(out, dtype, op, want, what):
    """The output window equals `want` under equal_bits_select and every byte around it still holds the fill."""
    got = out.bytes_now()
    assert np.all(got[:out.lo] == FILL), f"{what}: bytes before the output window written"
    assert np.all(got[out.hi:] == FILL), f"{what}: bytes after the output window written"
    win = got[out.lo:out.hi].view(O.NP_STORAGE[dtype])
    assert O.equal_bits_select(dtype, op, win, want), f"{what}: {diff_report(dtype, win, want)}"


# (out, src, dst) element offsets from a 16-byte boundary
REDUCE2_PLACEMENTS = [("aligned", (0, 0, 0)), ("all +1", (1, 1, 1)), ("out +1 (scalar kernel)", (1, 0, 0))]


def reduce2_placements(dtype, op, src, dst, want, label):
    for name, (o_off, s_off, d_off) in REDUCE2_PLACEMENTS:
        what = f"HcclAmdLocalReduce2 {O.DTYPE_NAMES[dtype]} {O.OP_NAMES[op]} {name} ({label})"
        out, p_src, p_dst = Placed(dtype, o_off, src.size), Placed(dtype, s_off, src.size, src), \
            Placed(dtype, d_off, src.size, dst)
        H.local_reduce2(out.win, p_src.win, p_dst.win, op)
        torch.cuda.synchronize()
        check_placed(out, dtype, op, want, what)
        assert p_src.unchanged() and p_dst.unchanged(), f"{what}: an operand (or its guard) written"


@pytest.mark.parametrize("op", O.OPS, ids=_ids_op)
@pytest.mark.parametrize("dtype", ROUTED, ids=_ids_dt)
def test_local_reduce2_recorded(golden, dtype, op):
    name = O.DTYPE_NAMES[dtype]
    reduce2_placements(dtype, op, golden[f"{name}_src"], golden[f"{name}_dst"], golden[f"{name}_{O.OP_NAMES[op]}"],
                       "recorded reference")


@pytest.mark.parametrize("op", O.OPS, ids=_ids_op)
@pytest.mark.parametrize("dtype", [O.FP16, O.FP32, O.FP64, O.INT32], ids=_ids_dt)
def test_local_reduce_n_recorded_chain(golden, dtype, op):
    name = O.DTYPE_NAMES[dtype]
    srcs = [golden[f"{name}_chain_in{j}"] for j in range(8)]
    for k in CHAIN_STEPS:
        want = golden[f"{name}_chain_{O.OP_NAMES[op]}_{k}"]
        for off in (0, 1):
            what = f"HcclAmdLocalReduceN {name} {O.OP_NAMES[op]} {k} operands, every pointer +{off}"
            ins = [Placed(dtype, off, want.size, x) for x in srcs[:k]]
            out = Placed(dtype, off, want.size)
            H.local_reduce_n(out.win, [t.win for t in ins], op)
            torch.cuda.synchronize()
            check_placed(out, dtype, op, want, what)
            assert all(t.unchanged() for t in ins), f"{what}: an operand (or its guard) written"


# ------------------------------------------------------------------------------------------------ 2-rank worlds

@pytest.fixture(scope="module")
def world2():
    comms = H.loopback_world(2)
    for c in comms:
        c.set_config(H.Config.IPC_TIMEOUT_MS, 20000)  # a stuck barrier fails the test, never hangs the box

    def get(small, ll):
        for c in comms:
            c.set_config(H.Config.SMALL_IPC_BYTES, small)
            c.set_config(H.Config.IPC_LL_BYTES, ll)
        return comms

    yield get
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()


def roles_of(order, rank):
    """(rank whose buffer is src, rank whose buffer is dst) of rank `rank`'s one fold at n = 2."""
    if order == R.ALGO_ONESHOT:  # O1: acc = x_me; acc = x_peer (op) acc
        return 1 - rank, rank
    assert order == R.ALGO_TWOSHOT, f"no direction known for order {order}"  # O2: acc = x_0; acc = x_1 (op) acc
    return 1, 0


def two_rank_case(comms, ask, order, dtype, op, src, dst, want, what, after_call):
    """Both assignments of the fixture's (src, dst) to the two ranks; a rank's output is compared whenever its fold has
    the fixture's roles. after_call(what) asserts the family and the launch counters of one call."""
    checked = set()
    for xs in ([dst, src], [src, dst]):
        used, outs = collective(comms, AR, ask, dtype, op, xs, src.size)
        after_call(used)
        for rank in range(2):
            s, d = roles_of(order, rank)
            if xs[s] is src and xs[d] is dst:
                assert O.equal_bits_select(dtype, op, outs[rank], want), \
                    f"{what} rank {rank}: {diff_report(dtype, outs[rank], want)}"
                checked.add(rank)
    assert checked == {0, 1}, f"{what}: ranks compared {sorted(checked)}"


@pytest.mark.parametrize("dtype", [O.FP16, O.FP32, O.FP64], ids=_ids_dt)
@pytest.mark.parametrize("ll", [False, True], ids=["staged", "ll"])
def test_one_sided_kernel_recorded(world2, golden, ll, dtype):
    name = O.DTYPE_NAMES[dtype]
    src, dst = golden[f"{name}_src"], golden[f"{name}_dst"]
    comms = world2(SMALL_BYTES, LL_BYTES) if ll else world2(0, 0)
    ask = int(H.Algo.AUTO) if ll else AUTO9
    for op in SELECT_OPS:
        what = f"one-sided {'LL' if ll else 'staged'} {name} {O.OP_NAMES[op]}"
        order = _ipc_twin(AR, AUTO9, 2, src.size, dtype, op)
        assert order == R.ALGO_ONESHOT, f"{what}: family 9 follows order {order} at this size"
        before = [comms[0].ipc_ll_launches()]

        def after_call(used):
            assert used == AUTO9, f"{what}: ran {H.Algo(used).name}"
            assert comms[0].ipc_status() & 1 == 0, f"{what}: barrier timeout"
            now = comms[0].ipc_ll_launches()
            assert now - before[0] == (1 if ll else 0), f"{what}: {now - before[0]} LL launches"
            before[0] = now

        two_rank_case(comms, ask, order, dtype, op, src, dst, golden[f"{name}_{O.OP_NAMES[op]}"], what, after_call)


@pytest.mark.parametrize("dtype", [O.FP32, O.FP16], ids=_ids_dt)
def test_executor_one_shot_recorded(world2, golden, dtype):
    name = O.DTYPE_NAMES[dtype]
    src, dst = golden[f"{name}_src"], golden[f"{name}_dst"]
    comms = world2(0, 0)
    want_algo = H.build_schedule(AR, R.ALGO_ONESHOT, 2, 0, src.size, dtype, 0, 0)[2]
    assert want_algo == R.ALGO_ONESHOT
    for op in SELECT_OPS:
        what = f"executor one-shot {name} {O.OP_NAMES[op]}"
        before = comms[0].ipc_ll_launches()

        def after_call(used):
            assert used == R.ALGO_ONESHOT, f"{what}: ran {H.Algo(used).name}"
            assert comms[0].ipc_ll_launches() == before, f"{what}: an LL launch"

        two_rank_case(comms, R.ALGO_ONESHOT, R.ALGO_ONESHOT, dtype, op, src, dst, golden[f"{name}_{O.OP_NAMES[op]}"],
                      what, after_call)


# ------------------------------------------------------------------------------------------------ unrouted dtypes

UNPINNED = [(O.BFP16, O.MAX), (O.BFP16, O.MIN)] + [(O.INT16, op) for op in O.OPS]


def unpinned_operands(dtype):
    es, ed = O.edge_cross(dtype)
    ns, nd = O.nan_cross(dtype)
    fill = 4099 - es.size - ns.size
    rs, rd = (O.random_bit_patterns(dtype, fill, 0x0B160000 + 2 * dtype + k) for k in range(2))
    return np.ascontiguousarray(np.concatenate([es, ns, rs])), np.ascontiguousarray(np.concatenate([ed, nd, rd]))


@pytest.mark.parametrize("dtop", UNPINNED,
                         ids=lambda v: f"{O.DTYPE_NAMES[v[0]]}-{O.OP_NAMES[v[1]]}-unpinned by the reference")
def test_local_reduce2_unrouted_dtypes_against_the_oracle(dtop):
    dtype, op = dtop
    src, dst = unpinned_operands(dtype)
    assert src.size == 4099
    want = O.local_reduce(dtype, op, dst.copy(), src)
    reduce2_placements(dtype, op, src, dst, want, "oracle; unpinned by the reference")
