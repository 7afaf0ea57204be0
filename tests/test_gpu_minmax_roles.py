"""Which operand is src and which is dst, under MAX and MIN, on every path that folds (GPU).

The element rule is dst = src (op) dst with std::max / std::min semantics: +0 against -0 and a NaN on either side both
return src. Floating-point SUM and PROD commute bit for bit and ordinary data hides roles and association under MAX and
MIN, so only ties and NaNs that meet at one element index on different ranks pin them. tests/role_operands.py puts every
ordered pair of ranks, in each of three kinds ((+0, -0), (NaN, +0), (NaN, -0)), into every period of P = 3 n (n - 1)
elements; every other rank holds the op's loser. Each case asserts, before it runs, that every chunk (and, for the
MeshChunk families, every sub-slice) its family cuts holds a whole period, so every pair meets in every fold the family
performs. Outputs are compared with O.equal_bits_select (MAX and MIN: every byte equal, a NaN's payload included)
against the oracle: its n-ary fold, its replay of the schedule IR (for the one-sided kernel: of the twin schedule), or
the AIV closed forms of tests/sched_ref.py.
tests/test_role_operands.py (CPU) shows that the data has teeth and that the IR replay and the closed forms agree on it.

What a swapped `combine(x, acc)` would do. The kernels compute acc = combine(x_i, acc): x_i is src. Written the other
way round, acc = combine(acc, x_i), a (+0, -0) pair on ranks (a, b) returns the zero of whichever rank is folded first
instead of last, and a NaN on the rank folded first survives a finite later operand instead of being replaced by it.
The (+0, -0) elements alone therefore change in every fold of two or more operands, whatever its order: on the CPU,
tests/test_role_operands.py::test_swapped_roles_change_every_expectation restates every closed form with the two roles
exchanged and finds each family's expectation changed in every whole period of every output. Since the data also
changes the oracle's result under any exchange of two operands (::test_data_has_teeth), a wrong OperandRank shows too.
The role slot each path exposes:

* local n-ary folds (k_reduceN, k_reduceN_scalar; k_reduceN_batch_rows, k_reduceN_batch): the chain acc = x_i (op) acc,
  vector body, head / tail lanes and the scalar kernel separately; out aliasing srcs[0];
* executor schedules: every REDUCE record's operand order, as the generators emit it, over LaunchReduceN: the O1 / O2
  chains (families 1, 2), the ring's travelling partial as src (3), RHD's partner as src (4), NHR's sender as src (5),
  TreeFoldN's later block as src with M changing at n = 3, 5 (6), O6's rotation per sub-slice (8);
* staged one-sided kernel: FoldSeg's chain in OperandRank order O1 / O2 / O6 (families 7 and 9, AllReduce,
  ReduceScatter, Reduce), RhdFold's relabelled tree (12);
* LL form: the same folds over the unpack area's slot layout;
* AIV engine: O2 (one-shot, small-core two-shot, ReduceScatter big-data), O1 over group x n balanced slices (large-core
  two-shot), TreeStep's "later partial is src" (ReduceScatter local tree, O4);
* rank mode: family 9 with each rank in a process of its own (every rank folds from its own mappings).

HCCL_DETERMINISTIC=STRICT selects the order-preserved tree for SUM and PROD only (ops.cc NeedStrictOrder), and family
9 follows the auto selector's size rule whatever the mode: the one-sided kernel never gets O4 from family 9, so the
STRICT case here asserts that MAX / MIN keep the one-shot order O1. O4 on the one-sided kernel runs as the AIV local
tree.
"""
import datetime
import multiprocessing as mp
import os
import time
import traceback

import numpy as np
import pytest
import torch

import hccl_amd as H
from oracle import oracle as O
from tests import sched_ref as R
from tests._util import to_device, to_host, torch_dtype
from tests.role_operands import period, role_operands
from tests.test_gpu_collectives import AR, RED, RS, _ipc_twin, aiv_expected, collective, oracle_replay
from tests.test_gpu_fold_batch import _FLAT, _ROWS3, _layout
from tests.test_gpu_ipc_edges import _free_port
from tests.test_gpu_rccl import _ir
from tests.test_gpu_reduce_edges import Placed

pytestmark = pytest.mark.gpu

ROLE_OPS = (O.MAX, O.MIN)
EXTRA_DTYPES = (O.FP16, O.BFP16, O.FP64)
LL_BYTES = 64 << 10
SMALL_BYTES = 1 << 20
PIECE_BYTES = 32 << 10
TWOSHOT, AUTO9, AIV, RHD12 = int(H.Algo.IPC_TWOSHOT), int(H.Algo.IPC), int(H.Algo.AIV), int(H.Algo.IPC_RHD)
KIND_NAMES = {AR: "allreduce", RS: "reducescatter", RED: "reduce"}


def role_count(n):
    """The smallest counts of the issue: a whole period in every chunk and sub-slice, 4099 // 12 = 341 >= 36 and
    20011 // 56 = 357 >= 168."""
    return 4099 if n <= 4 else 20011


def _es(dtype):
    return np.dtype(O.NP_STORAGE[dtype]).itemsize


def assert_periods(n, count, parts):
    """Every one of the `parts` pieces a family cuts `count` elements into holds a whole period."""
    assert count // parts >= period(n), (n, count, parts, period(n))


def diff_report(dtype, got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.shape != w.shape:
        return f"shapes {g.shape} / {w.shape}"
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[g.itemsize]
    bad = np.flatnonzero(g.view(u) != w.view(u))
    return (f"{len(bad)} of {g.size} elements differ bitwise (NaN payloads included), first {bad[:6].tolist()}: got "
            f"{g.view(u)[bad[:6]].tolist()} want {w.view(u)[bad[:6]].tolist()}")


def check_outputs(what, kind, n, dtype, op, root, outs, want):
    for r in range(n):
        if kind == RED and r != root:
            assert not outs[r].any(), f"{what}: non-root rank {r} output written"
            continue
        assert O.equal_bits_select(dtype, op, outs[r], want[r]), f"{what} rank {r}: {diff_report(dtype, outs[r], want[r])}"


def role_inputs(kind, dtype, op, n, count, shift):
    return role_operands(dtype, op, n, count * n if kind == RS else count, shift)


# ------------------------------------------------------------------------------------------------ case tables
# (also read by tests/test_role_operands.py, which compares the two CPU models on exactly these cases)

# test_dtypes_ops' (operation, family) list; families 7 and 9 are the one-sided kernel and sit in STAGED_CASES
SCHED_PAIRS = [(AR, 1), (AR, 2), (AR, 3), (AR, 4), (AR, 5), (AR, 6), (AR, 8), (RS, 1), (RS, 5), (RS, 6), (RS, 8),
               (RED, 2), (RED, 5)]


def _dtype_n(algo):
    return 4 if algo in (R.ALGO_RHD, RHD12) else 3  # RHD needs a power of two


def sched_cases():
    """(operation, family, n, dtype): every pair at n = 4 and 3 in FP32, the other dtypes at one n, and the tree at
    every n from 2 to 8."""
    out = []
    for kind, algo in SCHED_PAIRS:
        out += [(kind, algo, n, O.FP32) for n in (4, 3)]
        out += [(kind, algo, _dtype_n(algo), dt) for dt in EXTRA_DTYPES]
    for n in (2, 5, 6, 7, 8):
        out += [(kind, R.ALGO_TREE, n, O.FP32) for kind in (AR, RS)]
    return out


def staged_cases():
    """(operation, family, n, dtype, count, twin family or None, strict)."""
    out = []
    for n in (2, 3, 4, 8):
        for fam in (TWOSHOT, AUTO9):
            out += [(kind, fam, n, O.FP32, role_count(n), None, 0) for kind in (AR, RS, RED)]
    out += [(AR, RHD12, n, O.FP32, role_count(n), R.ALGO_RHD, 0) for n in (2, 4, 8)]
    for dt in EXTRA_DTYPES:
        for fam in (TWOSHOT, AUTO9):
            out += [(kind, fam, 3, dt, role_count(3), None, 0) for kind in (AR, RS, RED)]
        out.append((AR, RHD12, 4, dt, role_count(4), R.ALGO_RHD, 0))
    # family 9 in each order the auto selector hands it (sizes of test_ipc_follows_auto_family at the default
    # HCCL_BUFFSIZE): O1 one-shot, O2 two-shot (> 8 MiB), O6 MeshChunk (AllReduce bytes * 8 / n^2 > 32 MiB,
    # ReduceScatter bytes * (8 / n)^2 > 16 MiB), and STRICT, which leaves MAX / MIN on O1
    out.append((AR, AUTO9, 4, O.FP32, 4099, R.ALGO_ONESHOT, 0))
    out.append((AR, AUTO9, 8, O.FP32, (9 << 20) // 4 + 3, R.ALGO_TWOSHOT, 0))
    out.append((AR, AUTO9, 3, O.FP32, (40 << 20) // 4 + 1, R.ALGO_MESHCHUNK, 0))
    out.append((RS, AUTO9, 4, O.FP32, (5 << 20) // 4 + 7, R.ALGO_MESHCHUNK, 0))
    out.append((AR, AUTO9, 4, O.FP32, 4099, R.ALGO_ONESHOT, 1))
    return out


def ll_count(kind, n):
    if kind == AR:
        return 4099 if n <= 4 else 8191
    return 4099 if n <= 4 else 2047  # n = 8: the whole input of 8 blocks within 64 KiB


def ll_cases():
    """(operation, family asked for, family that runs, n, dtype, count)."""
    pairs = [(AR, int(H.Algo.AUTO), AUTO9), (AR, int(H.Algo.RHD), RHD12), (RS, int(H.Algo.AUTO), AUTO9)]
    out = []
    for kind, ask, fam in pairs:
        out += [(kind, ask, fam, n, O.FP32, ll_count(kind, n)) for n in (2, 3, 4, 8) if fam != RHD12 or n != 3]
        out += [(kind, ask, fam, _dtype_n(fam), dt, ll_count(kind, 4)) for dt in EXTRA_DTYPES]
    return out


def aiv_cases():
    """(operation, n, dtype, count, core limit, variant): the core limits of AIV_CASES (tests/test_gpu_collectives.py)
    per variant; counts: role_count(n) where the variant is the small-data one, otherwise 3 elements past the variant's
    byte threshold (128 KiB per rank for the two-shot AllReduces, 512 KiB of output for the big-data ReduceScatter).
    FP32 at several n per variant, FP16 and BFP16 at n = 4; the engine has no FP64."""
    out = []
    for dt in (O.FP32, O.FP16, O.BFP16):
        two, big = (128 << 10) // _es(dt) + 3, (512 << 10) // _es(dt) + 3
        rows = [(AR, 2, role_count(2), 48, R.AIV_AR_ONESHOT), (AR, 4, role_count(4), 48, R.AIV_AR_ONESHOT),
                (AR, 8, role_count(8), 48, R.AIV_AR_ONESHOT),
                (AR, 4, two, 48, R.AIV_AR_TWOSHOT_LARGE), (AR, 8, two, 48, R.AIV_AR_TWOSHOT_LARGE),
                (AR, 3, two, 56, R.AIV_AR_TWOSHOT_LARGE),
                (AR, 4, two, 8, R.AIV_AR_TWOSHOT_SMALL), (AR, 8, two, 9, R.AIV_AR_TWOSHOT_SMALL),
                (AR, 8, two, 4, R.AIV_AR_TWOSHOT_SMALL),
                (RS, 4, role_count(4), 48, R.AIV_RS_LOCAL_TREE), (RS, 8, role_count(8), 48, R.AIV_RS_LOCAL_TREE),
                (RS, 3, role_count(3), 6, R.AIV_RS_LOCAL_TREE), (RS, 8, big, 16, R.AIV_RS_LOCAL_TREE),
                (RS, 4, big, 48, R.AIV_RS_BIGDATA), (RS, 2, big, 48, R.AIV_RS_BIGDATA),
                (RS, 8, big, 48, R.AIV_RS_BIGDATA)]
        seen = set()
        for kind, n, count, limit, variant in rows:
            if dt != O.FP32 and (n != 4 or variant in seen):
                continue
            seen.add(variant)
            out.append((kind, n, dt, count, limit, variant))
    return out


def twin_of(kind, fam, n, count, dtype, op):
    return _ipc_twin(kind, fam, n, count, dtype, op)


def _name(kind, fam, n, dtype, op, extra=""):
    return f"{KIND_NAMES[kind]}-f{fam}-n{n}-{O.DTYPE_NAMES[dtype]}-{O.OP_NAMES[op]}{extra}"


KIND_IDS = {AR: "ar", RS: "rs", RED: "red"}


def _params(cases, ident):
    """(case index, case) parameters: the index is the case's shift; MAX and MIN both run inside the case."""
    return [pytest.param(i, c, id=ident(c)) for i, c in enumerate(cases)]


def _fam_id(kind, fam, n, dtype):
    return f"{KIND_IDS[kind]}-f{fam}-n{n}-{O.DTYPE_NAMES[dtype]}"


# ------------------------------------------------------------------------------------------------ worlds

@pytest.fixture(scope="module")
def role_worlds():
    cache = {}

    def get(n, small=0, ll=0, core_limit=48, strict=0):
        if n not in cache:
            cache[n] = H.loopback_world(n)
            for c in cache[n]:
                c.set_config(H.Config.IPC_TIMEOUT_MS, 20000)  # a stuck barrier fails the test, never hangs the box
        for c in cache[n]:
            c.set_config(H.Config.SMALL_IPC_BYTES, small)
            c.set_config(H.Config.IPC_LL_BYTES, ll)
            c.set_config(H.Config.AIV_CORE_LIMIT, core_limit)
            c.set_config(H.Config.DETERMINISTIC_STRICT, strict)
        return cache[n]

    yield get
    torch.cuda.synchronize()
    for comms in cache.values():
        for c in comms:
            c.destroy()


# ------------------------------------------------------------------------------------------------ local folds

LOCAL_COUNT = 3 * 4096 + 3  # fp32: three tiles of the n-ary kernel (1024 vectors each) and a tail


@pytest.mark.parametrize("dtype", [O.FP32, O.FP16, O.BFP16, O.FP64], ids=lambda v: O.DTYPE_NAMES[v])
@pytest.mark.parametrize("nsrc", [2, 3, 4, 7, 8, 16])
def test_local_reduce_n_roles(nsrc, dtype):
    for op in ROLE_OPS:
        _local_reduce_n_roles(nsrc, dtype, op)


def _local_reduce_n_roles(nsrc, dtype, op):
    """HcclAmdLocalReduceN: aligned (vector body and tail), common phase 1 (head lanes too), the output one element
    off the operands' phase (k_reduceN_scalar), and out aliasing srcs[0]."""
    count = LOCAL_COUNT
    assert_periods(nsrc, count, 3)  # every tile of the vector body holds a whole period
    for k, (out_off, src_off, alias) in enumerate([(0, 0, None), (1, 1, None), (1, 0, None), (0, 0, 0)]):
        what = f"{nsrc} operands {O.DTYPE_NAMES[dtype]} {O.OP_NAMES[op]} out +{out_off} srcs +{src_off} alias {alias}"
        xs = role_operands(dtype, op, nsrc, count, shift=4 * nsrc + k)
        want = O.reduce_n(dtype, op, xs)
        ins = [Placed(dtype, src_off, count, x) for x in xs]
        out = ins[alias] if alias is not None else Placed(dtype, out_off, count)
        H.local_reduce_n(out.win, [t.win for t in ins], op)
        torch.cuda.synchronize()
        out.check_output(want, what, op)
        for j, t in enumerate(ins):
            if j != alias:
                assert t.unchanged(), f"{what}: operand {j} (or its guard) written"


@pytest.mark.parametrize("name,segs", [("rows3", _ROWS3), ("flat3", _FLAT)], ids=["rows3", "flat3"])
def test_batched_fold_roles(role_worlds, name, segs):
    for op in ROLE_OPS:
        _batched_fold_roles(role_worlds, name, segs, op)


def _batched_fold_roles(role_worlds, name, segs, op):
    """LaunchReduceNBatch (k_reduceN_batch_rows; k_reduceN_batch for the flat shapes of tests/test_gpu_fold_batch.py):
    fold-only IR programs through HcclAmdCommExecute, 3 FP32 operands per segment."""
    dtype, nsrc = O.FP32, 3
    comm = role_worlds(2)[0]
    plan, in_len, out_len = _layout(nsrc, segs, None, 16 // _es(dtype))
    host_in = np.zeros(in_len, np.float32)
    for g, (count, srcs, _) in enumerate(plan):
        assert_periods(nsrc, count, 1)
        for s, x in zip(srcs, role_operands(dtype, op, nsrc, count, shift=g + 1)):
            host_in[s:s + count] = x
    dev_in = to_device(dtype, host_in)
    prog = [_ir(H.IrKind.REDUCE, count, dst=(1, d), srcs=[(0, s) for s in srcs]) for count, srcs, d in plan]
    arr = (H.HcclAmdIrOp * len(prog))(*prog)
    out = torch.empty(out_len, dtype=torch_dtype(dtype), device="cuda")
    out.view(torch.uint8).fill_(0xA5)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    comm.execute(arr, len(prog), dev_in, out, op, False, stream)
    torch.cuda.synchronize()
    got = to_host(dtype, out)
    untouched = np.ones(out_len, dtype=bool)
    for g, (count, srcs, d) in enumerate(plan):
        want = O.reduce_n(dtype, op, [host_in[s:s + count] for s in srcs])
        assert O.equal_bits_select(dtype, op, got[d:d + count], want), f"{name} segment {g}: " \
            f"{diff_report(dtype, got[d:d + count], want)}"
        untouched[d:d + count] = False
    assert np.all(got[untouched].view(np.uint8) == 0xA5), f"{name}: bytes outside the segments' windows written"


# ------------------------------------------------------------------------------------------------ executor schedules

@pytest.mark.parametrize("idx,case", _params(sched_cases(), lambda c: _fam_id(*c)))
def test_executor_schedule_roles(role_worlds, idx, case):
    for op in ROLE_OPS:
        _executor_schedule_roles(role_worlds, idx, case, op)


def _executor_schedule_roles(role_worlds, idx, case, op):
    kind, algo, n, dtype = case
    count, root = role_count(n), n - 1
    assert_periods(n, count, n * (n - 1))
    what = _name(kind, algo, n, dtype, op)
    comms = role_worlds(n)
    xs = role_inputs(kind, dtype, op, n, count, idx)
    want_algo = H.build_schedule(kind, algo, n, 0, count, dtype, root, PIECE_BYTES)[2]
    used, outs = collective(comms, kind, algo, dtype, op, xs, count, root=root, piece_bytes=PIECE_BYTES)
    assert used == want_algo, f"{what}: ran {H.Algo(used).name}"
    want = oracle_replay(kind, algo, n, count, dtype, op, xs, root, PIECE_BYTES)
    check_outputs(what, kind, n, dtype, op, root, outs, want)


# ------------------------------------------------------------------------------------------------ one-sided kernel

@pytest.mark.parametrize("idx,case", _params(staged_cases(), lambda c: f"{_fam_id(*c[:4])}-c{c[4]}-s{c[6]}"))
def test_staged_kernel_roles(role_worlds, idx, case):
    for op in ROLE_OPS:
        _staged_kernel_roles(role_worlds, idx, case, op)


def _staged_kernel_roles(role_worlds, idx, case, op):
    """HCCL_AMD_IPC_LL_BYTES = 0 and HCCL_AMD_SMALL_IPC_BYTES = 0: the staged kernel."""
    kind, fam, n, dtype, count, twin_want, strict = case
    root = n - 1
    what = _name(kind, fam, n, dtype, op, f" count {count} strict {strict}")
    twin = twin_of(kind, fam, n, count, dtype, op)
    if twin_want is not None:
        assert twin == twin_want, f"{what}: twin family {twin}"
    assert_periods(n, count, n * (n - 1) if twin == R.ALGO_MESHCHUNK or count == role_count(n) else n)
    comms = role_worlds(n, strict=strict)
    xs = role_inputs(kind, dtype, op, n, count, 100 + idx)
    before = comms[0].ipc_ll_launches()
    used, outs = collective(comms, kind, fam, dtype, op, xs, count, root=root)
    assert used == fam, f"{what}: ran {H.Algo(used).name}"
    assert comms[0].ipc_status() & 1 == 0, f"{what}: barrier timeout"
    assert comms[0].ipc_ll_launches() == before, f"{what}: an LL launch"
    want = oracle_replay(kind, twin, n, count, dtype, op, xs, root, 0)
    check_outputs(what, kind, n, dtype, op, root, outs, want)


@pytest.mark.parametrize("idx,case", _params(ll_cases(), lambda c: f"{_fam_id(c[0], c[2], c[3], c[4])}-c{c[5]}"))
def test_ll_form_roles(role_worlds, idx, case):
    for op in ROLE_OPS:
        _ll_form_roles(role_worlds, idx, case, op)


def _ll_form_roles(role_worlds, idx, case, op):
    """Default thresholds (small-call rule 1 MiB, LL form up to 64 KiB): exactly one LL launch per call."""
    kind, ask, fam, n, dtype, count = case
    what = _name(kind, fam, n, dtype, op, f" count {count} (LL)")
    assert_periods(n, count, n)  # the LL form cuts block windows only: whole-range folds, one block each for an RS
    comms = role_worlds(n, small=SMALL_BYTES, ll=LL_BYTES)
    xs = role_inputs(kind, dtype, op, n, count, 300 + idx)
    before = comms[0].ipc_ll_launches()
    used, outs = collective(comms, kind, ask, dtype, op, xs, count)
    assert used == fam, f"{what}: ran {H.Algo(used).name}"
    assert comms[0].ipc_status() & 1 == 0, f"{what}: barrier timeout"
    assert comms[0].ipc_ll_launches() - before == 1, f"{what}: {comms[0].ipc_ll_launches() - before} LL launches"
    want = oracle_replay(kind, twin_of(kind, fam, n, count, dtype, op), n, count, dtype, op, xs, 0, 0)
    check_outputs(what, kind, n, dtype, op, 0, outs, want)


@pytest.mark.parametrize("idx,case", _params(aiv_cases(), lambda c: f"{_fam_id(c[0], 'aiv', c[1], c[2])}-c{c[3]}-l{c[4]}-v{c[5]}"))
def test_aiv_engine_roles(role_worlds, idx, case):
    for op in ROLE_OPS:
        _aiv_engine_roles(role_worlds, idx, case, op)


def _aiv_engine_roles(role_worlds, idx, case, op):
    kind, n, dtype, count, core_limit, variant_want = case
    what = _name(kind, "aiv", n, dtype, op, f" count {count} core limit {core_limit}")
    comms = role_worlds(n, core_limit=core_limit)
    xs = role_inputs(kind, dtype, op, n, count, 500 + idx)
    variant, want = aiv_expected(kind, dtype, op, xs, count, n, core_limit)
    assert variant == variant_want, f"{what}: closed form selects variant {variant}"
    got_variant, group = H.select_aiv_algo(kind, n, count, dtype, op, core_limit)
    assert int(got_variant) == variant_want, f"{what}: the library selects {got_variant!r}"
    assert_periods(n, count, group * n)
    before = comms[0].ipc_ll_launches()
    used, outs = collective(comms, kind, AIV, dtype, op, xs, count)
    assert used == AIV, f"{what}: ran {H.Algo(used).name}"
    assert comms[0].ipc_status() & 1 == 0, f"{what}: barrier timeout"
    assert comms[0].ipc_ll_launches() == before, f"{what}: an LL launch"
    check_outputs(what, kind, n, dtype, op, 0, outs, want)


# ------------------------------------------------------------------------------------------------ rank mode

RANK_N, RANK_COUNT = 2, 4099


def _rank_cases():
    return [(kind, ll, dtype, op) for kind in (AR, RS) for ll in (False, True) for dtype in (O.FP32, O.BFP16)
            for op in ROLE_OPS]


def _rank_inputs(i, case):
    kind, _, dtype, op = case
    return role_inputs(kind, dtype, op, RANK_N, RANK_COUNT, 700 + i)


def _rank_main(rank, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"  # a lost peer shows as a status bit, never a hang
    try:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=RANK_N,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)

        def all_gather(b):
            out = [None] * RANK_N
            dist.all_gather_object(out, b)
            return out

        comm = H.comm_init_host_exchange(RANK_N, rank, all_gather)
        comm.set_algo(AUTO9)
        stream = torch.cuda.Stream()
        results = []
        for i, case in enumerate(_rank_cases()):
            kind, ll, dtype, op = case
            comm.set_config(H.Config.IPC_LL_BYTES, LL_BYTES if ll else 0)
            send = to_device(dtype, _rank_inputs(i, case)[rank])
            recv = to_device(dtype, np.zeros(RANK_COUNT, O.NP_STORAGE[dtype]))
            torch.cuda.synchronize()
            before = comm.ipc_ll_launches()
            if kind == AR:
                comm.all_reduce(send, recv, op, stream=stream)
            else:
                comm.reduce_scatter(send, recv, op, stream=stream)
            stream.synchronize()
            status = comm.ipc_status()
            results.append((status, comm.last_algo, comm.ipc_ll_launches() - before, to_host(dtype, recv)))
            if max(all_gather(status & 1)) != 0:  # every rank stops together after a barrier timeout anywhere
                break
        dist.barrier()
        comm.destroy()  # collective: no rank unmaps while a peer's kernel may still store into it
        dist.destroy_process_group()
        q.put((rank, "ok", results))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)  # failure only: peers' kernels are bounded, let them drain before this process's memory goes


def test_rank_mode_roles():
    """Two processes on the one GPU, family 9 staged and in the LL form, AllReduce and ReduceScatter, FP32 and BFP16,
    MAX and MIN, 4099 elements."""
    cases = _rank_cases()
    assert_periods(RANK_N, RANK_COUNT, RANK_N * (RANK_N - 1))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, port, q)) for r in range(RANK_N)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in procs:
            rank, msg, res = q.get(timeout=300)
            got[rank] = (msg, res)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(RANK_N):
        assert got[r][0] == "ok", f"rank {r}:\n{got[r][0]}"
        assert len(got[r][1]) == len(cases), f"rank {r} stopped after case {len(got[r][1]) - 1}"
    for i, case in enumerate(cases):
        kind, ll, dtype, op = case
        xs = _rank_inputs(i, case)
        twin = twin_of(kind, AUTO9, RANK_N, RANK_COUNT, dtype, op)
        want = oracle_replay(kind, twin, RANK_N, RANK_COUNT, dtype, op, xs, 0, 0)
        for r in range(RANK_N):
            what = f"rank {r} {_name(kind, AUTO9, RANK_N, dtype, op)} ll {ll}"
            status, algo, ll_launches, out = got[r][1][i]
            assert status & 1 == 0, f"{what}: barrier timeout (status {status:#x})"
            assert algo == AUTO9, f"{what}: ran {algo}"
            assert ll_launches == (1 if ll else 0), f"{what}: {ll_launches} LL launches"
            assert O.equal_bits_select(dtype, op, out, want[r]), f"{what}: {diff_report(dtype, out, want[r])}"
