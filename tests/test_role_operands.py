"""The role operands of tests/role_operands.py on the CPU: the data has teeth, and the two CPU models that serve as
the GPU's references in tests/test_gpu_minmax_roles.py agree on it.

* Exchanging any two operands of the oracle's n-ary fold changes at least 6 elements of every whole period.
* The closed forms of tests/sched_ref.py and the oracle's replay of the schedule IR (H.build_schedule) give the same
  bits on role data for every (operation, family) the GPU module runs, at n = 2 .. 8 and at its counts. The AIV engine
  has no IR of its own: its closed forms are compared with the IR of the schedule whose order each variant follows
  (two-shot AllReduce for O2, the one-shot AllReduce's rank c output on the slices rank c owns for the large-core
  two-shot's O1, the order-preserved ReduceScatter for the local tree).
* With the two roles exchanged in the closed forms (dst (op) src for src (op) dst), every family's expectation changes
  in every whole period of every output: a kernel whose combine() took its operands the other way round could not give
  the bits the GPU module expects.
"""
import numpy as np
import pytest

import hccl_amd as H
from oracle import oracle as O
from tests import sched_ref as R
from tests.role_operands import period, role_operands
from tests.test_gpu_collectives import AR, RED, RS, oracle_replay
from tests.test_gpu_minmax_roles import (EXTRA_DTYPES, PIECE_BYTES, ROLE_OPS, SCHED_PAIRS, aiv_cases, ll_cases,
                                         role_count, role_inputs, sched_cases, staged_cases, twin_of)

FLOATS = [O.FP32, O.FP16, O.BFP16, O.FP64]
_ids_dt = lambda v: O.DTYPE_NAMES[v]  # noqa: E731
_ids_op = lambda v: O.OP_NAMES[v]  # noqa: E731


def differ(dtype, a, b):
    """Element mask: bits differ, any NaN matching any NaN (O.equal_bits' rule, per element)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if dtype in (O.FP32, O.FP64):
        an, bn = np.isnan(a), np.isnan(b)
        u = np.uint32 if dtype == O.FP32 else np.uint64
    else:
        exp, man = (0x7C00, 0x03FF) if dtype == O.FP16 else (0x7F80, 0x007F)
        an, bn = ((a & exp) == exp) & ((a & man) != 0), ((b & exp) == exp) & ((b & man) != 0)
        u = np.uint16
    return (an != bn) | (~an & ~bn & (a.view(u) != b.view(u)))


def per_period(mask, p):
    """Changed elements in each whole period of p elements."""
    whole = mask.size // p
    return mask[:whole * p].reshape(whole, p).sum(axis=1)


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids_dt)
@pytest.mark.parametrize("op", ROLE_OPS, ids=_ids_op)
@pytest.mark.parametrize("n", [2, 3, 4, 8, 16])
def test_data_has_teeth(n, op, dtype):
    """A condition on the data alone: any transposition of two operands of O.reduce_n changes at least 6 elements of
    every whole period (the pair's own two orderings in three kinds)."""
    p = period(n)
    xs = role_operands(dtype, op, n, 2 * p)
    base = O.reduce_n(dtype, op, xs)
    for a in range(n):
        for b in range(a + 1, n):
            ys = list(xs)
            ys[a], ys[b] = xs[b], xs[a]
            changed = per_period(differ(dtype, O.reduce_n(dtype, op, ys), base), p)
            assert len(changed) == 2 and changed.min() >= 6, (a, b, changed.tolist())


def test_layout_is_the_specified_one():
    """Element e of rank r, for n = 3 and a shift: pairs in lexicographic order, three kinds per pair, the loser
    elsewhere; explicit bit patterns for the 16-bit formats."""
    n, shift = 3, 5
    pairs = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for dtype, (pz, nz, nan, m1, p1) in ((O.FP16, (0x0000, 0x8000, 0x7E00, 0xBC00, 0x3C00)),
                                         (O.BFP16, (0x0000, 0x8000, 0x7FC0, 0xBF80, 0x3F80))):
        kinds = [(pz, nz), (nan, pz), (nan, nz)]
        for op, loser in ((O.MAX, m1), (O.MIN, p1)):
            xs = role_operands(dtype, op, n, 40, shift)
            for e in range(40):
                q = (e + shift) % 18
                a, b = pairs[q // 3]
                want = {a: kinds[q % 3][0], b: kinds[q % 3][1]}
                assert [int(xs[r][e]) for r in range(n)] == [want.get(r, loser) for r in range(n)], (dtype, op, e)
    x32 = role_operands(O.FP32, O.MAX, 2, 6)
    assert x32[0].view(np.uint32).tolist()[:3] == [0x00000000, 0x7FC00000, 0x7FC00000]
    assert x32[1].view(np.uint32).tolist()[:3] == [0x80000000, 0x00000000, 0x80000000]


@pytest.mark.parametrize("dtype", [O.INT8, O.INT32, O.INT64], ids=_ids_dt)
def test_integers_have_no_roles(dtype):
    """Integer ties are bit-identical, so no order of the operands can show under MAX / MIN: nothing is generated for
    them, and the oracle's fold of integer data is the same under every rotation of its operands."""
    with pytest.raises(AssertionError):
        role_operands(dtype, O.MAX, 3, 100)
    xs = [O.random_operands(dtype, 4099, seed=40 + r, small_ints=True) for r in range(4)]
    for r in range(4):
        xs[r][::7] = xs[0][::7]  # ties
    for op in ROLE_OPS:
        base = O.reduce_n(dtype, op, xs)
        for k in range(1, 4):
            assert np.array_equal(O.reduce_n(dtype, op, xs[k:] + xs[:k]), base)


# ------------------------------------------------------------------------------------------------ the two CPU models

def closed_form(kind, algo, n, count, dtype, op, xs, root):
    used = H.build_schedule(kind, algo, n, 0, count, dtype, root, 0)[2]
    return R.expected(kind, used, dtype, op, xs, count, root=root)


def assert_models_agree(kind, algo, n, count, dtype, op, shift, piece_bytes=0):
    root = n - 1
    xs = role_inputs(kind, dtype, op, n, count, shift)
    ir = oracle_replay(kind, algo, n, count, dtype, op, xs, root, piece_bytes)
    cf = closed_form(kind, algo, n, count, dtype, op, xs, root)
    for r in range(n):
        if kind == RED and r != root:
            assert not ir[r].any()
            continue
        assert O.equal_bits(dtype, ir[r], cf[r]), (kind, algo, n, count, dtype, op, r)


@pytest.mark.parametrize("op", ROLE_OPS, ids=_ids_op)
@pytest.mark.parametrize("n", range(2, 9))
@pytest.mark.parametrize("kind,algo", SCHED_PAIRS + [(RS, 3), (RED, 1)])
def test_ir_replay_and_closed_forms_agree_fp32(kind, algo, n, op):
    """Families 1-8 (what family 4 and the Reduce families resolve to at this n included), every n, the GPU module's
    count for that n; (RED, 1) is the twin of family 9's small Reduce, (RS, 3) the ring's ReduceScatter."""
    assert_models_agree(kind, algo, n, role_count(n), O.FP32, op, shift=n + algo, piece_bytes=PIECE_BYTES)


@pytest.mark.parametrize("op", ROLE_OPS, ids=_ids_op)
@pytest.mark.parametrize("case", [c for c in sched_cases() if c[3] in EXTRA_DTYPES],
                         ids=lambda c: f"{c[0]}-f{c[1]}-n{c[2]}-{O.DTYPE_NAMES[c[3]]}")
def test_ir_replay_and_closed_forms_agree_other_dtypes(case, op):
    kind, algo, n, dtype = case
    assert_models_agree(kind, algo, n, role_count(n), dtype, op, shift=3, piece_bytes=PIECE_BYTES)


def _twin_cases():
    """(operation, twin family, n, dtype, count) of every one-sided case of the GPU module, both ops' twins merged."""
    out = set()
    for op in ROLE_OPS:
        for kind, fam, n, dtype, count, _, _ in staged_cases():
            out.add((kind, twin_of(kind, fam, n, count, dtype, op), n, dtype, count))
        for kind, _, fam, n, dtype, count in ll_cases():
            out.add((kind, twin_of(kind, fam, n, count, dtype, op), n, dtype, count))
    return sorted(out)


@pytest.mark.parametrize("op", ROLE_OPS, ids=_ids_op)
@pytest.mark.parametrize("case", _twin_cases(), ids=lambda c: f"{c[0]}-f{c[1]}-n{c[2]}-{O.DTYPE_NAMES[c[3]]}-c{c[4]}")
def test_one_sided_twins_agree(case, op):
    """The twin schedules of the staged and LL cases, at their own counts (the 9 MiB two-shot and the MeshChunk sizes
    included)."""
    kind, twin, n, dtype, count = case
    assert_models_agree(kind, twin, n, count, dtype, op, shift=n)


def aiv_by_ir(kind, variant, group, n, count, dtype, op, xs):
    """The AIV variant's order from schedule IR: see the module docstring."""
    if kind == AR and variant in (R.AIV_AR_ONESHOT, R.AIV_AR_TWOSHOT_SMALL):
        return oracle_replay(AR, R.ALGO_TWOSHOT, n, count, dtype, op, xs, 0, 0)
    if kind == AR:
        o1 = oracle_replay(AR, R.ALGO_ONESHOT, n, count, dtype, op, xs, 0, 0)
        out = np.empty_like(xs[0])
        for off, cnt in R.ref_loops(count, xs[0].itemsize, R.UB_MAX_DATA_SIZE, 4, R.ccl_bytes_from_env()):
            sl = R.balanced_bounds(cnt, group * n)
            for c in range(n):
                b, e = off + sl[c * group][0], off + sl[(c + 1) * group - 1][1]
                out[b:e] = o1[c][b:e]
        return [out] * n
    if variant == R.AIV_RS_LOCAL_TREE:
        return oracle_replay(RS, R.ALGO_TREE, n, count, dtype, op, xs, 0, 0)
    full = oracle_replay(AR, R.ALGO_TWOSHOT, n, count * n, dtype, op, xs, 0, 0)
    return [full[me][me * count:(me + 1) * count] for me in range(n)]


@pytest.mark.parametrize("op", ROLE_OPS, ids=_ids_op)
@pytest.mark.parametrize("case", aiv_cases(),
                         ids=lambda c: f"{c[0]}-n{c[1]}-{O.DTYPE_NAMES[c[2]]}-c{c[3]}-l{c[4]}-v{c[5]}")
def test_aiv_closed_forms_agree_with_ir_orders(case, op):
    kind, n, dtype, count, core_limit, variant_want = case
    xs = role_inputs(kind, dtype, op, n, count, shift=7)
    variant, group = R.aiv_select(kind, n, count, xs[0].itemsize, False, False, core_limit=core_limit)
    assert variant == variant_want
    got_variant, got_group = H.select_aiv_algo(kind, n, count, dtype, op, core_limit)
    assert (int(got_variant), got_group) == (variant, group)
    cf = R.allreduce_aiv(dtype, op, xs, variant, group) if kind == AR \
        else R.reduce_scatter_aiv(dtype, op, xs, count, variant)
    ir = aiv_by_ir(kind, variant, group, n, count, dtype, op, xs)
    for r in range(n):
        assert O.equal_bits(dtype, cf[r], ir[r]), (case, op, r)


# ------------------------------------------------------------------------------------------------ a swapped combine

def _swapped_fold(dtype, op, arrays):
    """R.fold with the roles exchanged: acc = acc (op) x_j, the accumulator as src."""
    acc = np.ascontiguousarray(arrays[0]).copy()
    for x in arrays[1:]:
        acc = O.local_reduce(dtype, op, np.ascontiguousarray(x).copy(), acc)
    return acc


def _swapped_apply(dtype, op, src, dst):
    return O.local_reduce(dtype, op, np.ascontiguousarray(src).copy(), np.ascontiguousarray(dst))


@pytest.mark.parametrize("op", ROLE_OPS, ids=_ids_op)
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_swapped_roles_change_every_expectation(monkeypatch, n, op):
    """Every closed form the GPU module's references rest on, restated with combine's operands exchanged: each
    output's every whole period changes in at least its n (n - 1) tie elements (the (+0, -0) pair returns the other
    zero wherever the two meet, whatever the order and whatever was folded in between)."""
    dtype, count, root, p = O.FP32, role_count(n), n - 1, period(n)
    forms = [(kind, algo) for kind, algo in SCHED_PAIRS + [(RS, 3), (RED, 1)]]
    aiv = [(AR, R.AIV_AR_ONESHOT, 1), (AR, R.AIV_AR_TWOSHOT_LARGE, 2), (RS, R.AIV_RS_BIGDATA, 1),
           (RS, R.AIV_RS_LOCAL_TREE, 1)]

    def every():
        out = {}
        for kind, algo in forms:
            xs = role_inputs(kind, dtype, op, n, count, 0)
            out[(kind, algo)] = [w for w in closed_form(kind, algo, n, count, dtype, op, xs, root) if w is not None]
        for kind, variant, group in aiv:
            xs = role_inputs(kind, dtype, op, n, count, 0)
            out[("aiv", kind, variant)] = R.allreduce_aiv(dtype, op, xs, variant, group) if kind == AR \
                else R.reduce_scatter_aiv(dtype, op, xs, count, variant)
        return out

    right = every()
    monkeypatch.setattr(R, "fold", _swapped_fold)
    monkeypatch.setattr(R, "apply", _swapped_apply)
    wrong = every()
    for key, outs in right.items():
        for r, want in enumerate(outs):
            changed = per_period(differ(dtype, wrong[key][r], want), p)
            assert len(changed) >= 1 and changed.min() >= n * (n - 1), (key, r, changed.min())
