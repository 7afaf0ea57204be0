"""The element rules of the local reduce kernels over the whole encoding space, against the CPU oracle (GPU).

The other parity tests draw operands from (-1, 1) and add a dozen edge values per dtype, so results in the subnormal
range, overflow on rounding, operands whose exponents are far apart, the bf16 narrowing of fp32-subnormal sums and
products and the fp16 add / mul on subnormal results are hardly met. Here:

* FP16 and BFP16, SUM / PROD / MAX / MIN: src runs over all 65,536 bit patterns, each against 64 partner patterns in
  dst (the dtype's O.edge_values, filled up to 64 with seeded random 16-bit patterns): 4,194,304 elements through
  HcclAmdLocalReduce (the vector body of k_reduce2). A subset of 8 partners (524,288 elements) runs through
  HcclAmdLocalReduce2 with (out, src, dst) at different 16-byte phases (k_reduce2_scalar) and through
  HcclAmdLocalReduceN with a third operand, the partner list rolled by one (k_reduceN, a separate instantiation of the
  same rule).
* FP32 and FP64, every op, 1 << 20 elements each, in two sets: (a) both operands uniform random bit patterns (the
  exponents span the whole range, NaNs and infinities occur as they fall); (b) dst built from src with an exponent
  within +-2, a fresh random mantissa and the sign flipped on half the elements (cancellation into the subnormal range,
  overflow at the top). Each through HcclAmdLocalReduce and through HcclAmdLocalReduceN with 3 operands.
* INT8 SUM over all 65,536 ordered pairs: the packed four-lanes-per-dword add of combine().

Every comparison is O.equal_bits_select against O.local_reduce / O.reduce_n: SUM and PROD bit for bit, any NaN matching
any NaN (their payloads are not canonical across CPU and GPU); MAX and MIN byte for byte, since a select returns one
operand's bits, NaN payloads and signalling NaNs included. No value is left out.
"""
import numpy as np
import pytest
import torch

import hccl_amd as H
from oracle import oracle as O
from tests._util import to_device, to_host
from tests.test_gpu_minmax_roles import diff_report
from tests.test_gpu_reduce_edges import Placed

pytestmark = pytest.mark.gpu

_ids_dt = lambda v: O.DTYPE_NAMES[v]  # noqa: E731
_ids_op = lambda v: O.OP_NAMES[v]  # noqa: E731

PARTNERS = 64
SUBSET = 8


def partners16(dtype):
    """The 64 dst patterns of a 16-bit dtype: its edge values, then seeded random 16-bit patterns."""
    edges = O.edge_values(dtype)
    rng = np.random.default_rng(1600 + dtype)
    fill = rng.integers(0, 1 << 16, PARTNERS - len(edges), dtype=np.uint16)
    return np.concatenate([edges, fill]).astype(np.uint16)


def sweep16(partners):
    """(src, dst): every 16-bit pattern in src, each repeated against every partner."""
    src = np.repeat(np.arange(1 << 16, dtype=np.uint32).astype(np.uint16), len(partners))
    dst = np.tile(partners, 1 << 16)
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


@pytest.fixture(scope="module")
def sweeps():
    """Inputs built once per dtype and shared, unchanged, among the ops."""
    out = {}
    for dtype in (O.FP16, O.BFP16):
        p = partners16(dtype)
        sub = p[::PARTNERS // SUBSET]  # edge values and random patterns alike
        assert len(p) == PARTNERS and len(sub) == SUBSET
        src, dst = sweep16(p)
        s8, d8 = sweep16(sub)
        third = np.ascontiguousarray(np.tile(np.roll(sub, 1), 1 << 16))
        assert src.size == 4194304 and s8.size == 524288
        for a in (src, dst, s8, d8, third):
            a.setflags(write=False)
        out[dtype] = (src, dst, s8, d8, third)
    return out


def expect_equal(dtype, op, got, want, what):
    assert O.equal_bits_select(dtype, op, got, want), f"{what}: {diff_report(dtype, got, want)}"


@pytest.mark.parametrize("op", O.OPS, ids=_ids_op)
@pytest.mark.parametrize("dtype", [O.FP16, O.BFP16], ids=_ids_dt)
def test_16bit_every_pattern_vector_body(sweeps, dtype, op):
    src, dst, _, _, _ = sweeps[dtype]
    want = O.local_reduce(dtype, op, dst.copy(), src)
    d_src, d_dst = to_device(dtype, src), to_device(dtype, dst)
    H.local_reduce(d_dst, d_src, op)
    torch.cuda.synchronize()
    expect_equal(dtype, op, to_host(dtype, d_dst), want, "HcclAmdLocalReduce")


@pytest.mark.parametrize("op", O.OPS, ids=_ids_op)
@pytest.mark.parametrize("dtype", [O.FP16, O.BFP16], ids=_ids_dt)
def test_16bit_every_pattern_scalar_and_nary(sweeps, dtype, op):
    _, _, src, dst, third = sweeps[dtype]
    count = src.size
    want = O.local_reduce(dtype, op, dst.copy(), src)
    out, p_src, p_dst = Placed(dtype, 1, count), Placed(dtype, 2, count, src), Placed(dtype, 3, count, dst)
    H.local_reduce2(out.win, p_src.win, p_dst.win, op)  # three different phases: k_reduce2_scalar
    torch.cuda.synchronize()
    out.check_output(want, "HcclAmdLocalReduce2, mixed phases", op)
    assert p_src.unchanged() and p_dst.unchanged()
    want3 = O.reduce_n(dtype, op, [src, dst, third])
    ds = [to_device(dtype, a) for a in (src, dst, third)]
    out3 = torch.empty_like(ds[0])
    H.local_reduce_n(out3, ds, op)
    torch.cuda.synchronize()
    expect_equal(dtype, op, to_host(dtype, out3), want3, "HcclAmdLocalReduceN, 3 operands")


WIDE_COUNT = 1 << 20


def random_bits(dtype, seed):
    return O.random_bit_patterns(dtype, WIDE_COUNT, seed)


def near(dtype, src, seed):
    """src's exponent moved by -2 .. +2 (kept inside the field), a fresh random mantissa, the sign flipped on half."""
    return O.near_operands(dtype, src, seed)


@pytest.fixture(scope="module")
def wide_sets():
    out = {}
    for dtype in (O.FP32, O.FP64):
        a_src, a_dst, a_third = (random_bits(dtype, 3200 + 10 * dtype + k) for k in range(3))
        b_dst = near(dtype, a_src, 3300 + dtype)
        b_third = near(dtype, b_dst, 3400 + dtype)
        sets = {"random": (a_src, a_dst, a_third), "near": (a_src, b_dst, b_third)}
        for t in sets.values():
            for a in t:
                a.setflags(write=False)
        out[dtype] = sets
    return out


def test_near_set_reaches_the_subnormal_range_and_overflow(wide_sets):
    """What set (b) is for, checked on the oracle (no value is filtered: this only shows the set is not vacuous)."""
    for dtype in (O.FP32, O.FP64):
        src, dst, _ = wide_sets[dtype]["near"]
        tiny = np.finfo(O.NP_STORAGE[dtype]).tiny
        s = O.local_reduce(dtype, O.SUM, dst.copy(), src)
        ok = np.isfinite(src) & np.isfinite(dst)
        assert np.count_nonzero(ok & (s != 0) & (np.abs(s) < tiny)) > 100      # subnormal sums
        assert np.count_nonzero(ok & np.isinf(s)) > 100                        # overflow on rounding
        assert np.count_nonzero(np.signbit(src) != np.signbit(dst)) > WIDE_COUNT // 3         # cancelling pairs


@pytest.mark.parametrize("op", O.OPS, ids=_ids_op)
@pytest.mark.parametrize("which", ["random", "near"])
@pytest.mark.parametrize("dtype", [O.FP32, O.FP64], ids=_ids_dt)
def test_wide_floats_full_range(wide_sets, dtype, which, op):
    src, dst, third = wide_sets[dtype][which]
    want = O.local_reduce(dtype, op, dst.copy(), src)
    d_src, d_dst = to_device(dtype, src), to_device(dtype, dst)
    H.local_reduce(d_dst, d_src, op)
    torch.cuda.synchronize()
    expect_equal(dtype, op, to_host(dtype, d_dst), want, "HcclAmdLocalReduce")
    want3 = O.reduce_n(dtype, op, [src, dst, third])
    ds = [to_device(dtype, a) for a in (src, dst, third)]
    out3 = torch.empty_like(ds[0])
    H.local_reduce_n(out3, ds, op)
    torch.cuda.synchronize()
    expect_equal(dtype, op, to_host(dtype, out3), want3, "HcclAmdLocalReduceN, 3 operands")


def test_int8_sum_every_pair():
    v = np.arange(256, dtype=np.uint8).view(np.int8)
    src, dst = np.ascontiguousarray(np.repeat(v, 256)), np.ascontiguousarray(np.tile(v, 256))
    want = O.local_reduce(O.INT8, O.SUM, dst.copy(), src)
    d_src, d_dst = to_device(O.INT8, src), to_device(O.INT8, dst)
    H.local_reduce(d_dst, d_src, O.SUM)
    torch.cuda.synchronize()
    expect_equal(O.INT8, O.SUM, to_host(O.INT8, d_dst), want, "HcclAmdLocalReduce int8 sum")
