"""Heads, tails, tiny counts, mixed phases and aliased buffers of the local reduce kernels (HcclAmdLocalReduce2 / N).

The kernels pick their path from two facts (reduce_kernels.hip SplitAligned): the 16-byte phase of the caller's
pointers and the count. Pointers that share a phase get a scalar head (lanes 0.. of block 0), a 16-byte vector body
and a scalar tail (lanes 64.. of block 0); a head longer than the count is clamped; pointers of different phases take
the scalar kernels. Every case here places each operand and the output inside a larger allocation at a chosen element
offset from a 16-byte boundary, fills the output allocation with 0xA5 and checks, after the call,

* the output window bit for bit against the CPU oracle (O.local_reduce / O.reduce_n),
* every other byte of the output allocation (at least 64 bytes on each side) still 0xA5,
* every input allocation unchanged, unless it is the output.

With V = 16 / itemsize and a common phase p (head h = (V - p) % V) the counts sit on the edges the code has: nothing
but a head, the head alone, the first and the last element of the first vector, the longest tail (V - 1 elements),
one tile of the 2-input kernel (256 vectors, unroll 1) and of the n-ary kernel (1024 vectors, unroll 4) each +- 1, and
a count with full tiles, leftover vectors and a tail. A pytest case is one (dtype, op, kernel); its phases and counts
run inside it and a failure names the (phase, count).
"""
import numpy as np
import pytest
import torch

import hccl_amd as H
from oracle import oracle as O
from tests._util import torch_dtype

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes on each side of every window, a multiple of 16
FILL = 0xA5

# MIN stands in for MAX for one dtype of each width, so SUM, MAX and MIN all appear at 1, 2, 4 and 8 bytes
_MIN_DTYPES = (O.INT8, O.BFP16, O.INT32, O.FP64)
DT_OPS = [(dt, op) for dt in O.REDUCE_DTYPES for op in (O.SUM, O.MIN if dt in _MIN_DTYPES else O.MAX)]
KERNELS = [2, 3, 8, 16]  # operands: 2 = HcclAmdLocalReduce2 (k_reduce2), the others HcclAmdLocalReduceN (k_reduceN)


def _ids(v):
    dt, op = v
    return f"{O.DTYPE_NAMES[dt]}-{O.OP_NAMES[op]}"


def _es(dtype):
    return np.dtype(O.NP_STORAGE[dtype]).itemsize


def phases(dtype):
    v = 16 // _es(dtype)
    return sorted({0, 1, v - 1})


def common_counts(dtype, p, nary):
    """The counts of the module docstring for common phase p, positive and without duplicates, in ascending order."""
    v = 16 // _es(dtype)
    h = (v - p) % v
    c = [1, h - 1, h, h + 1, h + v - 1, h + v, h + v + 1, h + 63 * v + (v - 1),
         h + 256 * v - 1, h + 256 * v, h + 256 * v + 1, h + (2 * 256 + 3) * v + 1]
    if nary:
        c += [h + 1024 * v - 1, h + 1024 * v, h + 1024 * v + 1]
    return sorted({x for x in c if x > 0})


def mixed_counts(dtype):
    v = 16 // _es(dtype)
    # 4 * 256 + 1: the first count past the one-block share of the scalar kernels (kBlock * 4 elements per block)
    return sorted({x for x in (1, v - 1, v + 1, 1025, 4 * 256 + 1) if x > 0})


class Placed:
    """`count` elements of `dtype` at element offset `off` from a 16-byte boundary, with GUARD bytes of 0xA5 before the
    boundary and at least GUARD after the window. data = None leaves the window filled with 0xA5 as well."""

    def __init__(self, dtype, off, count, data=None):
        es = _es(dtype)
        self.dtype, self.lo, self.hi = dtype, GUARD + off * es, GUARD + (off + count) * es
        self.host = np.full(self.hi + GUARD + 16, FILL, np.uint8)
        if data is not None:
            self.host[self.lo:self.hi] = np.ascontiguousarray(data).view(np.uint8)
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.win = self.dev[self.lo:self.hi].view(torch_dtype(dtype))

    def bytes_now(self):
        return self.dev.cpu().numpy()

    def unchanged(self):
        return bool(np.array_equal(self.bytes_now(), self.host))

    def check_output(self, want, what, op=None):
        check_window(self.dtype, self.bytes_now(), self.lo, self.hi, want, what, op)


def check_window(dtype, got, lo, hi, want, what, op=None):
    """got = the bytes of a Placed output allocation after the call: the window [lo, hi) equals `want` bit for bit and
    every byte around it still holds the fill. With `op` the comparison is O.equal_bits_select (MAX / MIN byte for
    byte, NaN payloads included), without it O.equal_bits."""
    assert np.all(got[:lo] == FILL), f"{what}: bytes before the output window written"
    assert np.all(got[hi:] == FILL), f"{what}: bytes after the output window written"
    win = got[lo:hi].view(O.NP_STORAGE[dtype])
    same = O.equal_bits(dtype, win, want) if op is None else O.equal_bits_select(dtype, op, win, want)
    assert same, f"{what}: output differs from the oracle"


def run_case(dtype, op, count, offs, seed, alias=None):
    """One call. offs = (out, operand 0, operand 1, ...) element offsets; two operands are (src, dst) of
    HcclAmdLocalReduce2, more are srcs[] of HcclAmdLocalReduceN. alias = the operand whose window is the output."""
    nops = len(offs) - 1
    xs = [O.random_operands(dtype, count, seed=seed + j, edge=True) for j in range(nops)]
    if nops == 2:
        want = O.local_reduce(dtype, op, xs[1].copy(), xs[0])  # out = src (op) dst
    else:
        want = O.reduce_n(dtype, op, xs)
    what = (f"dtype {O.DTYPE_NAMES[dtype]} op {O.OP_NAMES[op]} operands {nops} offsets {offs} count {count} "
            f"alias {alias}")
    ins = [Placed(dtype, offs[1 + j], count, xs[j]) for j in range(nops)]
    out = ins[alias] if alias is not None else Placed(dtype, offs[0], count)
    if nops == 2:
        H.local_reduce2(out.win, ins[0].win, ins[1].win, op)
    else:
        H.local_reduce_n(out.win, [t.win for t in ins], op)
    torch.cuda.synchronize()
    out.check_output(want, what)
    for j, t in enumerate(ins):
        if j != alias:
            assert t.unchanged(), f"{what}: operand {j} (or its guard) written"


@pytest.mark.parametrize("nops", KERNELS)
@pytest.mark.parametrize("dtop", DT_OPS, ids=_ids)
def test_common_phase_edges(dtop, nops):
    """Every pointer at the same phase: head, vector body and tail (k_reduce2 / k_reduceN), at every edge count."""
    dtype, op = dtop
    for p in phases(dtype):
        for count in common_counts(dtype, p, nary=nops > 2):
            run_case(dtype, op, count, (p,) * (nops + 1), seed=3000 + 17 * count + p)


@pytest.mark.parametrize("dtop", DT_OPS, ids=_ids)
def test_mixed_phase_reduce2(dtop):
    """(out, src, dst) at different phases: the whole call runs on k_reduce2_scalar."""
    dtype, op = dtop
    v = 16 // _es(dtype)
    for offs in ((0, 1, 0), (1, 0, 0), (1, 2 % v, 3 % v)):
        assert len(set(offs)) > 1
        for count in mixed_counts(dtype):
            run_case(dtype, op, count, offs, seed=4000 + 17 * count + offs[1])


@pytest.mark.parametrize("nops", [3, 8, 16])
@pytest.mark.parametrize("dtop", DT_OPS, ids=_ids)
def test_mixed_phase_reduce_n(dtop, nops):
    """Only the last source off phase: k_reduceN_scalar."""
    dtype, op = dtop
    for count in mixed_counts(dtype):
        run_case(dtype, op, count, (0,) * nops + (1,), seed=5000 + 17 * count + nops)


def _alias_count(dtype):
    v = 16 // _es(dtype)
    return (v - 1) % v + 256 * v + 1  # common phase 1: h + 256 V + 1 (head, one full 2-input tile, one element more)


@pytest.mark.parametrize("dtop", DT_OPS, ids=_ids)
def test_reduce2_out_aliases_src(dtop):
    """include/hccl_amd.h: "out may alias dst or src" (out == dst is HcclAmdLocalReduce itself)."""
    dtype, op = dtop
    run_case(dtype, op, _alias_count(dtype), (1, 1, 1), seed=6000, alias=0)


@pytest.mark.parametrize("slot", [3, 7])
@pytest.mark.parametrize("dtop", [(O.FP32, O.SUM), (O.INT8, O.SUM), (O.FP32, O.MAX), (O.INT8, O.MIN)], ids=_ids)
def test_reduce_n_out_aliases_a_middle_or_the_last_source(dtop, slot):
    """include/hccl_amd.h: "out may alias any srcs[j]" (srcs[0] is covered in test_gpu_local_reduce.py)."""
    dtype, op = dtop
    run_case(dtype, op, _alias_count(dtype), (1,) * 9, seed=6100 + slot, alias=slot)
