"""ctypes/numpy front end of the CPU oracle (oracle/hccl_oracle.c). TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module, and only as the
checker (or as the timed CPU baseline). The product (hccl_amd / libhccl_amd.so) never imports it.
See hccl_oracle.c for the reference file:line each function restates.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import List, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboracle.so")

# HcclDataType / HcclReduceOp numbering (include/hccl_types.h); kept local so the oracle imports nothing from the
# product package.
INT8, INT16, INT32, FP16, FP32, INT64, UINT64, UINT8, UINT16, UINT32, FP64, BFP16 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
SUM, PROD, MAX, MIN = 0, 1, 2, 3

REDUCE_DTYPES = [INT8, INT16, INT32, INT64, UINT64, FP16, FP32, FP64, BFP16]
OPS = [SUM, PROD, MAX, MIN]
# storage type of each dtype (fp16 / bf16 are kept as raw uint16 bits)
NP_STORAGE = {
    INT8: np.int8, INT16: np.int16, INT32: np.int32, INT64: np.int64, UINT64: np.uint64,
    FP16: np.uint16, BFP16: np.uint16, FP32: np.float32, FP64: np.float64,
}
DTYPE_NAMES = {INT8: "int8", INT16: "int16", INT32: "int32", INT64: "int64", UINT64: "uint64", FP16: "fp16",
               FP32: "fp32", FP64: "fp64", BFP16: "bf16"}
OP_NAMES = {SUM: "sum", PROD: "prod", MAX: "max", MIN: "min"}
FLOAT_DTYPES = {FP16, FP32, FP64, BFP16}


def _ensure_built() -> None:
    src = os.path.join(_HERE, "hccl_oracle.c")
    if not os.path.exists(LIB_PATH) or (os.path.exists(src) and os.path.getmtime(src) > os.path.getmtime(LIB_PATH)):
        subprocess.run(["make", "-C", _HERE], check=True, stdout=subprocess.DEVNULL)


_ensure_built()
_lib = ctypes.CDLL(LIB_PATH)
_vp = ctypes.c_void_p
_lib.orc_fp16_to_fp32.restype = ctypes.c_float
_lib.orc_fp16_to_fp32.argtypes = [ctypes.c_uint16]
_lib.orc_fp32_to_fp16.restype = ctypes.c_uint16
_lib.orc_fp32_to_fp16.argtypes = [ctypes.c_float]
_lib.orc_bf16_to_fp32.restype = ctypes.c_float
_lib.orc_bf16_to_fp32.argtypes = [ctypes.c_uint16]
_lib.orc_fp32_to_bf16.restype = ctypes.c_uint16
_lib.orc_fp32_to_bf16.argtypes = [ctypes.c_float]
for _name in ("orc_aicpu_reduce", "orc_local_reduce"):
    getattr(_lib, _name).restype = ctypes.c_int
    getattr(_lib, _name).argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_uint64]
_lib.orc_reduce_n.restype = ctypes.c_int
_lib.orc_reduce_n.argtypes = [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp), ctypes.c_uint32, ctypes.c_uint64]
_lib.orc_replay.restype = ctypes.c_int
_lib.orc_replay.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp),
                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_vp)]


def _bits_converters(lib, prefix):
    to32, to16 = getattr(lib, prefix + "fp16_to_fp32_bits"), getattr(lib, prefix + "fp32_to_fp16_bits")
    to32.restype = to16.restype = None
    to32.argtypes = [_vp, _vp, ctypes.c_uint64]
    to16.argtypes = [_vp, _vp, ctypes.c_uint64]
    return to32, to16


_orc_to32, _orc_to16 = _bits_converters(_lib, "orc_")

# The reference's own arithmetic, compiled by oracle/Makefile into oracle/_ref/ when the reference tree is there
# (see ref_entry.cc). Optional: only the tests that compare the oracle with it, and the fixture generator, load it.
REF_LIB_PATH = os.path.join(_HERE, "_ref", "libhccl_ref_reduce.so")
_ref = None


def ref_available() -> bool:
    return os.path.exists(REF_LIB_PATH)


def _ref_lib():
    global _ref
    if _ref is None:
        lib = ctypes.CDLL(REF_LIB_PATH)
        lib.ref_reduce.restype = ctypes.c_int
        lib.ref_reduce.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_uint64]
        lib.to32, lib.to16 = _bits_converters(lib, "ref_")
        _ref = lib
    return _ref


def _convert(fn, bits, t_in, t_out) -> np.ndarray:
    a = np.ascontiguousarray(bits, dtype=t_in)
    out = np.empty(a.shape, t_out)
    fn(_p(a), _p(out), a.size)
    return out


def fp16_to_fp32_bits(bits) -> np.ndarray:
    """orc_fp16_to_fp32 over an array of fp16 bit patterns; returns fp32 bit patterns (uint32)."""
    return _convert(_orc_to32, bits, np.uint16, np.uint32)


def fp32_to_fp16_bits(bits) -> np.ndarray:
    """orc_fp32_to_fp16 over an array of fp32 bit patterns (uint32); returns fp16 bit patterns."""
    return _convert(_orc_to16, bits, np.uint32, np.uint16)


def ref_fp16_to_fp32_bits(bits) -> np.ndarray:
    """The reference's Fp16ToFp32 over an array of fp16 bit patterns; returns fp32 bit patterns (uint32)."""
    return _convert(_ref_lib().to32, bits, np.uint16, np.uint32)


def ref_fp32_to_fp16_bits(bits) -> np.ndarray:
    """The reference's Fp32ToFp16 over an array of fp32 bit patterns (uint32); returns fp16 bit patterns."""
    return _convert(_ref_lib().to16, bits, np.uint32, np.uint16)


def ref_reduce(dtype: int, op: int, dst: np.ndarray, src: np.ndarray) -> int:
    """The reference's AicpuReduce: dst = src (op) dst in place. Returns its HcclResult."""
    assert dst.nbytes == src.nbytes
    return _ref_lib().ref_reduce(dtype, op, _p(dst), _p(src), dst.nbytes)


def ref_local_reduce(dtype: int, op: int, dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """dst = src (op) dst in place through the reference's AicpuReduce; returns dst."""
    ret = ref_reduce(dtype, op, dst, src)
    if ret != 0:
        raise RuntimeError(f"the reference's AicpuReduce returned {ret}")
    return dst


def fp16_to_fp32(bits: int) -> float:
    return _lib.orc_fp16_to_fp32(bits)


def fp32_to_fp16(value: float) -> int:
    return _lib.orc_fp32_to_fp16(value)


def bf16_to_fp32(bits: int) -> float:
    return _lib.orc_bf16_to_fp32(bits)


def fp32_to_bf16(value: float) -> int:
    return _lib.orc_fp32_to_bf16(value)


def _p(a: np.ndarray) -> int:
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def aicpu_reduce(dtype: int, op: int, dst: np.ndarray, src: np.ndarray) -> int:
    """AicpuReduce (alg_data_trans_wrapper.cc:1254-1311): dst = src (op) dst in place. Returns the HcclResult."""
    return _lib.orc_aicpu_reduce(dtype, op, _p(dst), _p(src), dst.size)


def local_reduce(dtype: int, op: int, dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """LocalReduce semantics for every reduce dtype: dst = src (op) dst in place; returns dst."""
    assert dst.size == src.size
    ret = _lib.orc_local_reduce(dtype, op, _p(dst), _p(src), dst.size)
    if ret != 0:
        raise RuntimeError(f"orc_local_reduce returned {ret}")
    return dst


def reduce_n(dtype: int, op: int, srcs: Sequence[np.ndarray]) -> np.ndarray:
    """acc = srcs[0]; acc = srcs[j] (op) acc; returns acc (a new array)."""
    out = np.empty_like(srcs[0])
    arr = (_vp * len(srcs))(*[_p(s) for s in srcs])
    ret = _lib.orc_reduce_n(dtype, op, _p(out), arr, len(srcs), out.size)
    if ret != 0:
        raise RuntimeError(f"orc_reduce_n returned {ret}")
    return out


def replay(n_ranks: int, dtype: int, op: int, progs: Sequence, bufs: Sequence[Sequence[np.ndarray]]) -> int:
    """Replay per-rank IR programs (sequence of (ctypes HcclAmdIrOp array, nops)) over host buffers
    bufs[r] = [input, output, scratch]. Returns 0, an HcclResult code, or -1 on deadlock."""
    prog_ptrs = (_vp * n_ranks)(*[ctypes.cast(p[0], _vp) for p in progs])
    nops = (ctypes.c_uint64 * n_ranks)(*[p[1] for p in progs])
    flat: List[int] = []
    for r in range(n_ranks):
        for b in range(3):
            flat.append(_p(bufs[r][b]))
    buf_ptrs = (_vp * (3 * n_ranks))(*flat)
    return _lib.orc_replay(n_ranks, dtype, op, prog_ptrs, nops, buf_ptrs)


def equal_bits(dtype: int, got: np.ndarray, want: np.ndarray) -> bool:
    """Bit equality, except that any NaN matches any NaN (NaN payloads are not canonical across CPU and GPU;
    SURVEY.md §7 'Denormals / NaN')."""
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    if g.shape != w.shape:
        return False
    if dtype in (FP32, FP64):
        gn, wn = np.isnan(g), np.isnan(w)
        return bool(np.array_equal(gn, wn) and np.array_equal(g.view(_uint(g))[~gn], w.view(_uint(w))[~wn]))
    if dtype == FP16:
        gn = ((g & 0x7C00) == 0x7C00) & ((g & 0x03FF) != 0)
        wn = ((w & 0x7C00) == 0x7C00) & ((w & 0x03FF) != 0)
        return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn]))
    if dtype == BFP16:
        gn = ((g & 0x7F80) == 0x7F80) & ((g & 0x007F) != 0)
        wn = ((w & 0x7F80) == 0x7F80) & ((w & 0x007F) != 0)
        return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn]))
    return bool(np.array_equal(g, w))


def _uint(a: np.ndarray):
    return {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.itemsize]


def equal_bits_select(dtype: int, op: int, got: np.ndarray, want: np.ndarray) -> bool:
    """equal_bits for SUM and PROD. MAX and MIN are selects (std::max / std::min return one operand, and the
    reference's fp16 round trip through Fp16ToFp32 / Fp32ToFp16 is the identity on every NaN pattern), so for them
    every byte must be equal: NaN payloads, signalling NaNs and NaN signs included."""
    if op not in (MAX, MIN):
        return equal_bits(dtype, got, want)
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    return bool(g.shape == w.shape and g.itemsize == w.itemsize and np.array_equal(g.view(np.uint8), w.view(np.uint8)))


# (unsigned storage, mantissa bits, exponent field maximum) of the float formats
FLOAT_LAYOUT = {FP16: (np.uint16, 10, 0x1F), BFP16: (np.uint16, 7, 0xFF), FP32: (np.uint32, 23, 0xFF),
                FP64: (np.uint64, 52, 0x7FF)}


def random_bit_patterns(dtype: int, count: int, seed: int) -> np.ndarray:
    """`count` uniform random bit patterns in the dtype's storage type: for floats the exponents span the whole range
    and NaNs and infinities occur as they fall."""
    st = np.dtype(NP_STORAGE[dtype])
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[st.itemsize]
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(u).max, count, dtype=u, endpoint=True).view(st)


def near_operands(dtype: int, src: np.ndarray, seed: int) -> np.ndarray:
    """FP32 / FP64: src's exponent moved by -2 .. +2 (kept inside the field), a fresh random mantissa, the sign flipped
    on half the elements: sums cancel into the subnormal range and overflow at the top."""
    u, mbits, emax = FLOAT_LAYOUT[dtype]
    rng = np.random.default_rng(seed)
    bits = src.view(u).astype(np.uint64)
    exp = ((bits >> np.uint64(mbits)) & np.uint64(emax)).astype(np.int64)
    exp = np.clip(exp + rng.integers(-2, 3, src.size), 0, emax).astype(np.uint64)
    man = rng.integers(0, 1 << mbits, src.size, dtype=np.uint64)
    sign = (bits >> np.uint64(mbits + 11 if dtype == FP64 else mbits + 8)) ^ rng.integers(0, 2, src.size,
                                                                                         dtype=np.uint64)
    out = (sign << np.uint64(63 if dtype == FP64 else 31)) | (exp << np.uint64(mbits)) | man
    return np.ascontiguousarray(out.astype(u).view(NP_STORAGE[dtype]))


def nan_values(dtype: int, seed: int = 0x4E414E) -> np.ndarray:
    """NaN bit patterns of a float dtype, in its storage type: quiet with payload 1, all ones, none (the quiet bit
    alone) and 64 seeded random payloads; signalling with payload 1, all ones and 64 random payloads; each with both
    signs. 266 patterns."""
    u, mbits, emax = FLOAT_LAYOUT[dtype]
    quiet = 1 << (mbits - 1)
    rng = np.random.default_rng(seed + dtype)
    rnd_q = [int(x) for x in rng.integers(1, quiet, 64)]
    rnd_s = [int(x) for x in rng.integers(1, quiet, 64)]
    mant = [quiet | p for p in [1, quiet - 1, 0] + rnd_q] + [1, quiet - 1] + rnd_s
    base = emax << mbits
    sign = 1 << (mbits + emax.bit_length())
    pats = [base | m for m in mant] + [sign | base | m for m in mant]
    return np.array(pats, dtype=u).view(NP_STORAGE[dtype])


def nan_cross(dtype: int):
    """(src, dst): every nan_values pattern against a finite number, +-Inf, +-0, a quiet and a signalling NaN of other
    payloads, once as src and once as dst. Empty for the integer dtypes."""
    st = NP_STORAGE[dtype]
    if dtype not in FLOAT_LAYOUT:
        return np.empty(0, st), np.empty(0, st)
    u, mbits, emax = FLOAT_LAYOUT[dtype]
    base, sign, quiet = emax << mbits, 1 << (mbits + emax.bit_length()), 1 << (mbits - 1)
    finite = sign | ((emax >> 1) + 1) << mbits | (1 << (mbits - 2))  # -2.5
    partners = np.array([finite, base, sign | base, 0, sign, base | quiet | 0x2A, sign | base | 0x15],
                        dtype=u).view(st)
    nans = nan_values(dtype)
    a, b = np.repeat(nans, len(partners)), np.tile(partners, len(nans))
    return np.ascontiguousarray(np.concatenate([a, b])), np.ascontiguousarray(np.concatenate([b, a]))


def random_operands(dtype: int, count: int, seed: int, edge: bool = True, small_ints: bool = False):
    """Seeded operands for parity tests, with the IEEE / integer edge cases the reference's converters and
    std::max/std::min semantics distinguish (±0 ties, NaN, ±Inf, subnormals, max finite, wrap-around)."""
    rng = np.random.default_rng(seed)
    st = NP_STORAGE[dtype]
    if dtype == FP32:
        a = rng.uniform(-1, 1, count).astype(np.float32)
    elif dtype == FP64:
        a = rng.uniform(-1, 1, count)
    elif dtype == FP16:
        a = _fast_fp16(rng, count)
    elif dtype == BFP16:
        f = rng.uniform(-1, 1, count).astype(np.float32)
        a = (f.view(np.uint32) >> 16).astype(np.uint16)
    else:
        info = np.iinfo(st)
        if small_ints:
            lo, hi = max(info.min, -(1 << 20)), min(info.max, 1 << 20)
        else:
            lo, hi = info.min, info.max
        a = rng.integers(lo, hi, count, dtype=st, endpoint=True)
    edges = edge_values(dtype)
    a = np.ascontiguousarray(a.astype(st, copy=False))
    if edge and count >= 2 * len(edges):
        pos = rng.choice(count, size=len(edges), replace=False)
        a[pos] = edges
    return a


def edge_values(dtype: int) -> np.ndarray:
    """The values whose handling differs between plausible implementations of the reference's element rule."""
    st = NP_STORAGE[dtype]
    if dtype == FP32:
        return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.17e-38, 3.4e38, -3.4e38, 1.0],
                        dtype=np.float32)
    if dtype == FP64:
        return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2e-308, 1.7e308, -1.7e308, 1.0])
    if dtype == FP16:  # ±0, ±Inf, qNaN, sNaN, ±min subnormal, max subnormal, min normal, ±max, 1, 65504/2
        return np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF,
                         0xFBFF, 0x3C00, 0x77FF], dtype=np.uint16)
    if dtype == BFP16:
        return np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F,
                         0x3F80], dtype=np.uint16)
    info = np.iinfo(st)
    return np.array([0, 1, info.max, info.min, info.max - 1, info.min + 1], dtype=st)


def edge_cross(dtype: int):
    """(src, dst) covering every ordered pair of edge values: exercises ties, NaN operand order and wrap."""
    e = edge_values(dtype)
    src = np.repeat(e, len(e))
    dst = np.tile(e, len(e))
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


def _fast_fp16(rng, count: int) -> np.ndarray:
    # numpy's float16 cast is IEEE round-to-nearest-even, the same as orc_fp32_to_fp16 for finite normal values
    return rng.uniform(-1, 1, count).astype(np.float32).astype(np.float16).view(np.uint16)
