"""The CPU oracle (oracle/hccl_oracle.c) against the reference's own arithmetic, compiled (CPU only).

oracle/Makefile cuts Fp16ToFp32, Fp32DenormToFp16, Fp32ToFp16, AicpuReduceFp16, AicpuReduce and AicpuReduceTemplate<T>
out of the reference's alg_data_trans_wrapper.cc and compiles them, unchanged, behind oracle/ref_shim.h into
oracle/_ref/libhccl_ref_reduce.so, with the oracle's flags. Every case here runs the same arrays through both libraries.
All values cross the boundary as bit patterns in arrays, so signalling NaNs are compared too.

Comparison (O.equal_bits_select): MAX and MIN byte for byte; SUM and PROD bit for bit wherever the reference's result is
not a NaN, and a NaN exactly where the reference's is. SUM / PROD payloads are left out because x86's add and mul return
the first operand's payload when both are NaNs, and two compilers (or two builds of one) may commute the operands of
`src + dst`: which payload survives is the compiler's choice, not the reference's rule.

Needs oracle/_ref/: without the library and without the reference tree the module skips; without the library while
the tree is there it fails (the build was not run). The fixture tests at the end that need no library always run.

Measured: the whole file takes 10 s on one CPU core (the fp32 -> fp16 subnormal sweep, 2 x 12 x 2^23 patterns, 2.8 s;
the four fp16 element-rule cases, 2 x 17.7 M elements each, 5 s).

Teeth, tried once on scratch copies of the oracle: exchanging src and dst in its MAX fails 5 tests here (the fp16, fp32
and fp64 MAX element rule and both fixture tests); dropping "NaN mantissa 0 becomes 1" from its fp32 -> fp16 converter
fails 2 (the guard / sticky / LSB sweep and the random patterns).
"""
import os

import numpy as np
import pytest

from oracle import oracle as O

HCCL_E_INTERNAL = 4
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
ROUTED = [O.INT8, O.INT32, O.FP16, O.FP32, O.INT64, O.UINT64, O.FP64]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_local_reduce.npz")
CHAIN_STEPS = (2, 3, 4, 7, 8)

_ids_dt = lambda v: O.DTYPE_NAMES[v]  # noqa: E731
_ids_op = lambda v: O.OP_NAMES[v]  # noqa: E731


@pytest.fixture(scope="module")
def ref():
    if not O.ref_available():
        if os.path.isdir(REFERENCE):
            pytest.fail(f"{O.REF_LIB_PATH} is missing although {REFERENCE} is there: run `make -C oracle`")
        pytest.skip("no compiled reference (oracle/_ref/) and no reference tree to build it from")
    return O


def first_diffs(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[g.itemsize]
    bad = np.flatnonzero(g.view(u) != w.view(u))
    return (f"{len(bad)} of {g.size} differ bitwise, first at {bad[:4].tolist()}: oracle "
            f"{[hex(x) for x in g.view(u)[bad[:4]].tolist()]} reference {[hex(x) for x in w.view(u)[bad[:4]].tolist()]}")


def assert_same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {g.dtype}{g.shape} / {w.dtype}{w.shape}"
    assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: {first_diffs(g, w)}"


# ----------------------------------------------------------------------------------------------- converters

def test_fp16_to_fp32_every_pattern(ref):
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    assert_same_bits(O.fp16_to_fp32_bits(bits), O.ref_fp16_to_fp32_bits(bits), "Fp16ToFp32")


def test_fp32_to_fp16_guard_sticky_lsb(ref):
    """Upper 19 bits: all 2^19 values; low 13 bits: 0, 1, 0xFFF, 0x1000, 0x1001, 0x1FFF."""
    hi = np.arange(1 << 19, dtype=np.uint32) << np.uint32(13)
    for low in (0, 1, 0xFFF, 0x1000, 0x1001, 0x1FFF):
        bits = hi | np.uint32(low)
        assert_same_bits(O.fp32_to_fp16_bits(bits), O.ref_fp32_to_fp16_bits(bits), f"Fp32ToFp16, low bits {low:#x}")


@pytest.mark.parametrize("sign", [0, 1], ids=["positive", "negative"])
def test_fp32_to_fp16_subnormal_path_every_mantissa(ref, sign):
    """Exponent fields 0x66 .. 0x71 (fp16 exponent -11 .. 0: Fp32DenormToFp16 and its flush threshold), all 2^23
    mantissas each: the shift moves the guard position with the exponent."""
    man = np.arange(1 << 23, dtype=np.uint32)
    for e in range(0x66, 0x72):
        bits = man | np.uint32((sign << 31) | (e << 23))
        assert_same_bits(O.fp32_to_fp16_bits(bits), O.ref_fp32_to_fp16_bits(bits), f"Fp32ToFp16, exponent {e:#x}")


def test_fp32_to_fp16_random_patterns(ref):
    bits = O.random_bit_patterns(O.INT32, 1 << 22, seed=0xF32F16).view(np.uint32)
    assert_same_bits(O.fp32_to_fp16_bits(bits), O.ref_fp32_to_fp16_bits(bits), "Fp32ToFp16, random")


# ----------------------------------------------------------------------------------------------- element rule

WIDE = 1 << 20


def rule_sets(dtype):
    """name -> (src, dst) of the issue's list for this dtype."""
    if dtype == O.INT8:
        v = np.arange(256, dtype=np.uint8).view(np.int8)
        return {"every pair": (np.repeat(v, 256), np.tile(v, 256))}
    if dtype == O.FP16:
        every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
        partners = np.concatenate([O.edge_values(O.FP16), every[::256]])
        assert len(partners) == 14 + 256
        a, b = np.repeat(every, len(partners)), np.tile(partners, 1 << 16)
        return {"every pattern as dst": (b, a), "every pattern as src": (a, b)}
    sets = {"edge cross": O.edge_cross(dtype)}
    src = O.random_bit_patterns(dtype, WIDE, 5200 + 10 * dtype)
    sets["random bits"] = (src, O.random_bit_patterns(dtype, WIDE, 5201 + 10 * dtype))
    if dtype in (O.FP32, O.FP64):
        sets["near"] = (src, O.near_operands(dtype, src, 5300 + dtype))
        sets["nan"] = O.nan_cross(dtype)
    return sets


@pytest.fixture(scope="module")
def sets_of():
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = {k: tuple(np.ascontiguousarray(a) for a in v) for k, v in rule_sets(dtype).items()}
            for pair in cache[dtype].values():
                for a in pair:
                    a.setflags(write=False)
        return cache[dtype]

    return get


@pytest.mark.parametrize("op", O.OPS, ids=_ids_op)
@pytest.mark.parametrize("dtype", ROUTED, ids=_ids_dt)
def test_element_rule(ref, sets_of, dtype, op):
    for name, (src, dst) in sets_of(dtype).items():
        want = O.ref_local_reduce(dtype, op, dst.copy(), src)
        got = O.local_reduce(dtype, op, dst.copy(), src)
        assert O.equal_bits_select(dtype, op, got, want), \
            f"{O.DTYPE_NAMES[dtype]} {O.OP_NAMES[op]}, {name}: {first_diffs(got, want)}"


def test_nan_set_is_what_it_says():
    """266 NaNs per float dtype (quiet and signalling, both signs), every one a NaN, each in both roles."""
    for dtype in (O.FP16, O.FP32, O.FP64):
        u, mbits, emax = O.FLOAT_LAYOUT[dtype]
        n = O.nan_values(dtype).view(u).astype(np.uint64)
        assert len(n) == 266 and len(np.unique(n)) > 200
        assert np.all((n >> np.uint64(mbits)) & np.uint64(emax) == emax) and np.all(n & np.uint64((1 << mbits) - 1) != 0)
        quiet = (n >> np.uint64(mbits - 1)) & np.uint64(1) == 1
        assert 100 < np.count_nonzero(quiet) < 166
        assert np.count_nonzero(n >> np.uint64(mbits + emax.bit_length())) == 133
        src, dst = O.nan_cross(dtype)
        assert src.size == dst.size == 2 * 266 * 7


@pytest.mark.parametrize("dtype", [O.INT16, O.BFP16], ids=_ids_dt)
def test_unrouted_dtypes(ref, dtype):
    a = np.ones(8, O.NP_STORAGE[dtype])
    for op in O.OPS:
        d_ref, d_orc = a.copy(), a.copy()
        assert O.ref_reduce(dtype, op, d_ref, a) == HCCL_E_INTERNAL
        assert O.aicpu_reduce(dtype, op, d_orc, a) == HCCL_E_INTERNAL
        assert np.array_equal(d_ref, a) and np.array_equal(d_orc, a)


@pytest.mark.parametrize("dtype", ROUTED, ids=_ids_dt)
def test_unknown_op(ref, dtype):
    a = np.ones(8, O.NP_STORAGE[dtype])
    for op in (4, 9):
        assert O.ref_reduce(dtype, op, a.copy(), a) == HCCL_E_INTERNAL
        assert O.aicpu_reduce(dtype, op, a.copy(), a) == HCCL_E_INTERNAL


# ----------------------------------------------------------------------------------------------- recorded fixture

@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def ordered_fold(reduce, dtype, op, srcs, steps=CHAIN_STEPS):
    """acc = srcs[0]; acc = srcs[j] (op) acc; yields (k, acc) after k operands for k in steps."""
    acc = srcs[0].copy()
    for j in range(1, len(srcs)):
        reduce(dtype, op, acc, srcs[j])
        if j + 1 in steps:
            yield j + 1, acc.copy()


def check_golden(z, reduce, exact):
    for dtype in ROUTED:
        name = O.DTYPE_NAMES[dtype]
        src, dst = z[f"{name}_src"], z[f"{name}_dst"]
        srcs = [z[f"{name}_chain_in{j}"] for j in range(8)]
        for op in O.OPS:
            opn = O.OP_NAMES[op]
            pairs = [(f"{name}_{opn}", reduce(dtype, op, dst.copy(), src))]
            pairs += [(f"{name}_chain_{opn}_{k}", acc) for k, acc in ordered_fold(reduce, dtype, op, srcs)]
            for key, got in pairs:
                if exact:
                    assert_same_bits(got, z[key], key)
                else:
                    assert O.equal_bits_select(dtype, op, got, z[key]), f"{key}: {first_diffs(got, z[key])}"


def test_oracle_reproduces_the_recorded_reference(golden):
    """Needs no compiled reference: tests/golden/ref_local_reduce.npz holds its results as data."""
    check_golden(golden, O.local_reduce, exact=False)


def test_oracle_reduce_n_reproduces_the_recorded_chain(golden):
    """O.reduce_n is the fold the GPU tests compare LaunchReduceN with."""
    for dtype in ROUTED:
        name = O.DTYPE_NAMES[dtype]
        srcs = [golden[f"{name}_chain_in{j}"] for j in range(8)]
        for op in O.OPS:
            for k in CHAIN_STEPS:
                key = f"{name}_chain_{O.OP_NAMES[op]}_{k}"
                got = O.reduce_n(dtype, op, srcs[:k])
                assert O.equal_bits_select(dtype, op, got, golden[key]), f"{key}: {first_diffs(got, golden[key])}"


def test_recorded_fixture_is_current(ref, golden):
    """The compiled reference reproduces the committed file exactly (a stale fixture fails here)."""
    check_golden(golden, O.ref_local_reduce, exact=True)
