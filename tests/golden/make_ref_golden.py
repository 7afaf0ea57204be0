"""Records tests/golden/ref_local_reduce.npz from the reference's own arithmetic, compiled (oracle/_ref/).

oracle/_ref/libhccl_ref_reduce.so is the reference's AicpuReduce and fp16 converters, built by `make -C oracle` when
the reference tree is there. It does not travel with a checkout, so what it computes is recorded here once, as data,
for the tests that must not depend on it (tests/test_gpu_reference_pins.py, tests/test_oracle_vs_reference.py). This
script loads nothing but that library (through oracle/oracle.py) and numpy.

Per routed dtype (INT8, INT32, FP16, FP32, INT64, UINT64, FP64):
  <dt>_src, <dt>_dst          O.edge_cross, then O.nan_cross (floats), then seeded random operands (full-range bit
                              patterns for floats and integers alike) up to PAIR_COUNT[dt] elements
  <dt>_<op>                   the reference's dst = src (op) dst
  <dt>_chain_in0 .. 7         eight operands of CHAIN_COUNT elements: for floats half of them drawn from the edge values
                              and O.nan_values, the rest random bit patterns; for integers edge values among random ones
  <dt>_chain_<op>_<k>         the reference's ordered fold acc = in0; acc = in_j (op) acc after k = 2, 3, 4, 7, 8 operands

Size: 34 arrays per dtype at 4,099 elements each would be 4.9 MB of mostly incompressible bits, against a limit of
1 MiB per committed file. Random elements are cut, never the edge or NaN sets: the 1-, 2- and 4-byte dtypes and FP64
(3,845 of whose elements are edge and NaN pairs, which compress) keep 4,099 pair elements, INT64 and UINT64 keep 1,027
(513 16-byte vectors and a tail), and the chains have 259 elements.

Run: make -C oracle && python tests/golden/make_ref_golden.py   (rewrites the .npz; the file is committed)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

ROUTED = [O.INT8, O.INT32, O.FP16, O.FP32, O.INT64, O.UINT64, O.FP64]
PAIR_COUNT = {O.INT8: 4099, O.INT32: 4099, O.FP16: 4099, O.FP32: 4099, O.INT64: 1027, O.UINT64: 1027, O.FP64: 4099}
CHAIN_COUNT = 259
CHAIN_STEPS = (2, 3, 4, 7, 8)


def pair_operands(dtype):
    es, ed = O.edge_cross(dtype)
    ns, nd = O.nan_cross(dtype)
    fill = PAIR_COUNT[dtype] - es.size - ns.size
    assert fill > 0
    rs = O.random_bit_patterns(dtype, fill, 0x5EF0000 + dtype)
    rd = O.random_bit_patterns(dtype, fill, 0x5EF1000 + dtype)
    return np.ascontiguousarray(np.concatenate([es, ns, rs])), np.ascontiguousarray(np.concatenate([ed, nd, rd]))


def chain_operand(dtype, j):
    rng = np.random.default_rng(0x5EF2000 + 16 * dtype + j)
    a = O.random_bit_patterns(dtype, CHAIN_COUNT, 0x5EF3000 + 16 * dtype + j).copy()
    pool = O.edge_values(dtype)
    if dtype in O.FLOAT_LAYOUT:
        pool = np.concatenate([pool, O.nan_values(dtype)])
        picks = CHAIN_COUNT // 2
    else:
        picks = 2 * len(pool)
    a[rng.choice(CHAIN_COUNT, size=picks, replace=False)] = rng.choice(pool, size=picks)
    return np.ascontiguousarray(a)


def main():
    assert O.ref_available(), "build oracle/_ref/ first: make -C oracle (needs the reference tree)"
    out = {}
    for dtype in ROUTED:
        name = O.DTYPE_NAMES[dtype]
        src, dst = pair_operands(dtype)
        out[f"{name}_src"], out[f"{name}_dst"] = src, dst
        srcs = [chain_operand(dtype, j) for j in range(8)]
        for j, a in enumerate(srcs):
            out[f"{name}_chain_in{j}"] = a
        for op in O.OPS:
            opn = O.OP_NAMES[op]
            out[f"{name}_{opn}"] = O.ref_local_reduce(dtype, op, dst.copy(), src)
            acc = srcs[0].copy()
            for j in range(1, 8):
                O.ref_local_reduce(dtype, op, acc, srcs[j])
                if j + 1 in CHAIN_STEPS:
                    out[f"{name}_chain_{opn}_{j + 1}"] = acc.copy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_local_reduce.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
