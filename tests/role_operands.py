"""Operands on which the src / dst roles of MAX and MIN show (a helper module: nothing here is collected).

The element rule is dst = src (op) dst with std::max / std::min semantics: a tie (+0 against -0) and an unordered
compare (a NaN on either side) both return src. On ordinary data neither the roles nor the association of a fold are
visible under MAX / MIN; they are where two ranks hold a tie or a NaN at the same element index. role_operands() lays
such pairs out densely: with pairs = the ordered rank pairs (a, b), a != b, in lexicographic order, kinds = [(+0, -0),
(NaN, +0), (NaN, -0)] and P = 3 n (n - 1), element e (q = (e + shift) % P) gives rank pairs[q // 3][0] the value
kinds[q % 3][0], rank pairs[q // 3][1] the value kinds[q % 3][1], and every other rank the op's loser (-1 for MAX, +1
for MIN), which loses against either zero and is returned (being src) or dropped (being dst) against a NaN.

Every whole period therefore holds every ordered pair of ranks in every kind, and exchanging two operands of any fold
changes the result in at least 6 elements of it (tests/test_role_operands.py checks that on the oracle alone).
"""
import numpy as np

from oracle import oracle as O

KINDS = 3  # (+0, -0), (NaN, +0), (NaN, -0)

# (+0, -0, quiet NaN, -1, +1) in the oracle's storage type; explicit bit patterns for the 16-bit formats
_BITS16 = {O.FP16: (0x0000, 0x8000, 0x7E00, 0xBC00, 0x3C00), O.BFP16: (0x0000, 0x8000, 0x7FC0, 0xBF80, 0x3F80)}


def period(n):
    return KINDS * n * (n - 1)


def _values(dtype):
    if dtype in _BITS16:
        return np.array(_BITS16[dtype], np.uint16)
    return np.array([0.0, -0.0, np.nan, -1.0, 1.0], O.NP_STORAGE[dtype])


def role_operands(dtype, op, n, count, shift=0):
    """n arrays of `count` elements in the oracle's storage type (see the module docstring). For a ReduceScatter pass
    the whole input length (recv count x n): every output block then sees whole periods at a shift of its own."""
    # integer ties are bit-identical, so no role can show on them: there is nothing to generate
    assert dtype in O.FLOAT_DTYPES, "role operands exist for floating-point dtypes only"
    assert op in (O.MAX, O.MIN), "SUM and PROD are commutative bit for bit: roles cannot show"
    assert n >= 2
    pz, nz, nan, minus1, plus1 = _values(dtype)
    loser = minus1 if op == O.MAX else plus1
    first = np.array([pz, nan, nan])   # held by pairs[q // 3][0]
    second = np.array([nz, pz, nz])    # held by pairs[q // 3][1]
    pairs = np.array([(a, b) for a in range(n) for b in range(n) if a != b])
    q = (np.arange(count, dtype=np.int64) + shift) % period(n)
    ra, rb, kind = pairs[q // KINDS, 0], pairs[q // KINDS, 1], q % KINDS
    xs = []
    for r in range(n):
        x = np.full(count, loser, O.NP_STORAGE[dtype])
        x[ra == r] = first[kind[ra == r]]
        x[rb == r] = second[kind[rb == r]]
        xs.append(np.ascontiguousarray(x))
    return xs
