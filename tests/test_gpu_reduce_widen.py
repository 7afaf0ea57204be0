"""The widening FP8 sum kernel (hccl_amd/csrc/reduce_widen.hip) through HcclAmdLocalReduceNWiden.

Reference: plain torch on the CPU. x.view(float8).to(float32) is the decode, the fold is float32 adds in operand order
(acc = x[j] + acc), narrowing is .to(bfloat16 / float16). NaN positions must agree and every other element bit for bit
(the sign of zero included); NaN payloads are not compared. For E4M3 the float64 sum must give the same bits too: up to
16 values within 2^-9 .. 16 * 448 < 2^13 sum exactly in float32 in any order, which pins the operand set apart from the
order.

Launch constants the shapes come from: a tile is 256 lanes x U output vectors = 8192 elements for every output type
(FP32: U = 8 vectors of 4; BF16 / FP16: U = 4 vectors of 8), and the persistent grid is 2 workgroups per CU.
"""
import itertools

import pytest
import torch

import hccl_amd as H

pytestmark = pytest.mark.gpu

TILE = 8192
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
PAIRS = list(itertools.product((E4M3, E5M2), (torch.float32, torch.bfloat16, torch.float16)))
pairs = pytest.mark.parametrize("fdt,odt", PAIRS, ids=lambda d: str(d).split(".")[-1])
GUARD = 64


def same(got, want):  # NaN masks equal, every other element equal in its bits
    ints = torch.int32 if got.dtype == torch.float32 else torch.int16
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(ints)[~nan], want.view(ints)[~nan])


def random_bytes(nsrc, count, seed):
    g = torch.Generator().manual_seed(seed)
    srcs = [torch.randint(0, 256, (count,), dtype=torch.uint8, generator=g) for _ in range(nsrc)]
    if nsrc >= 2:  # E5M2: +inf + -inf -> NaN (and inf + finite) always present
        srcs[0][0], srcs[1][0] = 0x7C, 0xFC
        srcs[0][count - 1] = 0x7C
    return srcs


def check_fold(fdt, odt, srcs, out_shift=0, src_shifts=None, what=""):
    """The fold of the byte tensors `srcs`, out out_shift elements and operand j src_shifts[j] bytes off 16-B alignment."""
    count, osize = srcs[0].numel(), torch.empty(0, dtype=odt).element_size()
    src_shifts = src_shifts or [0] * len(srcs)
    dev = []
    for s, sh in zip(srcs, src_shifts):
        d = torch.empty(count + 16, dtype=torch.uint8, device="cuda")[sh:sh + count]
        d.copy_(s)
        dev.append(d.view(fdt))
    lo = GUARD + out_shift * osize
    raw = torch.full((lo + count * osize + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = raw[lo:lo + count * osize].view(odt)
    H.local_reduce_n_widen(out, dev)
    torch.cuda.synchronize()
    guards_kept = bool((raw[:lo] == 0xA5).all()) and bool((raw[lo + count * osize:] == 0xA5).all())
    assert guards_kept, f"{what}: guard bytes written"
    f32 = [s.view(fdt).to(torch.float32) for s in srcs]
    acc = f32[0]
    for x in f32[1:]:
        acc = x + acc
    got = out.cpu()
    assert same(got, acc.to(odt)), f"{what}: differs from the ordered float32 fold"
    if fdt == E4M3:
        exact = f32[-1].to(torch.float64)  # summed backwards, without sum()'s +0 start (it would turn -0 + -0 into +0)
        for x in f32[-2::-1]:
            exact = exact + x.to(torch.float64)
        assert same(got, exact.to(torch.float32).to(odt)), f"{what}: differs from the exact sum"


@pairs
def test_every_pair_of_byte_patterns(fdt, odt):
    i = torch.arange(65536)
    check_fold(fdt, odt, [(i // 256).to(torch.uint8), (i % 256).to(torch.uint8)])


@pairs
def test_operand_counts(fdt, odt):
    for nsrc in (1, 3, 8, 16):
        check_fold(fdt, odt, random_bytes(nsrc, 2 * TILE + 37, seed=nsrc), what=f"nsrc {nsrc}")


@pairs
def test_shapes_and_misalignment(fdt, odt):
    """Counts: no vector body (1, 3); a tile less one; a tile and a ragged rest; more tiles than workgroups (some take a
    second). Then out one element past alignment and the operands one byte, so that their loads line up where out's
    vectors start (a head of 3 or 7 elements); one operand alone one byte off (the phases do not line up: the scalar
    kernel); every operand 4 bytes off with out aligned. One test per type pair: the suite's count of test ids is kept
    low, every case is named in its failure message."""
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    for count in (1, 3, TILE - 1, TILE + 5, grid * TILE + TILE + 5):
        check_fold(fdt, odt, random_bytes(3, count, seed=count % 1000), what=f"count {count}")
    for out_shift, src_shifts in ((1, [1, 1, 1]), (0, [0, 1, 0]), (0, [4, 4, 4])):
        check_fold(fdt, odt, random_bytes(3, TILE + 69, seed=7), out_shift, src_shifts,
                   what=f"out +{out_shift} elements, operands +{src_shifts} bytes")


def test_refusals():
    x = torch.zeros(64, dtype=torch.uint8, device="cuda").view(E4M3)
    cases = [([x, x], torch.int32, H.HcclResult.HCCL_E_NOT_SUPPORT),
             ([x.view(torch.uint8)[:32].view(torch.float16)] * 2, torch.float32, H.HcclResult.HCCL_E_NOT_SUPPORT),
             ([x] * 17, torch.float32, H.HcclResult.HCCL_E_PARA)]
    for srcs, odt, code in cases:
        out = torch.zeros(srcs[0].numel(), dtype=odt, device="cuda")
        with pytest.raises(H.HcclError) as e:
            H.local_reduce_n_widen(out, srcs)
        assert e.value.code == code
        assert not out.any()
    with pytest.raises(H.HcclError) as e:  # the same-type fold still has no FP8
        H.local_reduce_n(x.clone(), [x, x])
    assert e.value.code == H.HcclResult.HCCL_E_NOT_SUPPORT
