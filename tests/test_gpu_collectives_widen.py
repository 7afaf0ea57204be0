"""HcclAmdAllReduceWiden / ReduceScatterWiden / ReduceWiden on loopback worlds, one thread per rank.

Expected per rank: the O1 fold in float32 (the rank's own input first, then the other ranks' ascending), narrowed once;
plain torch on the CPU, compared as tests/test_gpu_reduce_widen.py compares (NaN positions, else bit for bit).
"""
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import hccl_amd as H
from tests.test_gpu_reduce_widen import E4M3, E5M2, same

pytestmark = pytest.mark.gpu

AR, RS = "all_reduce", "reduce_scatter"
OPS = [AR, RS, "reduce_root0", "reduce_rootlast"]


@pytest.fixture(scope="module")
def worlds():
    cache = {}
    yield lambda n: cache[n] if n in cache else cache.setdefault(n, H.loopback_world(n))
    torch.cuda.synchronize()
    for comms in cache.values():
        for c in comms:
            c.destroy()


def run_ranks(n, fn):
    """fn(r) for every rank, one thread each; a rank's exception is raised here."""
    with ThreadPoolExecutor(n) as pool:
        list(pool.map(fn, range(n)))


def inputs(n, op, count):
    g = torch.Generator().manual_seed(1000 * n + count)
    xs = [torch.randint(0, 256, (count * (n if op == RS else 1),), dtype=torch.uint8, generator=g) for _ in range(n)]
    xs[0][0], xs[n - 1][0] = 0x7C, 0xFC  # E5M2: +inf and -inf meet in element 0
    return xs


def expected(xs, fdt, odt, op, count, r):
    f32 = [(x[r * count:(r + 1) * count] if op == RS else x).view(fdt).to(torch.float32) for x in xs]
    acc = f32[r]
    for q in range(len(xs)):
        if q != r:
            acc = f32[q] + acc
    return acc.to(odt)


def run(comms, op, fdt, odt, xs, count, sends=None, recvs=None, streams=None):
    """One widened collective on every rank; returns (root, device inputs, device outputs)."""
    n = len(comms)
    root = 0 if op == "reduce_root0" else n - 1
    sends = sends or [x.cuda().view(fdt) for x in xs]
    recvs = recvs or [torch.full((count,), -7.0, dtype=odt, device="cuda") for _ in range(n)]
    streams = streams or [torch.cuda.Stream() for _ in range(n)]
    torch.cuda.synchronize()

    def body(r):
        if op == AR:
            comms[r].all_reduce_widen(sends[r], recvs[r], streams[r])
        elif op == RS:
            comms[r].reduce_scatter_widen(sends[r], recvs[r], streams[r])
        else:
            comms[r].reduce_widen(sends[r], recvs[r], root, streams[r])

    run_ranks(n, body)
    torch.cuda.synchronize()
    return root, sends, recvs


def check(xs, fdt, odt, op, count, root, recvs, what=""):
    for r, out in enumerate(recvs):
        if op.startswith("reduce_root") and r != root:
            assert bool((out == -7.0).all()), f"{what} rank {r}: a non-root output was written"
        else:
            assert same(out.cpu(), expected(xs, fdt, odt, op, count, r)), f"{what} rank {r}"


@pytest.mark.parametrize("n", [2, 3, 8])
def test_widened_collectives(worlds, n):
    """Every operator x type pair x count in one test per world size (the suite's count of test ids is kept low; the
    failing case is in the message)."""
    comms = worlds(n)
    for c in comms:
        c.set_algo(H.Algo.RING)  # the family override does not apply
    for op in OPS:
        for fdt, odt in ((E5M2, torch.float32), (E4M3, torch.bfloat16)):
            for count in (1, 1000, 40000):
                xs = inputs(n, op, count)
                root, _, recvs = run(comms, op, fdt, odt, xs, count)
                check(xs, fdt, odt, op, count, root, recvs, what=f"{op} {fdt} -> {odt} count {count}")
                assert comms[0].last_algo == H.Algo.MESH_ONESHOT
    for c in comms:
        c.set_algo(H.Algo.AUTO)


def test_pieces_wrap_the_staging_slots(worlds):
    """40,000 elements in pieces of 8 KiB: five pieces, so both staging slot sets are used again."""
    n, count = 3, 40000
    comms = worlds(n)
    for c in comms:
        c.set_piece_bytes(8192)
    for op in OPS:
        xs = inputs(n, op, count)
        root, _, recvs = run(comms, op, E5M2, torch.float32, xs, count)
        check(xs, E5M2, torch.float32, op, count, root, recvs, what=op)
    for c in comms:
        c.set_piece_bytes(0)


def test_one_rank_is_a_widening_copy(worlds):
    xs = inputs(1, AR, 1000)
    root, _, recvs = run(worlds(1), AR, E4M3, torch.float16, xs, 1000)
    check(xs, E4M3, torch.float16, AR, 1000, root, recvs)


def test_repeat_and_same_type_call_between(worlds):
    """The same buffers twice (compiled collective and graph keys), same-type all_reduce calls of the same count and
    family in between (FP32, and INT8 with the FP8 input's element size), then both 16-bit output types."""
    n, count = 2, 40000
    comms = worlds(n)
    xs = inputs(n, AR, count)
    streams = [torch.cuda.Stream() for _ in range(n)]
    root, sends, recvs = run(comms, AR, E5M2, torch.float32, xs, count, streams=streams)
    first = [r.clone() for r in recvs]
    for c in comms:
        c.set_config(H.Config.SMALL_IPC_BYTES, 0)  # the same-type calls run their schedule, not the one-sided kernel
        c.set_algo(H.Algo.MESH_ONESHOT)
    for dt in (torch.float32, torch.int8):
        fs = [torch.full((count,), r + 1, dtype=dt, device="cuda") for r in range(n)]
        fr = [torch.zeros(count, dtype=dt, device="cuda") for _ in range(n)]
        run_ranks(n, lambda r: comms[r].all_reduce(fs[r], fr[r], H.HcclReduceOp.SUM, streams[r]))
        torch.cuda.synchronize()
        assert all(bool((t == 3).all()) for t in fr)
    for c in comms:
        c.set_algo(H.Algo.AUTO)
        c.reload_config()
    for t in recvs:
        t.fill_(-7.0)
    run(comms, AR, E5M2, torch.float32, xs, count, sends=sends, recvs=recvs, streams=streams)
    check(xs, E5M2, torch.float32, AR, count, root, recvs)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, recvs))
    for odt in (torch.bfloat16, torch.float16):
        root, _, outs = run(comms, AR, E5M2, odt, xs, count, sends=sends, streams=streams)
        check(xs, E5M2, odt, AR, count, root, outs)
