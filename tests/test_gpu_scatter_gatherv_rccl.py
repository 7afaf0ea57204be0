"""The Scatter's and the AllGatherV's schedule programs through RCCL send/recv groups and the executor on hardware, over
a self loop; and the compiled-collective cache key of both operators in a loopback world.

No rank's own program pairs on a self loop (the Scatter's root only sends; an AllGatherV rank sends its own count and
receives its peers'), the limit tests/test_gpu_broadcast_rccl.py records. The stand-ins are merged group by group, every
record as the generators made it, only its peer set to 0 (the self loop):
  * Scatter, n = 4: the root's sends to one peer with that peer's receives (the root's own-block COPY is left out: on
    one output buffer it would overwrite what the receives delivered);
  * AllGatherV, n = 4: two ranks with equal counts, each one's sends to the other with the other's receives, and a third
    rank's own-block COPY: three disjoint blocks of the output written by RECV, RECV and COPY.
Both with one group and cut into pieces, eager and replayed from the executor's graph cache in both executor modes,
with no staging; every run is compared byte for byte with the oracle's replay of the same program.
"""
import multiprocessing as mp
import os
import threading
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCATTER, COPY, SEND, RECV = 7, 0, 2, 3
N, SROOT, PEER = 4, 2, 1
A, B, C = 0, 3, 1  # AllGatherV: the pair with equal counts and the rank whose own copy is kept
COUNTS, DISPLS = [70001, 333, 0, 70001], [400, 7, 0, 70500]
# (count or None for AllGatherV, pieceBytes): one group, and pieces of 64 KiB
CASES = [(65536, 0), (65536, 64 << 10), (1000, 0), (None, 0), (None, 64 << 10)]


def pair_up(down, up):
    assert [o.count for o in down] == [o.count for o in up]
    out = []
    for s, r in zip(down, up):
        out += [s, r]
    return out


def merged_scatter(H, count, dtype, piece_bytes):
    r_ops, r_n, _, _ = H.build_schedule(SCATTER, 0, N, SROOT, count, dtype, SROOT, piece_bytes)
    p_ops, p_n, _, scratch = H.build_schedule(SCATTER, 0, N, PEER, count, dtype, SROOT, piece_bytes)
    assert scratch == 0
    rs, ps = [r_ops[i] for i in range(r_n)], [p_ops[i] for i in range(p_n)]
    out = []
    for g in sorted({o.group for o in rs + ps if o.kind != COPY}):
        out += pair_up([o for o in rs if o.group == g and o.kind == SEND and o.peer == PEER],
                       [o for o in ps if o.group == g and o.kind == RECV])
    return out


def merged_gatherv(H, dtype, piece_bytes):
    progs = {}
    for r in (A, B, C):
        ops, nops, scratch = H.build_schedule_all_gather_v(N, r, COUNTS, DISPLS, dtype, piece_bytes)
        assert scratch == 0
        progs[r] = [ops[i] for i in range(nops)]
    out = [o for o in progs[C] if o.kind == COPY]
    for g in sorted({o.group for r in (A, B) for o in progs[r] if o.kind != COPY}):
        for x, y in ((A, B), (B, A)):
            out += pair_up([o for o in progs[x] if o.group == g and o.kind == SEND and o.peer == y],
                           [o for o in progs[y] if o.group == g and o.kind == RECV and o.peer == x])
    return out


def _worker(q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        import torch
        import hccl_amd as H
        from oracle import oracle as O
        from tests._util import to_device, to_host
        torch.cuda.set_device(0)
        comm = H.comm_init_selfloop(N, PEER)
        stream = torch.cuda.Stream()
        dtype = O.INT32
        results = []
        for k, (count, piece) in enumerate(CASES):
            recs = merged_scatter(H, count, dtype, piece) if count is not None else merged_gatherv(H, dtype, piece)
            for o in recs:
                o.peer = 0 if o.kind != COPY else o.peer
            arr, nops = (H.HcclAmdIrOp * len(recs))(*recs), len(recs)
            groups = len({o.group for o in recs if o.kind != COPY})
            in_len = N * count if count is not None else COUNTS[A]
            out_len = count if count is not None else max(d + c for d, c in zip(DISPLS, COUNTS)) + 3
            for single in (False, True):
                d_in = to_device(dtype, np.zeros(in_len, np.int32))  # fixed addresses: the graph cache's key
                d_out = to_device(dtype, np.zeros(out_len, np.int32))
                before = comm.graph_stats()[0]
                for rep in range(5):  # eager, then captured, then replayed from the executor's graph cache
                    rng = np.random.default_rng(100 * k + rep)
                    x = rng.integers(-2**31, 2**31 - 1, in_len, dtype=np.int32)
                    fill = rng.integers(-2**31, 2**31 - 1, out_len, dtype=np.int32)
                    want = fill.copy()
                    assert O.replay(1, dtype, O.SUM, [(arr, nops)], [[x.copy(), want, np.zeros(1, np.int32)]]) == 0
                    torch.cuda.synchronize()
                    d_in.copy_(to_device(dtype, x))
                    d_out.copy_(to_device(dtype, fill))
                    torch.cuda.synchronize()
                    comm.execute(arr, nops, d_in, d_out, O.SUM, single, stream, dtype=dtype)
                    torch.cuda.synchronize()
                    got = to_host(dtype, d_out)
                    results.append((k, single, rep, bool(got.tobytes() == want.tobytes()),
                                    bool(want.tobytes() != fill.tobytes())))
                results.append((k, single, "graph_launches", comm.graph_stats()[0] - before, groups))
        results.append(("scratch", comm.scratch()[0], comm.device_bytes()))
        comm.destroy()
        q.put(("ok", results))
    except Exception as e:  # noqa: BLE001
        q.put(("err", f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))


def test_programs_over_the_rccl_self_loop():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(q,))
    p.start()
    try:
        status, results = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert status == "ok", results
    runs = [r for r in results if len(r) == 5 and r[2] != "graph_launches"]
    assert len(runs) == len(CASES) * 2 * 5
    assert all(r[3] for r in runs), [r for r in runs if not r[3]]
    assert all(r[4] for r in runs)  # the program moved something: the comparison is not of untouched buffers
    launches = [r for r in results if len(r) == 5 and r[2] == "graph_launches"]
    # the later calls were graph replays; a single-stream program of one group is never worth a graph (executor.cc)
    assert all(r[3] == 0 if r[1] and r[4] <= 1 else r[3] >= 3 for r in launches), launches
    assert {r[4] for r in launches} == {1, 4, 5}, launches  # one group, and the pieces' groups of both operators
    assert results[-1][:2] == ("scratch", 0), results[-1]  # no executor staging was ever allocated


def test_cache_key_holds_the_root_and_the_in_place_flag():
    """The compiled-collective cache (a self loop cannot reach it: no rank's own program pairs there) in a 2-rank
    loopback world on the schedule path: the same Scatter from another root, and the same AllGatherV in place, are new
    entries and deliver the right bytes; repeating a call is a hit."""
    import torch

    import hccl_amd as H

    n, count = 2, 3001
    comms = H.loopback_world(n)
    try:
        for c in comms:
            c.set_algo(int(H.Algo.MESH_ONESHOT))
        streams = [torch.cuda.Stream() for _ in range(n)]
        src = [torch.arange(n * count, dtype=torch.int32, device="cuda") * (r + 3) for r in range(n)]
        counts, displs = [count, count], [0, count]

        def on_all(fn):
            errs = []

            def body(r):
                try:
                    fn(r)
                except Exception as e:  # noqa: BLE001
                    errs.append((r, e))

            th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=120)
            torch.cuda.synchronize()
            assert not errs, errs

        stats = [comms[0].compile_stats()]
        for root in (0, 1, 0):
            outs = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
            on_all(lambda r: comms[r].scatter(src[r] if r == root else None, outs[r], root, streams[r]))
            for r in range(n):
                assert torch.equal(outs[r], src[root][r * count:(r + 1) * count]), (root, r)
            stats.append(comms[0].compile_stats())
        hits = [b[0] - a[0] for a, b in zip(stats, stats[1:])]
        misses = [b[1] - a[1] for a, b in zip(stats, stats[1:])]
        assert (hits, misses) == ([0, 0, 1], [1, 1, 0]), stats
        stats = [comms[0].compile_stats()]
        for in_place in (False, True, False):
            outs = [torch.full((n * count,), -1, dtype=torch.int32, device="cuda") for _ in range(n)]
            ins = [src[r][:count] for r in range(n)]
            if in_place:
                for r in range(n):
                    outs[r][displs[r]:displs[r] + count] = ins[r]
                ins = [outs[r][displs[r]:displs[r] + count] for r in range(n)]
            on_all(lambda r: comms[r].all_gather_v(ins[r], outs[r], counts, displs, streams[r]))
            for r in range(n):
                assert torch.equal(outs[r], torch.cat([src[q][:count] for q in range(n)])), (in_place, r)
            stats.append(comms[0].compile_stats())
        hits = [b[0] - a[0] for a, b in zip(stats, stats[1:])]
        misses = [b[1] - a[1] for a, b in zip(stats, stats[1:])]
        assert (hits, misses) == ([0, 0, 1], [1, 1, 0]), stats
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()
