"""The Broadcast's schedule programs through RCCL send/recv groups and the executor on hardware, over a self loop.

Neither rank's own program pairs on a self loop (the root's only sends, a non-root's receives more than it sends; the
same limit tests/test_gpu_rccl.py records for Reduce). The stand-in is the traffic between the root and one non-root
rank of n = 4, merged group by group into one program: every send of the root to that rank meets the rank's receive,
and the rank's gather sends meet its gather receives of equal size. It keeps what the RCCL path of this operator has
that no other test runs there: programs of SEND and RECV records only, no staging (the communicator holds none, so
the executor's staging pointer is null), INPUT and OUTPUT at one base, pipelined groups, eager and replayed from the
executor's graph cache in both executor modes. Every run is compared byte for byte with the oracle's replay of the
same program on the same (aliased) buffers.
"""
import multiprocessing as mp
import os
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BCAST, SEND, RECV = 5, 2, 3
N, BROOT, PEER = 4, 2, 1
# (count, pieceBytes): one piece (two groups), and four pipelined pieces of 64 KiB (five groups); int32, equal chunks
CASES = [(4 * 65536, 0), (4 * 65536, 64 << 10), (4 * 1000, 0)]


def merged_program(H, count, dtype, piece_bytes):
    """One program for a self loop from the root's and one non-root rank's programs: per group, the root's sends to
    that rank interleaved with the rank's receives from the root, then the rank's gather sends each followed by a
    gather receive of the same size. Every record's peer becomes 0 (the self loop)."""
    r_ops, r_n, _, _ = H.build_schedule(BCAST, 0, N, BROOT, count, dtype, BROOT, piece_bytes)
    p_ops, p_n, _, scratch = H.build_schedule(BCAST, 0, N, PEER, count, dtype, BROOT, piece_bytes)
    assert scratch == 0
    rs = [r_ops[i] for i in range(r_n)]
    ps = [p_ops[i] for i in range(p_n)]
    out = []
    for g in sorted({o.group for o in rs + ps}):
        down = [o for o in rs if o.group == g and o.kind == SEND and o.peer == PEER]
        up = [o for o in ps if o.group == g and o.kind == RECV and o.peer == BROOT]
        assert [o.count for o in down] == [o.count for o in up]
        for s, r in zip(down, up):
            out += [s, r]
        sends = [o for o in ps if o.group == g and o.kind == SEND]
        recvs = [o for o in ps if o.group == g and o.kind == RECV and o.peer != BROOT]
        assert sorted(o.count for o in sends) == sorted(o.count for o in recvs)
        for s in sends:
            r = next(x for x in recvs if x.count == s.count)
            recvs.remove(r)
            out += [s, r]
    for o in out:
        o.peer = 0
    return (H.HcclAmdIrOp * len(out))(*out), len(out)


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
            arr, nops = merged_program(H, count, dtype, piece)
            groups = len({arr[i].group for i in range(nops)})
            for single in (False, True):
                buf = to_device(dtype, np.zeros(count, np.int32))
                before = comm.graph_stats()[0]
                for rep in range(5):  # eager, then captured, then replayed from the executor's graph cache
                    x = np.random.default_rng(100 * k + rep).integers(-2**31, 2**31 - 1, count, dtype=np.int32)
                    want = x.copy()
                    assert O.replay(1, dtype, O.SUM, [(arr, nops)], [[want, want, np.zeros(1, np.int32)]]) == 0
                    torch.cuda.synchronize()
                    buf.copy_(to_device(dtype, x))
                    torch.cuda.synchronize()
                    comm.execute(arr, nops, buf, buf, O.SUM, single, stream, dtype=dtype)  # INPUT = OUTPUT
                    torch.cuda.synchronize()
                    got = to_host(dtype, buf)
                    results.append((k, single, rep, bool(got.tobytes() == want.tobytes()),
                                    bool(want.tobytes() != x.tobytes())))
                results.append((k, single, "graph_launches", comm.graph_stats()[0] - before, groups))
        results.append(("scratch", comm.scratch()[0], comm.device_bytes()))
        comm.destroy()
        q.put(("ok", results))
    except Exception as e:  # noqa: BLE001
        q.put(("err", f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))


def test_broadcast_programs_over_the_rccl_self_loop():
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
    assert all(r[3] >= 3 for r in launches), launches  # the later calls were graph replays
    assert results[-1][:2] == ("scratch", 0), results[-1]  # no executor staging was ever allocated
