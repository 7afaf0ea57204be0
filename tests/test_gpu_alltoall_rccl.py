"""The all-to-all's schedule program through RCCL send/recv groups and the executor on hardware, over a self loop.

One rank's program of an n = 4 world with even counts pairs on a self loop as it stands: every peer gets one send and
one receive of the same size, posted in the same order, so each send meets the receive posted beside it. It keeps what
the RCCL path of this operator has: SEND and RECV records at arbitrary offsets of two distinct buffers, one COPY, no
staging (the communicator holds none), one group by default and one per piece with an explicit granule, eager and
replayed from the executor's graph cache in both executor modes. Every run is compared byte for byte with the oracle's
replay of the same program; the operator itself (HcclAlltoAll on the self-loop communicator, where the one-sided kernel
is unavailable) must take the schedule and give the same bytes.
"""
import multiprocessing as mp
import os
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, RANK = 4, 1
# (elements per pair, pieceBytes): one group; four groups of 64 KiB pieces; a small ragged-free one. int32.
CASES = [(65536, 0), (65536, 64 << 10), (1000, 0)]


def _worker(q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        import torch
        import hccl_amd as H
        from oracle import oracle as O
        from tests._util import to_device, to_host
        torch.cuda.set_device(0)
        comm = H.comm_init_selfloop(N, RANK)
        stream = torch.cuda.Stream()
        dtype = O.INT32
        results = []
        for k, (count, piece) in enumerate(CASES):
            counts = [count] * N
            displs = [p * count for p in range(N)]
            arr, nops, scratch = H.build_schedule_alltoall(N, RANK, counts, displs, counts, displs, dtype, piece)
            assert scratch == 0
            groups = len({arr[i].group for i in range(nops) if arr[i].kind in (2, 3)})
            assert groups == (1 if piece == 0 else -(-count * 4 // piece))
            for i in range(nops):
                if arr[i].kind in (2, 3):
                    arr[i].peer = 0  # the self loop
            for single in (False, True):
                src = to_device(dtype, np.zeros(N * count, np.int32))
                dst = to_device(dtype, np.zeros(N * count, np.int32))
                before = comm.graph_stats()[0]
                for rep in range(5):  # eager, then captured, then replayed from the executor's graph cache
                    x = np.random.default_rng(100 * k + rep).integers(-2**31, 2**31 - 1, N * count, dtype=np.int32)
                    want = np.zeros(N * count, np.int32)
                    assert O.replay(1, dtype, O.SUM, [(arr, nops)], [[x.copy(), want, np.zeros(1, np.int32)]]) == 0
                    torch.cuda.synchronize()
                    src.copy_(to_device(dtype, x))
                    dst.zero_()
                    torch.cuda.synchronize()
                    comm.execute(arr, nops, src, dst, O.SUM, single, stream, dtype=dtype)
                    torch.cuda.synchronize()
                    got = to_host(dtype, dst)
                    results.append((k, single, rep, bool(got.tobytes() == want.tobytes()),
                                    bool(want.tobytes() == x.tobytes()), bool(to_host(dtype, src).tobytes() == x.tobytes())))
                results.append((k, single, "graph_launches", comm.graph_stats()[0] - before, groups))
        # the operator: the one-sided kernel is unavailable here, so the call takes the schedule
        count = 4099
        x = torch.randint(-2**31, 2**31 - 1, (N * count,), dtype=torch.int32, device="cuda")
        y = torch.zeros_like(x)
        for rep in range(3):
            y.zero_()
            torch.cuda.synchronize()
            comm.alltoall(x, y, stream)
            torch.cuda.synchronize()
            results.append(("op", rep, bool(torch.equal(x, y)), comm.last_algo))
        results.append(("scratch", comm.scratch()[0], comm.device_bytes()))
        comm.destroy()
        q.put(("ok", results))
    except Exception as e:  # noqa: BLE001
        q.put(("err", f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))


def test_alltoall_program_over_the_rccl_self_loop():
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
    runs = [r for r in results if len(r) == 6]
    assert len(runs) == len(CASES) * 2 * 5
    assert all(r[3] for r in runs), [r for r in runs if not r[3]]
    assert all(r[4] for r in runs)  # on the self loop with even counts every block comes back to its own place
    assert all(r[5] for r in runs)  # the send buffer is unchanged
    launches = [r for r in results if len(r) == 5 and r[2] == "graph_launches"]
    assert len(launches) == len(CASES) * 2
    for k, single, _, replays, groups in launches:
        # later calls were graph replays, but for a single-stream program of one group, which the executor always runs
        # eagerly (one group launch is cheaper than a graph launch: executor.cc RunCompiled)
        assert (replays == 0) if (single and groups <= 1) else (replays >= 3), launches
    ops = [r for r in results if r[0] == "op"]
    assert ops == [("op", rep, True, 1) for rep in range(3)], ops  # HCCL_AMD_ALGO_MESH_ONESHOT: the schedule path
    assert results[-1][:2] == ("scratch", 0), results[-1]  # no executor staging was ever allocated
