"""The one-sided widening FP8 sum (hccl_amd/csrc/ipc_k_widen.hip): HcclAmdAllReduceWiden / ReduceScatterWiden /
ReduceWiden under HCCL_AMD_ALGO_IPC in loopback worlds, and on a communicator without a send/recv transport (two
processes on the one GPU).

Expected values as in tests/test_gpu_collectives_widen.py: decode to float32, the O1 fold in float32 (own input first,
then the other ranks ascending), one .to(output type); NaN positions equal, everything else bit for bit.

Shapes: with element size 1 a block window is a multiple of 16 elements. Count 1 is the element-wise edge alone, 1000
leaves a ragged end behind the load units, 40,000 spreads over several block windows.
"""
import datetime
import multiprocessing as mp
import os
import traceback

import pytest
import torch

import hccl_amd as H
from test_gpu_ipc_ranks import _free_port
from tests.test_gpu_collectives_widen import AR, OPS, RS, check, expected, inputs, run
from tests.test_gpu_reduce_widen import E4M3, E5M2, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds():
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = H.loopback_world(n)
            for c in cache[n]:
                c.set_config(H.Config.IPC_TIMEOUT_MS, 20000)  # a stuck barrier fails the test, never hangs the box
                c.set_algo(H.Algo.IPC)
        return cache[n]

    yield get
    torch.cuda.synchronize()
    for comms in cache.values():
        for c in comms:
            c.destroy()


def run_checked(comms, op, fdt, odt, xs, count, what, **kw):
    root, _, recvs = run(comms, op, fdt, odt, xs, count, **kw)
    check(xs, fdt, odt, op, count, root, recvs, what=what)
    assert comms[0].last_algo == H.Algo.IPC and comms[0].ipc_status() & 1 == 0, what
    return recvs


@pytest.mark.parametrize("n", [2, 3, 8])
def test_one_sided_widened_collectives(worlds, n):
    for op in OPS:
        for fdt, odt in ((E5M2, torch.float32), (E4M3, torch.bfloat16), (E4M3, torch.float16)):
            for count in (1, 1000, 40000):
                run_checked(worlds(n), op, fdt, odt, inputs(n, op, count), count, f"{op} {fdt} -> {odt} count {count}")


def test_several_rounds(monkeypatch):
    """The large staging tier at its smallest accepted size (16 MiB alternate areas, three slots each): 11.2 M elements
    take three rounds, asserted from the planner before anything runs, so both alternate areas are used again."""
    monkeypatch.setenv("HCCL_AMD_IPC_STAGING_MIB", "16")
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")
    n, count = 3, 11_200_000
    _, launches = H.ipc_plan(H.OpType.ALLREDUCE, n, count, H.HcclDataType.INT8, family=int(H.Algo.MESH_ONESHOT),
                             sharedDevice=1)
    assert len(launches) == 1 and launches[0].rounds >= 3, launches[0].rounds
    comms = H.loopback_world(n)
    try:
        for c in comms:
            c.set_algo(H.Algo.IPC)
        for op in OPS:
            run_checked(comms, op, E5M2, torch.float32, inputs(n, op, count), count, op)
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("op", [AR, RS])
def test_misaligned_buffers(worlds, op):
    """sendBuf one byte and recvBuf one element off 16-byte alignment: every window is element-wise."""
    n, count, fdt, odt = 2, 40001, E4M3, torch.bfloat16
    xs = inputs(n, op, count)
    sends = [torch.cat([x[:1], x]).cuda()[1:].view(fdt) for x in xs]
    recvs = [torch.full((count + 1,), -7.0, dtype=odt, device="cuda")[1:] for _ in range(n)]
    assert all(t.data_ptr() % 16 != 0 for t in sends + recvs)
    run_checked(worlds(n), op, fdt, odt, xs, count, op, sends=sends, recvs=recvs)


def test_same_bits_as_the_schedule_path(worlds):
    n, count = 3, 40000
    comms, xs = worlds(n), inputs(n, AR, count)
    ipc = run_checked(comms, AR, E5M2, torch.float32, xs, count, "ipc")
    for c in comms:
        c.set_algo(H.Algo.AUTO)
    try:
        _, _, sched = run(comms, AR, E5M2, torch.float32, xs, count)
        assert comms[0].last_algo == H.Algo.MESH_ONESHOT
    finally:
        for c in comms:
            c.set_algo(H.Algo.IPC)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ipc, sched))


def _rank_main(rank, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"  # a lost peer shows as a status bit, never a hang
    try:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)

        def all_gather(b):
            out = [None] * 2
            dist.all_gather_object(out, b)
            return out

        comm = H.comm_init_host_exchange(2, rank, all_gather)
        stream = torch.cuda.Stream()
        n, count, root, fdt, odt, out = 2, 5001, 1, E4M3, torch.bfloat16, {}
        for op in (AR, RS, "reduce_rootlast"):
            xs = inputs(n, op, count)
            send = xs[rank].cuda().view(fdt)
            recv = torch.full((count,), -7.0, dtype=odt, device="cuda")
            torch.cuda.synchronize()
            if op == AR:
                comm.all_reduce_widen(send, recv, stream)
            elif op == RS:
                comm.reduce_scatter_widen(send, recv, stream)
            else:
                comm.reduce_widen(send, recv, root, stream)
            stream.synchronize()
            if op == "reduce_rootlast" and rank != root:
                ok = bool((recv == -7.0).all())
            else:
                ok = same(recv.cpu(), expected(xs, fdt, odt, op, count, rank))
            out[op] = (ok, comm.last_algo, comm.ipc_status() & 0xFF)
        dist.barrier()
        comm.destroy()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:  # noqa: BLE001
        q.put((rank, {"error": traceback.format_exc()}))


def test_two_processes_without_a_transport():
    """Rank mode: host-exchange communicators have no send/recv transport, so every widened call takes the kernel."""
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(2):
        assert "error" not in got[r], got[r].get("error")
        assert got[r] == {op: (True, int(H.Algo.IPC), 0) for op in (AR, RS, "reduce_rootlast")}, (r, got[r])
