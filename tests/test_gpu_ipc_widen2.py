"""The one-sided two-shot widening FP8 AllReduce (hccl_amd/csrc/ipc_k_widen2.hip): HcclAmdAllReduceWiden after
set_algo(IPC_TWOSHOT), in loopback worlds and in two processes on the one GPU.

Expected on every rank: decode to float32, the O2 fold in float32 (rank 0's input, then ranks 1 .. n-1 ascending), one
.to(output type); NaN positions equal, everything else bit for bit, and every rank's bytes equal to rank 0's.
"""
import contextlib
import datetime
import multiprocessing as mp
import os
import traceback

import pytest
import torch

import hccl_amd as H
from test_gpu_ipc_ranks import _free_port
from tests.test_gpu_collectives_widen import AR, inputs, run
from tests.test_gpu_reduce_widen import E4M3, E5M2, same

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def world(n):
    comms = H.loopback_world(n)
    try:
        for c in comms:
            c.set_config(H.Config.IPC_TIMEOUT_MS, 20000)  # a stuck barrier fails the test, never hangs the box
            c.set_algo(H.Algo.IPC_TWOSHOT)
        yield comms
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()


def expected(xs, fdt, odt):
    f32 = [x.view(fdt).to(torch.float32) for x in xs]
    acc = f32[0]
    for x in f32[1:]:
        acc = x + acc
    return acc.to(odt)


def run_checked(comms, fdt, odt, xs, count, what, **kw):
    _, _, recvs = run(comms, AR, fdt, odt, xs, count, **kw)
    assert comms[0].last_algo == H.Algo.IPC_TWOSHOT and comms[0].ipc_status() & 1 == 0, what
    ints = torch.int32 if odt == torch.float32 else torch.int16
    outs, want = [r.cpu() for r in recvs], expected(xs, fdt, odt)
    for r, out in enumerate(outs):
        assert same(out, want), f"{what} rank {r}: differs from the O2 fold"
        assert torch.equal(out.view(ints), outs[0].view(ints)), f"{what} rank {r}: bytes differ from rank 0's"
    if fdt == E4M3:  # exact in float32 in any order: pins the operand set apart from the order (check_fold)
        exact = xs[-1].view(fdt).to(torch.float64)
        for x in xs[-2::-1]:
            exact = exact + x.view(fdt).to(torch.float64)
        assert same(outs[0], exact.to(torch.float32).to(odt)), f"{what}: differs from the exact sum"


def misaligned_buffers(comms):
    """sendBuf one byte and recvBuf one element off 16-byte alignment: the element-wise path to all destinations."""
    n, count, fdt, odt, guard = 2, 40001, E4M3, torch.bfloat16, 8
    xs = inputs(n, AR, count)
    sends = [torch.cat([x[:1], x]).cuda()[1:].view(fdt) for x in xs]
    raws = [torch.full((count + 2 * guard + 1,), -7.0, dtype=odt, device="cuda") for _ in range(n)]
    recvs = [t[guard + 1:guard + 1 + count] for t in raws]
    assert all(t.data_ptr() % 16 != 0 for t in sends + recvs)
    run_checked(comms, fdt, odt, xs, count, "misaligned", sends=sends, recvs=recvs)
    for t in raws:
        assert bool((t[:guard + 1] == -7.0).all()) and bool((t[guard + 1 + count:] == -7.0).all()), "guards written"


def several_rounds(monkeypatch):
    """16 MiB areas, three ranks, FP32 output: a slot holds 1,398,100 elements, so 8.4 M elements take three rounds
    (asserted from the planner before anything runs) and slots and result areas are used again."""
    monkeypatch.setenv("HCCL_AMD_IPC_STAGING_MIB", "16")
    n, count = 3, 8_400_003
    _, launches = H.ipc_plan(H.OpType.ALLREDUCE, n, count, H.HcclDataType.FP32, family=int(H.Algo.MESH_TWOSHOT),
                             sharedDevice=1)
    assert len(launches) == 1 and launches[0].rounds >= 3, launches[0].rounds
    with world(n) as comms:
        run_checked(comms, E5M2, torch.float32, inputs(n, AR, count), count, "three rounds")


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
        count, fdt, odt, out = 5001, E4M3, torch.bfloat16, []
        xs = inputs(2, AR, count)
        send = xs[rank].cuda().view(fdt)
        for algo in (None, H.Algo.IPC_TWOSHOT):  # the creation default must not take the two-shot kernel
            if algo is not None:
                comm.set_algo(algo)
            recv = torch.full((count,), -7.0, dtype=odt, device="cuda")
            torch.cuda.synchronize()
            comm.all_reduce_widen(send, recv, stream)
            stream.synchronize()
            out.append((same(recv.cpu(), expected(xs, fdt, odt)), comm.last_algo, comm.ipc_status() & 0xFF))
        dist.barrier()
        comm.destroy()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc()))


def two_processes_on_one_gpu():
    """Rank mode. At n = 2 with exact E4M3 sums O1 gives the O2 values, so the call before set_algo is checked alike."""
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(2):
        assert got[r] == [(True, int(H.Algo.IPC), 0), (True, int(H.Algo.IPC_TWOSHOT), 0)], (r, got[r])


def test_two_shot_widened_all_reduce(monkeypatch):
    """One test id (the suite's count of test ids is kept low); the failing case is in the message. Counts: one element
    (every chunk but the first empty); 33 (at n = 8 one full chunk, one element, six empty); a ragged last chunk behind
    the 128-B rounded stride; several block windows."""
    for n in (2, 3, 8):
        with world(n) as comms:
            for fdt, odt in ((E5M2, torch.float32), (E4M3, torch.bfloat16), (E4M3, torch.float16)):
                for count in (1, 33, 1000, 40000):
                    run_checked(comms, fdt, odt, inputs(n, AR, count), count, f"n {n} {fdt} -> {odt} count {count}")
            if n == 2:
                misaligned_buffers(comms)
    several_rounds(monkeypatch)
    two_processes_on_one_gpu()
