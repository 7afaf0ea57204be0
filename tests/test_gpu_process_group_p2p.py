"""dist.send / dist.recv and isend / irecv().wait() over the "hccl" backend at world 2: HcclSend and HcclRecv on the
tensors' bytes. The processes share the GPU (the backend's IPC transport, as
tests/test_gpu_process_group_scatter_gatherv.py), which has no send/recv of its own, so HCCL_AMD_P2P_IPC=1 makes the
backend call HcclAmdCommEnableP2p when it creates the communicator and every message runs on the one-sided kernel.
"""
import datetime
import multiprocessing as mp
import os
import traceback

import pytest

from test_gpu_process_group_alltoall import _free_port

pytestmark = pytest.mark.gpu


def _rank_main(rank, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"
    os.environ["HCCL_AMD_PG_TRANSPORT"] = "ipc"
    os.environ["HCCL_AMD_P2P_IPC"] = "1"
    try:
        import torch
        import torch.distributed as dist
        import hccl_amd.process_group  # noqa: F401  (registers backend "hccl")

        torch.cuda.set_device(0)
        dist.init_process_group(backend="hccl", rank=rank, world_size=2, init_method=f"tcp://127.0.0.1:{port}",
                                timeout=datetime.timedelta(seconds=120))
        checks, peer = {}, 1 - rank

        def data(seed, shape, dtype):
            g = torch.Generator().manual_seed(777 + seed)
            nbytes = torch.empty(shape, dtype=dtype).numel() * torch.empty(0, dtype=dtype).element_size()
            return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g).cuda().view(dtype).reshape(shape)

        def same(a, b):
            return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))

        # blocking calls, both directions in turn; the second message is longer than two slots
        for k, (src, shape, dtype) in enumerate([(0, (3, 7), torch.bfloat16), (1, (300001,), torch.float32),
                                                 (0, (1,), torch.uint8)]):
            if rank == src:
                dist.send(data(k, shape, dtype), dst=peer)
            else:
                got = torch.zeros(shape, dtype=dtype, device="cuda")
                dist.recv(got, src=peer)
                torch.cuda.synchronize()
                checks[f"send_recv_{k}"] = same(got, data(k, shape, dtype))
        # isend / irecv: two messages in flight on the pair, matched in call order
        shapes = [(4099,), (5, 5)]
        if rank == 0:
            works = [dist.isend(data(10 + k, s, torch.float16), dst=1) for k, s in enumerate(shapes)]
        else:
            outs = [torch.zeros(s, dtype=torch.float16, device="cuda") for s in shapes]
            works = [dist.irecv(o, src=0) for o in outs]
        for w in works:
            w.wait()
        torch.cuda.synchronize()
        if rank == 1:
            checks["isend_irecv"] = all(same(o, data(10 + k, s, torch.float16)) for k, (o, s) in enumerate(zip(outs, shapes)))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", checks))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))


def test_dist_send_recv_and_isend_irecv():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in procs:
            rank, msg, res = q.get(timeout=240)
            got[rank] = (msg, res)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(2):
        msg, res = got[r]
        assert msg == "ok", f"rank {r}: {msg}"
        assert res and all(res.values()), f"rank {r}: {res}"
