"""dist.broadcast over the "hccl" backend: HcclBroadcast on the tensor's bytes, in place, with no temporary.

Two processes share the GPU (the backend's IPC transport, as tests/test_gpu_process_group.py). The memory check is the
point of the operator: the AllGather-based broadcast it replaces allocated world_size x bytes (128 MiB for the 64 MiB
tensor here); a Broadcast of its own allocates nothing in the caching allocator.
"""
import datetime
import multiprocessing as mp
import os
import socket
import time
import traceback

import pytest

pytestmark = pytest.mark.gpu

SRC = 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, n, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"
    os.environ["HCCL_AMD_PG_TRANSPORT"] = "ipc"
    try:
        import torch
        import torch.distributed as dist
        import hccl_amd.process_group  # noqa: F401  (registers backend "hccl")

        torch.cuda.set_device(0)
        dist.init_process_group(backend="hccl", rank=rank, world_size=n, init_method=f"tcp://127.0.0.1:{port}",
                                timeout=datetime.timedelta(seconds=120))
        checks = {}
        g = torch.Generator(device="cuda")

        def data(seed_rank, shape, dtype):
            g.manual_seed(4242 + seed_rank)
            nbytes = max(1, torch.empty(shape, dtype=dtype).numel() * torch.empty(0, dtype=dtype).element_size())
            raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
            if dtype == torch.bool:
                raw = raw & 1
            return raw.view(dtype).reshape(shape).clone()

        for name, shape, dtype in (("bf16", (333, 7), torch.bfloat16), ("int64", (5001,), torch.int64),
                                   ("bool", (4099,), torch.bool), ("zero_dim", (), torch.float32)):
            t = data(rank, shape, dtype)
            want = data(SRC, shape, dtype)
            dist.broadcast(t, src=SRC)
            torch.cuda.synchronize()
            checks[name] = bool(torch.equal(t.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8)))
        # a non-contiguous tensor is still refused
        try:
            dist.broadcast(torch.zeros(8, 8, device="cuda").t(), src=SRC)
            checks["non_contiguous_refused"] = False
        except ValueError:
            checks["non_contiguous_refused"] = True
        # 64 MiB: the peak of the caching allocator rises by less than 32 MiB around the call
        big = torch.full((64 << 20,), rank + 1, dtype=torch.uint8, device="cuda")
        dist.broadcast(torch.zeros(1024, device="cuda"), src=SRC)  # anything set up lazily is set up by now
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        dist.broadcast(big, src=SRC)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        checks["big_exact"] = bool((big == SRC + 1).all())
        checks["rise_bytes"] = rise
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", checks))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)


def test_dist_broadcast_world_2():
    n = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, n, port, q)) for r in range(n)]
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
    for r in range(n):
        msg, res = got[r]
        assert msg == "ok", f"rank {r}: {msg}"
        rise = res.pop("rise_bytes")
        assert all(res.values()), f"rank {r}: {res}"
        assert rise < (32 << 20), f"rank {r}: max_memory_allocated rose by {rise} B around a 64 MiB broadcast"
