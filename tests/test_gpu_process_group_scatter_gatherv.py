"""dist.scatter and dist.all_gather with outputs of unequal sizes over the "hccl" backend: HcclScatter and HcclAllGatherV
on the tensors' bytes. The processes share the GPU (the backend's IPC transport, as
tests/test_gpu_process_group_alltoall.py); every rank builds every rank's inputs from seeds and checks its outputs
against the expectation computed with torch. The equal-size all_gather keeps its own path and result.
"""
import datetime
import multiprocessing as mp
import os
import time
import traceback

import pytest

from test_gpu_process_group_alltoall import _free_port

pytestmark = pytest.mark.gpu


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

        def data(seed, shape, dtype):
            g = torch.Generator(device="cuda").manual_seed(4242 + seed)
            nbytes = torch.empty(shape, dtype=dtype).numel() * torch.empty(0, dtype=dtype).element_size()
            raw = torch.randint(0, 256, (max(nbytes, 1),), dtype=torch.uint8, device="cuda", generator=g)[:nbytes]
            return raw.view(dtype).reshape(shape).clone()

        def same(a, b):
            return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))

        # dist.scatter from the last rank and from rank 0: every rank knows the source's list from the seeds
        for name, src, dtype, shape in (("scatter_bf16", n - 1, torch.bfloat16, (3, 7)),
                                        ("scatter_f64", 0, torch.float64, (4099,)),
                                        ("scatter_u8", n - 1, torch.uint8, (1,))):
            parts = [data(100 + q2, shape, dtype) for q2 in range(n)]
            out = torch.zeros(shape, dtype=dtype, device="cuda")
            dist.scatter(out, [p.clone() for p in parts] if rank == src else None, src=src)
            torch.cuda.synchronize()
            checks[name] = same(out, parts[rank])
        # dist.all_gather with outputs of unequal sizes, one of them empty
        sizes = [(4099 if r == 1 else 0 if r == n - 1 and n > 2 else 5 + 3 * r) for r in range(n)]
        ins = [data(200 + r, (sizes[r],), torch.float16) for r in range(n)]
        outs = [torch.zeros(sizes[r], dtype=torch.float16, device="cuda") for r in range(n)]
        dist.all_gather(outs, ins[rank])
        torch.cuda.synchronize()
        checks["uneven_all_gather"] = all(same(outs[r], ins[r]) for r in range(n))
        # the equal-size all_gather as before
        ins = [data(300 + r, (33, 5), torch.int32) for r in range(n)]
        outs = [torch.zeros((33, 5), dtype=torch.int32, device="cuda") for _ in range(n)]
        dist.all_gather(outs, ins[rank])
        torch.cuda.synchronize()
        checks["equal_all_gather"] = all(same(outs[r], ins[r]) for r in range(n))
        # an output of another dtype is refused before anything is enqueued
        try:
            bad = [torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(n)]
            dist.all_gather(bad, torch.zeros(4, device="cuda"))
            checks["dtype_mismatch_refused"] = False
        except ValueError:
            checks["dtype_mismatch_refused"] = True
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", checks))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)


@pytest.mark.parametrize("n", [2, 4])
def test_dist_scatter_and_uneven_all_gather(n):
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
        assert all(res.values()), f"rank {r}: {res}"
