"""dist.all_to_all_single (even and uneven splits) and dist.all_to_all over the "hccl" backend: HcclAlltoAll and
HcclAlltoAllV on the tensors' bytes. Two processes share the GPU (the backend's IPC transport, as
tests/test_gpu_process_group_broadcast.py); every rank builds every rank's inputs from seeds and checks its outputs
against the expectation computed with torch.
"""
import datetime
import multiprocessing as mp
import os
import socket
import time
import traceback

import pytest

pytestmark = pytest.mark.gpu


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

        def data(seed, shape, dtype):
            g = torch.Generator(device="cuda").manual_seed(777 + seed)
            nbytes = torch.empty(shape, dtype=dtype).numel() * torch.empty(0, dtype=dtype).element_size()
            raw = torch.randint(0, 256, (max(nbytes, 1),), dtype=torch.uint8, device="cuda", generator=g)[:nbytes]
            return raw.view(dtype).reshape(shape).clone()

        def same(a, b):
            return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))

        # even splits: rows [q * k, (q + 1) * k) of rank p's input arrive as rows [p * k, (p + 1) * k) on rank q
        for name, dtype, k, cols in (("even_bf16", torch.bfloat16, 3, 7), ("even_f64", torch.float64, 1000, 1)):
            ins = [data(10 + p, (n * k, cols), dtype) for p in range(n)]
            out = torch.zeros_like(ins[rank])
            dist.all_to_all_single(out, ins[rank])
            torch.cuda.synchronize()
            want = torch.cat([ins[p][rank * k:(rank + 1) * k] for p in range(n)])
            checks[name] = same(out, want)
        # uneven splits in rows of 5 int16: split[p][q] rows from p to q (zero included)
        split = [[4099, 0], [3, 17]]
        ins = [data(20 + p, (sum(split[p]), 5), torch.int16) for p in range(n)]
        out = torch.zeros((sum(split[p][rank] for p in range(n)), 5), dtype=torch.int16, device="cuda")
        dist.all_to_all_single(out, ins[rank], [split[p][rank] for p in range(n)], split[rank])
        torch.cuda.synchronize()
        off = [[sum(split[p][:q2]) for q2 in range(n)] for p in range(n)]
        want = torch.cat([ins[p][off[p][rank]:off[p][rank] + split[p][rank]] for p in range(n)])
        checks["uneven_single"] = same(out, want)
        # dist.all_to_all: a list of tensors of different sizes, one of them empty
        sizes = [[5, 70001], [0, 33]]
        ins = [[data(30 + p * n + q2, (sizes[p][q2],), torch.float32) for q2 in range(n)] for p in range(n)]
        outs = [torch.zeros(sizes[p][rank], dtype=torch.float32, device="cuda") for p in range(n)]
        dist.all_to_all(outs, ins[rank])
        torch.cuda.synchronize()
        checks["list"] = all(same(outs[p], ins[p][rank]) for p in range(n))
        # mismatched dtypes are refused before anything is enqueued
        try:
            dist.all_to_all_single(torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
            checks["dtype_mismatch_refused"] = False
        except ValueError:
            checks["dtype_mismatch_refused"] = True
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", checks))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        time.sleep(10)


def test_dist_all_to_all_world_2():
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
        assert all(res.values()), f"rank {r}: {res}"
