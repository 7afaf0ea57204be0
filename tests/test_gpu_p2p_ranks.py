"""The one-sided point-to-point path in RANK mode: two spawned processes sharing the GPU on host-exchange communicators
(as tests/test_gpu_ipc_ranks.py sets them up), each side launching its own lanes of k_ipc_p2p, the peer's area opened
from its IPC handle. Before enable_p2p() the three operators have no path there (HCCL_E_NOT_SUPPORT); after it a
ping-pong of three messages (one longer than two slots, so its sender needs the receiver's credit), a batch in which
both ranks send and receive at once, and one Send / Recv pair captured into a HIP graph and replayed three times with
new data: the piece counters live on the device, so every replay takes the next pieces. Every message is matched."""
import datetime
import multiprocessing as mp
import os
import traceback

import pytest

from test_gpu_ipc_ranks import _free_port

pytestmark = pytest.mark.gpu

SLOT = 256 << 10


def _rank_main(rank, port, q):
    os.environ["HCCL_AMD_IPC_TIMEOUT_MS"] = "20000"  # a lost peer shows as a status bit, never a hang
    try:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)
        import hccl_amd as H

        def all_gather(b):
            out = [None] * 2
            dist.all_gather_object(out, b)
            return out

        def data(seed, count):
            g = torch.Generator().manual_seed(seed)
            return torch.randint(-2**31, 2**31 - 1, (count,), dtype=torch.int32, generator=g).cuda()

        comm = H.comm_init_host_exchange(2, rank, all_gather)
        stream = torch.cuda.Stream()
        peer, out = 1 - rank, {}
        buf = torch.zeros(8, dtype=torch.int32, device="cuda")
        codes = []
        for call in (lambda: comm.send(buf, peer, stream), lambda: comm.recv(buf, peer, stream),
                     lambda: comm.batch_send_recv([(H.SendRecvType.SEND, buf, peer)], stream)):
            try:
                call()
                codes.append(0)
            except H.HcclError as e:
                codes.append(e.code)
        out["before"] = codes
        before = comm.device_bytes()
        comm.enable_p2p()
        plan = H.p2p_plan(0, 1, SLOT, 2)
        out["grown"] = comm.device_bytes() - before - (plan.areaBytes + plan.counterBytes)  # the base set-up's share
        # ping-pong: 0 -> 1, 1 -> 0, 0 -> 1; the second is longer than two slots
        ok = True
        for k, (src, count) in enumerate([(0, 1000), (1, 2 * SLOT // 4 + 5), (0, SLOT // 4 + 1)]):
            if rank == src:
                comm.send(data(100 + k, count), peer, stream)
            else:
                got = torch.zeros(count, dtype=torch.int32, device="cuda")
                comm.recv(got, peer, stream)
                stream.synchronize()
                ok = ok and torch.equal(got, data(100 + k, count))
        out["pingpong"] = ok
        out["algo"] = comm.last_algo
        # a batch: both ranks send two messages and receive two, listed in different orders on the two sides
        counts = [3 * SLOT // 4 + 7, 11]
        sends = [data(200 + rank * 10 + k, c) for k, c in enumerate(counts)]
        recvs = [torch.zeros(c, dtype=torch.int32, device="cuda") for c in counts]
        items = [(H.SendRecvType.SEND, t, peer) for t in sends] + [(H.SendRecvType.RECV, t, peer) for t in recvs]
        comm.batch_send_recv(items if rank == 0 else items[::-1], stream)
        stream.synchronize()
        out["batch"] = all(torch.equal(recvs[k], data(200 + peer * 10 + k, c)) for k, c in enumerate(counts))
        # one pair captured into a graph, replayed three times with new data (3 pieces per replay)
        count = 2 * SLOT // 4 + 9
        box = torch.zeros(count, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            if rank == 0:
                comm.send(box, 1, stream)
            else:
                comm.recv(box, 0, stream)
        replays = []
        for k in range(3):
            if rank == 0:
                box.copy_(data(300 + k, count))
            else:
                box.zero_()
            torch.cuda.synchronize()
            dist.barrier()
            g.replay()
            torch.cuda.synchronize()
            dist.barrier()  # the sender's buffer is rewritten only after the receiver has it
            replays.append(rank == 0 or torch.equal(box, data(300 + k, count)))
        out["replays"] = replays
        out["status"] = comm.ipc_status() & 0xFF
        out["async"] = comm.async_error()
        del g
        comm.destroy()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:  # noqa: BLE001
        q.put((rank, {"error": traceback.format_exc()}))


def test_two_processes_ping_pong_batch_and_graph_replay():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(2):
        out = got[r]
        assert "error" not in out, out.get("error")
        assert out["before"] == [5, 5, 5], out  # HCCL_E_NOT_SUPPORT: no transport, and p2p not enabled
        assert out["grown"] >= 0 and out["pingpong"] and out["batch"], out
        assert out["algo"] == 9 and out["replays"] == [True, True, True], out
        assert out["status"] == 0 and out["async"] == 0, out
