"""The cross-rank argument check (HCCL_DFS_CONFIG=inconsistent_check; k_ipc_check) in loopback worlds of 2 and 4 ranks.

Every communicator runs the one-sided family (Algo.IPC), so that after a failed check nothing is left waiting in a
transport: the launches queued behind the check return at once on the sticky bit. HCCL_AMD_IPC_TIMEOUT_MS is 20000: a
broken protocol shows as a status bit and a failed assertion, never a hang; a mismatch must be reported in well under
that (5 s of wall time are granted, the check itself takes microseconds).
"""
import ctypes
import time

import pytest
import torch

import hccl_amd as H
from hccl_amd import Config, HcclResult
from tests.test_gpu_collectives import run_ranks

pytestmark = pytest.mark.gpu

IPC = int(H.Algo.IPC)
SUM, MAX = int(H.HcclReduceOp.SUM), int(H.HcclReduceOp.MAX)
AREA_BYTES = 2 * 16 * 11 * 8  # two parities of HCCL_AMD_IPC_MAX_RANKS records of 11 words, 8 bytes per word
PRIV_BYTES = 6 * 8            # the sequence counter and the report
OFF, FIRST, ON = -1, 0, 1


@pytest.fixture(autouse=True)
def bounded_waits(monkeypatch):
    monkeypatch.setenv("HCCL_AMD_IPC_TIMEOUT_MS", "20000")


def world(n, mode):
    comms = H.loopback_world(n)
    for c in comms:
        c.set_algo(IPC)
        c.set_config(Config.INCONSISTENT_CHECK, mode)
    return comms


def destroy(comms):
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()


def sequence(n, mode):
    """AllReduce fp32 sum of 4099 elements, Broadcast of 33 bytes, AlltoAllV with ragged counts, Barrier,
    ReduceScatterV with ragged counts, enqueued back to back by every rank. Returns the outputs as host tensors, the
    device bytes held and the check launches of every rank."""
    comms = world(n, mode)
    try:
        g = torch.Generator().manual_seed(77)
        ar_in = [torch.randn(4099, generator=g).cuda() for _ in range(n)]
        ar_out = [torch.zeros(4099, device="cuda") for _ in range(n)]
        bc = [torch.randint(0, 255, (33,), generator=g, dtype=torch.uint8).cuda() for _ in range(n)]
        cnt = [[(3 * p + 5 * q) % 7 + (p != q) for q in range(n)] for p in range(n)]  # p sends cnt[p][q] to q
        a2a_in = [torch.randint(0, 1 << 20, (sum(cnt[p]),), generator=g, dtype=torch.int32).cuda() for p in range(n)]
        a2a_out = [torch.zeros(sum(cnt[p][q] for p in range(n)), dtype=torch.int32, device="cuda") for q in range(n)]
        rs_counts = [5 + 3 * q for q in range(n)]
        rs_displs = [sum(rs_counts[:q]) for q in range(n)]
        rs_in = [torch.randn(sum(rs_counts), generator=g).cuda() for _ in range(n)]
        rs_out = [torch.zeros(rs_counts[r], device="cuda") for r in range(n)]
        streams = [torch.cuda.Stream() for _ in range(n)]
        torch.cuda.synchronize()

        def body(r):
            c, s = comms[r], streams[r]
            c.all_reduce(ar_in[r], ar_out[r], SUM, s)
            c.broadcast(bc[r], n - 1, s)
            sc = cnt[r]
            rc = [cnt[p][r] for p in range(n)]
            c.alltoall_v(a2a_in[r], sc, [sum(sc[:q]) for q in range(n)], a2a_out[r], rc,
                         [sum(rc[:q]) for q in range(n)], s)
            c.barrier(s)
            c.reduce_scatter_v(rs_in[r], rs_counts, rs_displs, rs_out[r], SUM, s)

        run_ranks(n, body)
        torch.cuda.synchronize()
        assert all(c.async_error() == HcclResult.HCCL_SUCCESS for c in comms)
        assert all(c.inconsistency() is None for c in comms)
        assert all(c.ipc_status() & 3 == 0 for c in comms)
        outs = [t.cpu() for ts in (ar_out, bc, a2a_out, rs_out) for t in ts]
        return outs, [c.device_bytes() for c in comms], [c.check_launches() for c in comms]
    finally:
        destroy(comms)


@pytest.mark.parametrize("n", [2, 4])
def test_consistent_sequence_is_unchanged_and_costs_the_documented_bytes(n):
    off, bytes_off, launches_off = sequence(n, OFF)
    on, bytes_on, launches_on = sequence(n, ON)
    assert len(off) == len(on) and all(torch.equal(a, b) for a, b in zip(off, on))
    # the sequence did something: the AllReduce's result is the sum, the Broadcast's the root's bytes
    assert not torch.equal(on[0], torch.zeros(4099)) and all(torch.equal(on[n + r], on[n]) for r in range(n))
    assert [b - a for a, b in zip(bytes_off, bytes_on)] == [AREA_BYTES + PRIV_BYTES] * n
    # switch off: no check was launched and nothing of the check is held (the parent commit's launch sequence)
    assert launches_off == [0] * n
    assert launches_on == [5] * n  # one check per checked call, counted by the device's own sequence word


def mismatch_cases(n):
    """name -> (the call of rank r, the report expected on rank r: peer, field name, local, remote). Rank n - 1 is the
    one that differs, so every other rank names it, and it names rank 0 (the lowest peer that differs from it)."""
    odd = n - 1
    f32, i32 = int(H.HcclDataType.FP32), int(H.HcclDataType.INT32)

    def expect(name, usual, other):
        return lambda r: (0, name, other, usual) if r == odd else (odd, name, usual, other)

    def bufs(dtype=torch.float32, count=4100):
        return torch.ones(count, dtype=dtype, device="cuda"), torch.zeros(n * count, dtype=dtype, device="cuda")

    def count_case(c, r, s):
        x, y = bufs()
        k = 4100 if r == odd else 4099
        c.all_reduce(x[:k], y[:k], SUM, s)

    def dtype_case(c, r, s):
        x, y = bufs(torch.int32 if r == odd else torch.float32)
        c.all_reduce(x[:4099], y[:4099], SUM, s)

    def op_case(c, r, s):
        x, y = bufs()
        c.all_reduce(x[:4099], y[:4099], MAX if r == odd else SUM, s)

    def root_case(c, r, s):
        x, _ = bufs(torch.uint8, 33)
        c.broadcast(x, 1 if r == odd else 0, s)

    def operator_case(c, r, s):
        x, y = bufs()
        if r == odd:
            c.all_gather(x[:4099], y[:n * 4099], s)
        else:
            c.all_reduce(x[:4099], y[:4099], SUM, s)

    return {
        "count": (count_case, expect("DataCount", 4099, 4100)),
        "dtype": (dtype_case, expect("HcclDataType", f32, i32)),
        "op": (op_case, expect("HcclReduceOp", SUM, MAX)),
        "root": (root_case, expect("RootRankId", 0, 1)),
        "operator": (operator_case, expect("OpType", int(H.OpType.ALLREDUCE), int(H.OpType.ALLGATHER))),
    }


@pytest.mark.parametrize("case", ["count", "dtype", "op", "root", "operator"])
@pytest.mark.parametrize("n", [2, 4])
def test_one_rank_differs(n, case):
    call, expect = mismatch_cases(n)[case]
    comms = world(n, ON)
    try:
        streams = [torch.cuda.Stream() for _ in range(n)]
        x = [torch.ones(64, device="cuda") for _ in range(n)]
        y = [torch.zeros(64, device="cuda") for _ in range(n)]
        g_in = [torch.ones(4099, device="cuda") for _ in range(n)]
        g_out = [torch.zeros(n * 4099, device="cuda") for _ in range(n)]

        def warm_up(r):
            # The collective set-ups, and two checks that pass. The staging tier too, which the AllGather of the
            # operator case needs and the AllReduce it meets (LL form) does not: a set-up is a host rendezvous of all
            # ranks, which ranks that disagree about the operator would not enter together. The check is stream-ordered
            # and cannot stand in front of a host rendezvous.
            comms[r].all_reduce(x[r], y[r], SUM, streams[r])
            comms[r].all_gather(g_in[r], g_out[r], streams[r])

        run_ranks(n, warm_up)
        torch.cuda.synchronize()
        assert all(c.async_error() == HcclResult.HCCL_SUCCESS for c in comms)
        assert [c.check_launches() for c in comms] == [2] * n
        t0 = time.monotonic()
        run_ranks(n, lambda r: call(comms[r], r, streams[r]))
        torch.cuda.synchronize()
        errors = [c.async_error() for c in comms]
        reports = [c.inconsistency() for c in comms]
        wall = time.monotonic() - t0
        print(f"n={n} {case}: {wall:.3f} s, reports {reports}")
        assert errors == [HcclResult.HCCL_E_PARA] * n
        for r in range(n):
            peer, name, local, remote = expect(r)
            assert reports[r] is not None, r
            got = (reports[r]["peer"], reports[r]["name"], reports[r]["local"], reports[r]["remote"])
            assert got == (peer, name, local, remote), (r, got)
        assert wall < 5.0
        assert all(c.ipc_status() & 3 == 3 for c in comms)  # the sticky bit and "inconsistent arguments"
        # the next collective entry returns the error itself, later ones the status gate's
        for want in (HcclResult.HCCL_E_PARA, HcclResult.HCCL_E_SUSPENDING, HcclResult.HCCL_E_SUSPENDING):
            for r in range(n):
                with pytest.raises(H.HcclError) as e:
                    comms[r].all_reduce(x[r], y[r], SUM, streams[r])
                assert e.value.code == want, (r, want)
    finally:
        destroy(comms)


def test_first_mode_checks_each_operator_type_once():
    n = 2
    comms = world(n, FIRST)
    try:
        streams = [torch.cuda.Stream() for _ in range(n)]
        x = [torch.ones(4 * n, device="cuda") for _ in range(n)]
        y = [torch.zeros(4 * n, device="cuda") for _ in range(n)]
        z = [torch.zeros(4, device="cuda") for _ in range(n)]
        seen = []
        for step in ("ar", "ar", "rs", "ar", "rs"):
            if step == "ar":
                run_ranks(n, lambda r: comms[r].all_reduce(x[r], y[r], SUM, streams[r]))
            else:
                run_ranks(n, lambda r: comms[r].reduce_scatter(x[r], z[r], SUM, streams[r]))
            torch.cuda.synchronize()
            seen.append([c.check_launches() for c in comms])
        # the first AllReduce and the first ReduceScatter launch a check, the others none
        assert seen == [[1] * n, [1] * n, [2] * n, [2] * n, [2] * n]
        assert all(torch.equal(t, torch.full((4 * n,), float(n), device="cuda")) for t in y)
        assert all(c.async_error() == HcclResult.HCCL_SUCCESS for c in comms)
    finally:
        destroy(comms)


def test_switch_off_launches_nothing_and_holds_nothing():
    """Unset means off: the configuration says -1, no check runs, and the communicator holds what it held without the
    feature: the flags and LL area, the status words and the unpack area of the first one-sided call (a 64-element
    AllReduce takes the LL form and no staging tier)."""
    n = 2
    comms = H.loopback_world(n)
    try:
        assert all(c.get_config(Config.INCONSISTENT_CHECK) == OFF for c in comms)
        for c in comms:
            c.set_algo(IPC)
        streams = [torch.cuda.Stream() for _ in range(n)]
        x = [torch.ones(64, device="cuda") for _ in range(n)]
        y = [torch.zeros(64, device="cuda") for _ in range(n)]
        run_ranks(n, lambda r: comms[r].all_reduce(x[r], y[r], SUM, streams[r]))
        torch.cuda.synchronize()
        flags = 512 * 16 * 4 + 2 * 16 * 2 * (64 << 10)  # kIpcFlagBytes + 2 x kIpcLlParityBytes
        unpack = 16 * ((64 << 10) + 256)                # kIpcLlUnpackBytes
        assert [c.device_bytes() for c in comms] == [flags + 32 + unpack] * n
        assert [c.check_launches() for c in comms] == [0] * n
        assert comms[0].ipc_ll_launches() == 1
        for c in comms:
            with pytest.raises(H.HcclError) as e:
                c.set_config(Config.INCONSISTENT_CHECK, 2)
            assert e.value.code == HcclResult.HCCL_E_PARA
    finally:
        destroy(comms)


def test_capture_in_a_loopback_world_reports_what_the_data_path_reports():
    """A loopback world exchanges events between host threads per call, which no capture can hold: a captured checked
    call answers HCCL_E_NOT_SUPPORT, as the same call does with the switch off, and launches no check."""
    n = 2
    hip = ctypes.CDLL("libamdhip64.so")
    for mode in (OFF, ON):
        comms = world(n, mode)
        try:
            streams = [torch.cuda.Stream() for _ in range(n)]
            x = [torch.ones(64, device="cuda") for _ in range(n)]
            y = [torch.zeros(64, device="cuda") for _ in range(n)]
            run_ranks(n, lambda r: comms[r].all_reduce(x[r], y[r], SUM, streams[r]))
            torch.cuda.synchronize()
            before = [c.check_launches() for c in comms]
            codes = [None] * n
            # the refusal comes before any rendezvous, so the ranks can be asked one after another on this thread
            for r in range(n):
                handle, graph = ctypes.c_void_p(streams[r].cuda_stream), ctypes.c_void_p()
                assert hip.hipStreamBeginCapture(handle, 1) == 0  # hipStreamCaptureModeThreadLocal
                try:
                    comms[r].all_reduce(x[r], y[r], SUM, streams[r])
                except H.HcclError as e:
                    codes[r] = e.code
                finally:
                    assert hip.hipStreamEndCapture(handle, ctypes.byref(graph)) == 0
                assert hip.hipGraphDestroy(graph) == 0
            torch.cuda.synchronize()
            assert codes == [HcclResult.HCCL_E_NOT_SUPPORT] * n, (mode, codes)
            assert [c.check_launches() for c in comms] == before
        finally:
            destroy(comms)
