"""HcclScatter and HcclAllGatherV at the ABI: the symbols exist with the reference's argument order (a plain C caller
assigns them to function pointers of the reference's prototypes, include/hccl.h:104-106 and 138-140 there, and links),
and every argument check returns the reference's code in the reference's order (scatter_op.cc:70-84, 126-139;
all_gather_v_op.cc:40-54, 136-188), plus the two additions of HcclAllGatherV that include/hccl.h documents. The checks
that come before the communicator is looked at run anywhere; the others need a loopback communicator and so a GPU."""
import ctypes
import os
import subprocess

import pytest

import hccl_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, E = H.lib, H.HcclResult
U8, INT128 = H.HcclDataType.UINT8, 13
P, P2 = 0x1000, 0x2000  # never dereferenced
SYS_MAX_COUNT = 0x7FFFFFFFF

C_CALLER = r"""
#include <stdint.h>
#include <stdio.h>
#include "hccl.h"
typedef HcclResult (*ScatterFn)(void*, void*, uint64_t, HcclDataType, uint32_t, HcclComm, aclrtStream);
typedef HcclResult (*AllGatherVFn)(void*, uint64_t, void*, const void*, const void*, HcclDataType, HcclComm,
                                   aclrtStream);
int main(void)
{
    ScatterFn scatter = HcclScatter;
    AllGatherVFn gatherv = HcclAllGatherV;
    uint64_t arr[2] = {0, 0};
    char buf[8];
    if (scatter(NULL, NULL, 0, HCCL_DATA_TYPE_INT8, 0, NULL, NULL) != HCCL_SUCCESS) return 1;
    if (scatter(buf, buf, 8, HCCL_DATA_TYPE_INT8, 0, NULL, (aclrtStream)buf) != HCCL_E_PTR) return 2;
    if (gatherv(buf, 8, buf, arr, arr, HCCL_DATA_TYPE_INT8, NULL, (aclrtStream)buf) != HCCL_E_PTR) return 3;
    if (gatherv(NULL, 8, buf, arr, arr, HCCL_DATA_TYPE_INT8, (HcclComm)buf, (aclrtStream)buf) != HCCL_E_PTR) return 4;
    puts("OK");
    return 0;
}
"""


def test_c_caller_links_with_the_reference_prototypes(tmp_path):
    src, exe = tmp_path / "caller.c", tmp_path / "caller"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(H.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe), "-L", libdir, "-lhccl_amd", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "OK", (out.returncode, out.stdout, out.stderr)
    assert len(H.SIGNATURES["HcclScatter"][1]) == 7
    assert len(H.SIGNATURES["HcclAllGatherV"][1]) == 8
    assert len(H.SIGNATURES["HcclAmdBuildScheduleAllGatherV"][1]) == 11


def test_checks_before_the_communicator():
    # HcclScatter: recvCount 0 before anything else, then comm, recvBuf, stream
    assert L.HcclScatter(None, None, 0, U8, 99, None, None) == E.HCCL_SUCCESS
    assert L.HcclScatter(P, P2, 8, U8, 0, None, P) == E.HCCL_E_PTR    # comm
    assert L.HcclScatter(P, None, 8, U8, 0, P, P) == E.HCCL_E_PTR     # recvBuf
    assert L.HcclScatter(P, P2, 8, U8, 0, P, None) == E.HCCL_E_PTR    # stream
    # HcclAllGatherV: comm, recvCounts, recvDispls, stream, then sendBuf when sendCount > 0
    arr = (ctypes.c_uint64 * 4)()
    assert L.HcclAllGatherV(P, 8, P2, arr, arr, U8, None, P) == E.HCCL_E_PTR   # comm
    assert L.HcclAllGatherV(P, 8, P2, None, arr, U8, P, P) == E.HCCL_E_PTR     # recvCounts
    assert L.HcclAllGatherV(P, 8, P2, arr, None, U8, P, P) == E.HCCL_E_PTR     # recvDispls
    assert L.HcclAllGatherV(P, 8, P2, arr, arr, U8, P, None) == E.HCCL_E_PTR   # stream
    assert L.HcclAllGatherV(None, 8, P2, arr, arr, U8, P, P) == E.HCCL_E_PTR   # sendBuf with sendCount > 0
    # the schedule export's own checks
    n_ops = ctypes.c_uint64(0)
    assert L.HcclAmdBuildScheduleAllGatherV(2, 0, arr, None, 0, U8, 0, None, 0, ctypes.byref(n_ops),
                                            None) == E.HCCL_E_PTR
    assert L.HcclAmdBuildScheduleAllGatherV(2, 2, arr, arr, 0, U8, 0, None, 0, ctypes.byref(n_ops),
                                            None) == E.HCCL_E_PARA
    big = (ctypes.c_uint64 * 2)(1, (1 << 64) - 1)
    assert L.HcclAmdBuildScheduleAllGatherV(2, 0, big, big, 0, U8, 0, None, 0, ctypes.byref(n_ops),
                                            None) == E.HCCL_E_PARA  # a block's end does not fit 64 bits


@pytest.mark.gpu
def test_checks_on_a_loopback_communicator():
    """Every check returns before any collective work, so one rank of a 2-rank world calls alone."""
    comms = H.loopback_world(2)
    try:
        c0, c1 = comms[0].handle, comms[1].handle
        # HcclScatter: sendBuf on the root only, then root, count, data type
        assert L.HcclScatter(None, P2, SYS_MAX_COUNT + 1, U8, 0, c0, P) == E.HCCL_E_PTR   # the root: before the count
        assert L.HcclScatter(None, P2, 8, U8, 7, c1, P) == E.HCCL_E_PARA    # off the root a null sendBuf passes: root >= n
        assert L.HcclScatter(P, P2, 8, INT128, 2, c0, P) == E.HCCL_E_PARA   # root before the data type
        assert L.HcclScatter(P, P2, SYS_MAX_COUNT + 1, INT128, 0, c0, P) == E.HCCL_E_PARA   # count before the data type
        assert L.HcclScatter(None, P2, SYS_MAX_COUNT + 1, U8, 0, c1, P) == E.HCCL_E_PARA    # off the root: the count
        assert L.HcclScatter(P, P2, 8, INT128, 0, c0, P) == E.HCCL_E_NOT_SUPPORT
        assert L.HcclScatter(P, P2, 8, 99, 0, c0, P) == E.HCCL_E_NOT_SUPPORT
        assert L.HcclScatter(None, P2, 8, INT128, 0, c1, P) == E.HCCL_E_NOT_SUPPORT
        # HcclAllGatherV
        u64 = ctypes.c_uint64 * 2
        zeros, displs = u64(0, 0), u64(0, 8)
        assert L.HcclAllGatherV(None, 0, None, zeros, displs, INT128, c0, P) == E.HCCL_SUCCESS  # all counts 0 first
        assert L.HcclAllGatherV(P, 8, None, u64(8, 8), displs, U8, c0, P) == E.HCCL_E_PTR      # then recvBuf
        assert L.HcclAllGatherV(None, 0, None, u64(0, 8), displs, U8, c0, P) == E.HCCL_E_PTR
        big = SYS_MAX_COUNT + 1
        assert L.HcclAllGatherV(P, big, P2, u64(big, 8), displs, INT128, c0, P) == E.HCCL_E_PARA  # count before type
        assert L.HcclAllGatherV(P, 8, P2, u64(9, 8), displs, INT128, c0, P) == E.HCCL_E_NOT_SUPPORT  # type before the
        assert L.HcclAllGatherV(P, 8, P2, u64(8, 8), displs, 99, c0, P) == E.HCCL_E_NOT_SUPPORT      # additions
        # the two additions
        assert L.HcclAllGatherV(P, 8, P2, u64(9, 8), displs, U8, c0, P) == E.HCCL_E_PARA    # sendCount != recvCounts[rank]
        assert L.HcclAllGatherV(P, 8, P2, u64(8, 9), displs, U8, c1, P) == E.HCCL_E_PARA
        assert L.HcclAllGatherV(P, 8, P2, u64(8, big), displs, U8, c0, P) == E.HCCL_E_PARA  # a peer's block too long
        assert L.HcclAllGatherV(P, 8, P2, u64(8, 8), u64(0, (1 << 64) - 4), U8, c0, P) == E.HCCL_E_PARA  # end overflows
        assert L.HcclAllGatherV(None, 0, P2, u64(0, 8), u64(0, (1 << 64) - 4), U8, c0, P) == E.HCCL_E_PARA
    finally:
        for c in comms:
            c.destroy()
