"""HcclSend, HcclRecv and HcclBatchSendRecv at the ABI: a plain C caller assigns the symbols to function pointers of the
reference's prototypes (include/hccl.h:154-169, 256-257 there) and links; HcclSendRecvItem has the public CANN
header's layout (32 bytes on LP64, the field order the reference's callers initialise) and HcclSendRecvType its
values; the checks that come before the communicator is looked at return the reference's codes (send_op.cc:33,
126-150; batch_send_recv_op.cc:39-56)."""
import ctypes
import os
import subprocess

import hccl_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, E = H.lib, H.HcclResult

C_CALLER = r"""
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "hccl.h"
typedef HcclResult (*SendFn)(void*, uint64_t, HcclDataType, uint32_t, HcclComm, aclrtStream);
typedef HcclResult (*BatchFn)(HcclSendRecvItem*, uint32_t, HcclComm, aclrtStream);
int main(void)
{
    SendFn send = HcclSend, recv = HcclRecv;
    BatchFn batch = HcclBatchSendRecv;
    char buf[8];
    /* the order the reference's callers initialise (batch_send_recv_testcase.cc:149-158) */
    HcclSendRecvItem item = {HCCL_SEND, buf, 8, HCCL_DATA_TYPE_INT8, 1};
    if (sizeof(HcclSendRecvItem) != 32) return 1;
    if (offsetof(HcclSendRecvItem, sendRecvType) != 0 || offsetof(HcclSendRecvItem, buf) != 8 ||
        offsetof(HcclSendRecvItem, count) != 16 || offsetof(HcclSendRecvItem, dataType) != 24 ||
        offsetof(HcclSendRecvItem, remoteRank) != 28) return 2;
    if (HCCL_SEND != 0 || HCCL_RECV != 1 || HCCL_SEND_RECV_RESERVED != 2) return 3;
    if (item.remoteRank != 1 || item.count != 8) return 4;
    if (send(NULL, 0, HCCL_DATA_TYPE_INT8, 0, NULL, NULL) != HCCL_SUCCESS) return 5;
    if (recv(buf, 8, HCCL_DATA_TYPE_INT8, 0, NULL, (aclrtStream)buf) != HCCL_E_PTR) return 6;
    if (batch(&item, 0, NULL, NULL) != HCCL_SUCCESS) return 7;
    if (batch(&item, 1, NULL, (aclrtStream)buf) != HCCL_E_PTR) return 8;
    puts("OK");
    return 0;
}
"""


def test_c_caller_links_and_sees_the_cann_layout(tmp_path):
    src, exe = tmp_path / "caller.c", tmp_path / "caller"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(H.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe), "-L", libdir, "-lhccl_amd", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "OK", (out.returncode, out.stdout, out.stderr)


def test_python_mirror_matches():
    assert ctypes.sizeof(H.HcclSendRecvItem) == 32
    assert [getattr(H.HcclSendRecvItem, f).offset for f in ("sendRecvType", "buf", "count", "dataType", "remoteRank")] \
        == [0, 8, 16, 24, 28]
    assert (int(H.SendRecvType.SEND), int(H.SendRecvType.RECV)) == (0, 1)
    assert len(H.SIGNATURES["HcclSend"][1]) == 6 and len(H.SIGNATURES["HcclRecv"][1]) == 6
    assert len(H.SIGNATURES["HcclBatchSendRecv"][1]) == 4


def test_checks_before_the_communicator():
    P, FP32 = 0x1000, int(H.HcclDataType.FP32)  # never dereferenced
    for fn in (L.HcclSend, L.HcclRecv):
        assert fn(None, 0, 99, 99, None, None) == E.HCCL_SUCCESS  # count 0 before any other check
        assert fn(P, 8, FP32, 1, None, P) == E.HCCL_E_PTR         # comm
        assert fn(None, 8, FP32, 1, P, P) == E.HCCL_E_PTR         # buffer
    items = H.send_recv_items([(H.SendRecvType.SEND, (P, 8, FP32), 1)])
    assert L.HcclBatchSendRecv(None, 0, None, None) == E.HCCL_SUCCESS  # itemNum 0
    assert L.HcclBatchSendRecv(items, 1, P, None) == E.HCCL_E_PTR      # stream
    assert L.HcclBatchSendRecv(items, 1, None, P) == E.HCCL_E_PTR      # comm
    assert L.HcclBatchSendRecv(None, 1, P, P) == E.HCCL_E_PTR          # the list
    assert L.HcclAmdCommEnableP2p(None) == E.HCCL_E_PTR
