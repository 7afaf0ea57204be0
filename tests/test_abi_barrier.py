"""HcclBarrier at the ABI: a plain C caller assigns the symbol to a function pointer of the reference's prototype
(src/ops/barrier/barrier_op.h there: HcclResult HcclBarrier(HcclComm comm, aclrtStream stream)) and links; the checks
that come before the communicator is looked at return the reference's codes in its order (barrier_op.cc:91-102: the
stream, then the communicator)."""
import os
import subprocess

import hccl_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, E = H.lib, H.HcclResult

C_CALLER = r"""
#include <stddef.h>
#include <stdio.h>
#include "hccl.h"
typedef HcclResult (*BarrierFn)(HcclComm, aclrtStream);
int main(void)
{
    BarrierFn barrier = HcclBarrier;
    char word[8];
    if (barrier((HcclComm)word, NULL) != HCCL_E_PTR) return 1;    /* a null stream */
    if (barrier(NULL, (aclrtStream)word) != HCCL_E_PTR) return 2; /* a null communicator */
    if (barrier(NULL, NULL) != HCCL_E_PTR) return 3;
    puts("OK");
    return 0;
}
"""


def test_c_caller_links_with_the_reference_signature(tmp_path):
    src, exe = tmp_path / "caller.c", tmp_path / "caller"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(H.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe), "-L", libdir, "-lhccl_amd", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "OK", (out.returncode, out.stdout, out.stderr)


def test_python_mirror_matches():
    res, args = H.SIGNATURES["HcclBarrier"]
    assert len(args) == 2
    assert int(H.OpType.BARRIER) == 9
    assert callable(H.Comm.barrier)


def test_checks_before_the_communicator():
    P = 0x1000  # never dereferenced
    assert L.HcclBarrier(P, None) == E.HCCL_E_PTR     # the stream comes first: the communicator is not looked at
    assert L.HcclBarrier(None, P) == E.HCCL_E_PTR
    assert L.HcclBarrier(None, None) == E.HCCL_E_PTR
