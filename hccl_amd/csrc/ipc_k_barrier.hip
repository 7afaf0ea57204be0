// ipc_k_barrier.hip — the one-sided barrier (IpcKind kIpcBarrier: HcclBarrier) over the peer-mapped flag words.
//
// A kernel of its own, typeless like the Scatter's: it moves no data, so it has one instantiation. It is the flag
// exchange of the collectives' own barrier and nothing else, built from the same device functions (ipc_kernel_body.h):
// the sticky-bit check, the epoch counter, Barrier() with its fences and bounded poll, the wait diagnostic and the
// launch's end count. It touches no staging tier and no user buffer.
//
// Launch shape: one workgroup of one wave per rank (blockIdx.y is the rank in a loopback world, as elsewhere). Lane
// t < n stores the flag word of workgroup 0 on peer t and polls the word peer t stores here; the other lanes only take
// part in the workgroup barriers inside Barrier().
//
// Protocol: read the epoch counter E, arrive, one Barrier() at E + 1 on workgroup 0's flag words, then the launch's
// end count advances the counter by epochSpan = 1. A rank's kernel therefore ends only after every rank's kernel has
// stored its flag, which a rank's stream reaches only after everything enqueued before its HcclBarrier has ended.
//
// Why this is sound next to launches with more workgroups. Every launch of a communicator takes its epochs from the
// one counter, whatever its workgroup count, and workgroup b only ever looks at flag words [b][.]. After this launch
// the counter stands at E + 1 while only workgroup 0's words hold E + 1: the words of workgroups b >= 1 still hold
// what their last launch left, some value <= E. The next launch's workgroup b stores and waits for E + 2 (or later
// epochs). PollFlag waits until the signed difference flag - want is no longer negative, so a word that skips E + 1
// and goes from <= E straight to E + 2 is waited for exactly as one that held E + 1 in between: a skipped epoch is
// harmless, as it already is between a launch of many workgroups and a later one of few. Nor can a stale word pass
// for a fresh one: a peer's workgroup b stores E + 2 only from the launch that follows its own barrier launch.
// The single-barrier kinds pick their alternate area by the epoch's parity, and this launch flips it. That only makes
// two launches around a barrier use the same area, which is safe because of the barrier itself: a peer's stores of
// the later launch follow its barrier kernel, which ends only after this rank's barrier kernel has begun, that is
// after every workgroup of this rank's earlier launch has ended and read what it needed.
// The LL form keeps a sequence word of its own (kIpcLlSeqWord) and flags beside its data: it never sees an epoch.
// Model-checked among the other kinds by tests/test_ipc_protocol_barrier.py.
//
// Memory ordering: the data of earlier and later kernels is released and acquired by the kernel boundaries on either
// side of this launch (ipc.cc, IpcLightFence). The kernel adds nothing beyond what Barrier() does for the
// communicator's fence mode; its flag stores are Barrier()'s system-scope vector stores behind the explicit wait.
#include "ipc_kernel_body.h"

namespace hccl_amd {

namespace {

constexpr uint32_t kBarrierThreads = 64;  // one wave: kIpcMaxRanks lanes hold a flag pair each
static_assert(kIpcMaxRanks <= int(kBarrierThreads), "one lane per peer");

__global__ __launch_bounds__(kBarrierThreads) void k_ipc_barrier(IpcArgs a)
{
    const uint32_t me = a.me >= 0 ? static_cast<uint32_t>(a.me) : blockIdx.y;
    // the sticky bit and the epoch counter as in k_ipc_collective
    const uint32_t sticky = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t epoch = __hip_atomic_load(a.status + kIpcEpochWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((sticky & 1u) != 0) return;
    Stamp(a, me, kTrEntry);
    const uint32_t arrivedBefore = Arrive(a, epoch);
    uint32_t waitMax = 0;
    Stamp(a, me, kTrRound);
    const FlagLane fl = LaneFlags(a, me);  // blockIdx.x == 0: workgroup 0's words
    if (Barrier(a, fl, epoch + 1, waitMax)) Stamp(a, me, kTrBarrier1);
    if (a.trace != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        Stamp(a, me, kTrExit);
    }
    PublishWait(a, waitMax);
    EndLaunch(a, arrivedBefore);
}

}  // namespace

hipError_t LaunchIpcBarrier(const IpcArgs& a, uint32_t worldRanks, hipStream_t s)
{
    hipLaunchKernelGGL(k_ipc_barrier, dim3(1, worldRanks == 0 ? 1 : worldRanks), dim3(kBarrierThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace hccl_amd
