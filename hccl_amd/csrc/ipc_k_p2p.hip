// ipc_k_p2p.hip — the one-sided HcclSend / HcclRecv / HcclBatchSendRecv over a peer-mapped area of their own.
//
// A kernel of its own and typeless, like k_ipc_sg: it moves data only, so it is instantiated per element size. It
// shares the copy loop, the fences, the phase stamps, the sticky-bit check and the bounded poll with the other kinds
// (ipc_kernel_body.h), and nothing else: only two ranks run a message, so it reads and writes none of the collectives'
// state: not the barrier epochs (kIpcEpochWord, kIpcDoneWord), not the flag table, not the staging tiers, not callSeq.
// Of IpcArgs::status it touches word 0 alone (the sticky bit). Every access to a peer is a store (PUSH only); every
// load reads this rank's own memory.
//
// Layout (ipc_plan.h): a rank's area holds kP2pSlots data slots per source rank, then filled[p][b] (stored by sender
// p) and drained[q][b] (stored by receiver q: the credit for this rank's sends to q), one word per workgroup b. The
// piece numbers s of an ordered pair and workgroup run on across calls; they live on the device, in the private
// counters sent[q][b] and rcvd[p][b], so a captured launch replays correctly, as the epoch word lets the collectives.
//
// blockIdx.y is a lane: one (direction, peer) pair of the launch, which no other lane shares, so workgroup (b, lane)
// alone reads its counter at entry and writes it at exit, and no atomic is needed. The lane's items run in order. Per
// piece s of `slotElems` elements, workgroup b moves its window of the piece (both ends derive the windows from the
// count, the element size and the slot size alone; an empty window still takes every step, so the counters and the
// flags advance alike on both sides):
//   sender    wait  drained[q][b] >= s - kP2pSlots       (own area; no acquire: nothing is read behind it)
//             push  the window into slot s % kP2pSlots of row `me` in the receiver's area
//             drain, release, store filled[me][b] = s     into the receiver
//   receiver  wait  filled[p][b] >= s, acquire            (own area)
//             copy  the window from its own slot s % kP2pSlots to the user buffer
//             drain, store drained[me][b] = s              into the sender
// The comparisons are serial-number compares (PollFlag), so the 32-bit counters may wrap. A message of at most
// kP2pSlots pieces completes on the sender without the receiver having started. A wait that is cut short (its bound, or
// the sticky bit) ends the workgroup at once: it stores nothing more to the peer. Model-checked by
// tests/test_ipc_protocol_p2p.py.
#include "ipc_kernel_body.h"

namespace hccl_amd {

namespace {

// Thread 0 polls; the workgroup learns the outcome. Every P2pWait is followed by a P2pSignal, whose workgroup barrier
// lets every thread read `cut` before thread 0 writes it again.
__device__ __forceinline__ bool P2pWait(const IpcArgs& a, const uint32_t* word, uint32_t want, bool acquire)
{
    __shared__ uint32_t cut;
    if (threadIdx.x == 0) {
        uint32_t polls = 0;
        cut = PollFlag(a, word, want, polls) ? 1u : 0u;
        if (acquire) {
            // as Barrier: the CU's L1 (light), or the system-scope acquire that also invalidates the XCD's L2
            if (a.fence == 0) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            } else {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed before the copy starts
        }
    }
    __syncthreads();
    return cut == 0;
}

// Every wave's loads and stores of the piece have completed (vmcnt(0)); then one thread publishes the piece number, as
// Barrier publishes its epoch: behind the system-scope write-back when IpcArgs::fence asks for it.
__device__ __forceinline__ void P2pSignal(const IpcArgs& a, uint32_t* word, uint32_t s)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if (a.fence == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(word, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <typename S>
__global__ __launch_bounds__(kIpcMaxThreads) void k_ipc_p2p(IpcArgs a, IpcP2pArgs x)
{
    const IpcP2pLane& L = x.lane[blockIdx.y];
    const uint32_t n = a.n, b = blockIdx.x, me = L.me, peer = L.peerRank;
    const bool send = L.isSend != 0;
    const bool nt = a.nt != 0;
    const uint32_t bt = a.threads;
    if ((__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) & 1u) != 0) return;
    Stamp(a, me, kTrEntry);
    // sent[peer][b] or rcvd[peer][b]: pieces of this ordered pair and workgroup since the set-up
    uint32_t* ctr = L.ctr + (send ? 0u : n * kP2pBlocks) + peer * kP2pBlocks + b;
    uint32_t s = *ctr;
    // the word polled here and the word stored into the peer; the slots' row is the sender's rank on both sides
    const uint64_t sb = x.slotBytes;
    const uint32_t* waitWord = reinterpret_cast<const uint32_t*>(
        L.mine + (send ? P2pDrainedOffset(sb, n, peer, b) : P2pFilledOffset(sb, n, peer, b)));
    uint32_t* signalWord =
        reinterpret_cast<uint32_t*>(L.peer + (send ? P2pFilledOffset(sb, n, me, b) : P2pDrainedOffset(sb, n, me, b)));
    char* row = send ? L.peer + P2pSlotOffset(sb, me, 0) : L.mine + P2pSlotOffset(sb, peer, 0);
    bool live = true;
    for (uint32_t i = 0; i < L.num && live; ++i) {
        const IpcP2pItem& it = x.item[L.first + i];
        S* buf = static_cast<S*>(it.buf);
        for (uint64_t off = 0; off < it.count; off += x.slotElems) {
            ++s;
            const uint64_t len = min(x.slotElems, it.count - off);
            const uint64_t lo = min(len, uint64_t(b) * x.blockElems);
            const Range r{lo, min(len, lo + x.blockElems)};
            S* slot = reinterpret_cast<S*>(row + uint64_t(s % kP2pSlots) * sb);
            S* user = buf + off;  // off is a whole number of slots, so `user` is aligned as `buf` is
            const bool vec = (reinterpret_cast<uintptr_t>(user) & 15u) == 0;
            Stamp(a, me, kTrRound);
            live = P2pWait(a, waitWord, send ? s - kP2pSlots : s, !send);
            if (!live) break;
            Stamp(a, me, kTrBarrier1);
            if (send) {
                CopyRange<S>(slot, user, r, vec, nt, bt);
            } else {
                CopyRange<S>(user, slot, r, vec, nt, bt);
            }
            Stamp(a, me, kTrPhase1);
            P2pSignal(a, signalWord, s);
        }
    }
    if (live && threadIdx.x == 0) *ctr = s;
    if (a.trace != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        Stamp(a, me, kTrExit);
    }
}

template <class F>
auto WithElemSize(uint32_t es, F&& f) -> decltype(f(uint8_t{}))
{
    switch (es) {
        case 1: return f(uint8_t{});
        case 2: return f(uint16_t{});
        case 4: return f(uint32_t{});
        default: return f(uint64_t{});
    }
}

}  // namespace

hipError_t LaunchIpcP2p(uint32_t elemSize, const IpcArgs& a, const IpcP2pArgs& x, dim3 grid, hipStream_t s)
{
    if (elemSize != 1 && elemSize != 2 && elemSize != 4 && elemSize != 8) return hipErrorInvalidValue;
    return WithElemSize(elemSize, [&](auto e) {
        hipLaunchKernelGGL((k_ipc_p2p<decltype(e)>), grid, dim3(a.threads), 0, s, a, x);
        return hipGetLastError();
    });
}

const void* IpcP2pKernel(uint32_t elemSize)
{
    return WithElemSize(elemSize, [](auto e) { return reinterpret_cast<const void*>(&k_ipc_p2p<decltype(e)>); });
}

}  // namespace hccl_amd
