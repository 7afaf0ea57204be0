// ipc_k_a2a.hip — the one-sided all-to-all (IpcKind kIpcAllToAll: HcclAlltoAll, HcclAlltoAllV, HcclAlltoAllVC) over
// peer-mapped staging.
//
// A kernel of its own, like the Broadcast's: k_ipc_collective keeps its code and occupancy. It moves data only, so it
// is instantiated per element size, and it shares the barrier, the epoch counter, the sticky-bit check, the block
// windows and the copy loop with the other kinds (ipc_kernel_body.h). Every access to a peer is a store (PUSH only).
//
// A single-barrier kind: slot q of a rank's alternate area (by the parity of the round's barrier epoch, as the other
// single-barrier kinds do) receives pair (q, rank). Per round k, with `piece` elements of slot capacity:
//   push      for every peer q, in an order rotated by the block: elements [k piece, min((k + 1) piece, send[q])) of
//             sendBuf + sdispls[q] into slot `me` of q's area; the own block goes straight from sendBuf to recvBuf
//   barrier
//   copy out  for every peer q: the matching part of slot q of my own area to recvBuf + rdispls[q] + k piece, its
//             length from recv[q]
// User displacements are arbitrary, so the 16-byte vector path is chosen per (source, destination) pair; slots are
// always aligned.
//
// Rounds. AlltoAll and AlltoAllVC: every rank knows the count matrix and the host passes the round count. AlltoAllV
// (IpcA2aArgs::agreed): a rank knows its own row and column only, while block b's barrier waits for block b of every
// peer, so every rank must run the same number of barriers. Each block stores its rank's own need, ceil(max over its
// send counts / piece) (the row maximum suffices: every pair's count is in its sender's row), into word b of the header
// of the slot it pushes to each peer in round 0, and after that round's barrier takes the maximum over the n headers
// of its own area. The header is per block because block b's barrier orders only block b of each peer. A rank that has
// finished its own data runs the remaining barriers and pushes nothing; at least one round always runs, so a rank
// with nothing to move still meets its peers. The launch's end advances the device epoch counter by the agreed count
// (EndLaunchSpan). Model-checked by tests/test_ipc_protocol_alltoall.py.
#include "ipc_kernel_body.h"

namespace hccl_amd {

namespace {

template <typename S>
__global__ __launch_bounds__(kIpcMaxThreads) void k_ipc_a2a(IpcArgs a, IpcA2aArgs x)
{
    const uint32_t n = a.n;
    const uint32_t me = a.me >= 0 ? static_cast<uint32_t>(a.me) : blockIdx.y;
    const S* in = static_cast<const S*>(a.in[me]);
    S* out = static_cast<S*>(a.out[me]);
    const bool nt = a.nt != 0;
    const uint32_t bt = a.threads;
    // the sticky bit and the epoch counter as in k_ipc_collective
    const uint32_t sticky = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint32_t epoch = __hip_atomic_load(a.status + kIpcEpochWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((sticky & 1u) != 0) return;
    // this rank's tables, from the arguments (rank mode) or the world's table array, into LDS once
    __shared__ uint64_t tab[kA2aRows][kIpcMaxRanks];
    if (threadIdx.x < kA2aRows * kIpcMaxRanks) {
        const uint32_t row = threadIdx.x / kIpcMaxRanks, q = threadIdx.x % kIpcMaxRanks;
        tab[row][q] = a.me >= 0 ? x.mine.v[row][q] : x.world[me].v[row][q];
    }
    __syncthreads();
    Stamp(a, me, kTrEntry);
    const uint32_t arrivedBefore = Arrive(a, epoch);
    uint32_t waitMax = 0;
    // my own need; the agreed form learns the peers' after the first barrier
    uint64_t widest = 0;
    for (uint32_t q = 0; q < n; ++q) widest = max(widest, tab[kA2aSend][q]);
    const uint64_t needed = (widest + a.piece - 1) / a.piece;
    const uint32_t need = static_cast<uint32_t>(min(uint64_t(0xFFFFFFFFu), max(uint64_t(1), needed)));
    uint32_t rounds = x.agreed != 0 ? need : a.rounds;
    const uint64_t slotBytes = x.slotElems * sizeof(S);
    constexpr uintptr_t kVecMask = 15;
    auto aligned = [](const void* p, const void* q) {
        return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & kVecMask) == 0;
    };
    // elements of a pair of `count` elements that round k (offset kP) moves
    auto part = [&](uint64_t count, uint64_t kP) { return kP >= count ? uint64_t(0) : min(a.piece, count - kP); };
    for (uint32_t k = 0; k < rounds; ++k) {
        const uint64_t kP = uint64_t(k) * a.piece;
        const uint32_t par = (epoch + 1) & 1u;
        Stamp(a, me, kTrRound);
        if (x.agreed != 0 && k == 0 && threadIdx.x < n && threadIdx.x != me) {
            // lane t: my need into word `block` of the header of slot `me` on peer t
            char* slot = static_cast<char*>(a.stgAlt[par][threadIdx.x]) + uint64_t(me) * slotBytes;
            __hip_atomic_store(reinterpret_cast<uint32_t*>(slot) + blockIdx.x, need, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
        {
            // the own block never touches staging
            const S* src = in + tab[kA2aSdispl][me];
            S* dst = out + tab[kA2aRdispl][me];
            const bool vec = aligned(src, dst);
            ForBlockShare(a, part(tab[kA2aSend][me], kP), [&](Range r) { CopyRange<S>(dst + kP, src + kP, r, vec, nt, bt); });
        }
        // the peers in an order rotated by the block, so the blocks spread their stores over the links
        for (uint32_t i = 0; i + 1 < n; ++i) {
            const uint32_t q = (me + 1 + (i + blockIdx.x) % (n - 1)) % n;
            const S* src = in + tab[kA2aSdispl][q];
            S* slot = reinterpret_cast<S*>(static_cast<char*>(a.stgAlt[par][q]) + uint64_t(me) * slotBytes) + x.hdrElems;
            const bool vec = aligned(src, slot);
            ForBlockShare(a, part(tab[kA2aSend][q], kP), [&](Range r) { CopyRange<S>(slot, src + kP, r, vec, nt, bt); });
        }
        Stamp(a, me, kTrPhase0);
        const FlagLane fl = LaneFlags(a, me);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier1);
        const char* area = static_cast<const char*>(a.stgAlt[epoch & 1u][me]);
        if (x.agreed != 0 && k == 0) {
            // every thread reads the same n - 1 words, written by block `block` of each peer before its barrier
            for (uint32_t q = 0; q < n; ++q) {
                if (q == me) continue;
                const uint32_t* h = reinterpret_cast<const uint32_t*>(area + uint64_t(q) * slotBytes) + blockIdx.x;
                rounds = max(rounds, __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
            }
        }
        for (uint32_t q = 0; q < n; ++q) {
            if (q == me) continue;
            const S* slot = reinterpret_cast<const S*>(area + uint64_t(q) * slotBytes) + x.hdrElems;
            S* dst = out + tab[kA2aRdispl][q];
            const bool vec = aligned(slot, dst);
            ForBlockShare(a, part(tab[kA2aRecv][q], kP), [&](Range r) { CopyRange<S>(dst + kP, slot, r, vec, nt, bt); });
        }
        Stamp(a, me, kTrPhase1);
    }
    if (a.trace != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        Stamp(a, me, kTrExit);
    }
    PublishWait(a, waitMax);
    EndLaunchSpan(a, arrivedBefore, x.agreed != 0 ? rounds : a.epochSpan);
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

hipError_t LaunchIpcA2a(uint32_t elemSize, const IpcArgs& a, const IpcA2aArgs& x, dim3 grid, hipStream_t s)
{
    if (elemSize != 1 && elemSize != 2 && elemSize != 4 && elemSize != 8) return hipErrorInvalidValue;
    return WithElemSize(elemSize, [&](auto e) {
        hipLaunchKernelGGL((k_ipc_a2a<decltype(e)>), grid, dim3(a.threads), 0, s, a, x);
        return hipGetLastError();
    });
}

const void* IpcA2aKernel(uint32_t elemSize)
{
    return WithElemSize(elemSize, [](auto e) { return reinterpret_cast<const void*>(&k_ipc_a2a<decltype(e)>); });
}

}  // namespace hccl_amd
