// ipc_k_bcast.hip — the one-sided Broadcast (IpcKind kIpcBroadcast, kIpcBroadcastOneShot) over peer-mapped staging.
//
// A kernel of its own, like the RHD and LL forms: k_ipc_collective keeps its code and occupancy. It moves data only, so
// it is instantiated per element size, and it shares the barrier, the epoch counter, the sticky-bit check, the block
// windows and the copy loop with the other kinds (ipc_kernel_body.h). Every access to a peer is a store (PUSH only).
//
// kIpcBroadcast, per round (chunk c = ceil(count / n) rounded up to 128 B, owned by rank c; piece = the round's part):
//   phase 0  the root stores chunk c into slot 0 and its own chunk into slot 1 of rank c's slot area, c != root
//   barrier
//   phase 1  rank r != root copies both slots into its buffer and pushes chunk r (from slot 0) into the result area of
//            every peer other than the root, at chunk r's place
//   barrier
//   phase 2  rank r != root copies the chunks of the other non-root ranks from its own result area
// The root takes part in both barriers and never writes its own buffer.
// The slot and result areas are the ones the other two-barrier kinds use, with no barrier between calls, so the kind
// keeps their invariant: the slot area is read, and the result area written, only between a call's two barriers. That
// is why the root's chunk travels through the slot area and is copied out in phase 1 (the root's next call may store
// there right after barrier 2), and why the root pushes nothing into a result area in phase 0 (a peer may still read
// it in phase 2 of its previous call). Model-checked by tests/test_ipc_protocol_broadcast.py.
//
// kIpcBroadcastOneShot, per round: the root pushes the whole piece into slot 0 of every peer's alternate area (by the
// parity of the round's barrier epoch, as the other single-barrier kinds do); barrier; every peer copies it out.
#include "ipc_kernel_body.h"

namespace hccl_amd {

namespace {

// The j-th rank (ascending) that is neither x nor y.
__device__ __forceinline__ uint32_t SkipTwo(uint32_t j, uint32_t x, uint32_t y)
{
    const uint32_t lo = min(x, y), hi = max(x, y);
    if (j >= lo) ++j;
    if (j >= hi && hi != lo) ++j;
    return j;
}

template <typename S>
__global__ __launch_bounds__(kIpcMaxThreads) void k_ipc_bcast(IpcArgs a)
{
    const uint32_t n = a.n, root = a.root;
    const uint32_t me = a.me >= 0 ? static_cast<uint32_t>(a.me) : blockIdx.y;
    S* buf = static_cast<S*>(a.out[me]);
    const bool oneShot = a.kind == kIpcBroadcastOneShot;
    const bool nt = a.nt != 0;
    const uint32_t bt = a.threads;
    // the sticky bit and the epoch counter as in k_ipc_collective
    const uint32_t sticky = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint32_t epoch = __hip_atomic_load(a.status + kIpcEpochWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((sticky & 1u) != 0) return;
    Stamp(a, me, kTrEntry);
    const uint32_t arrivedBefore = Arrive(a, epoch);
    uint32_t waitMax = 0;
    for (uint32_t k = 0; k < a.rounds; ++k) {
        const uint64_t kP = uint64_t(k) * a.piece;
        Stamp(a, me, kTrRound);
        if (oneShot) {
            // every "chunk" is the whole range (kIpcGeomWhole): the round's piece is elements [kP, kP + len)
            const uint64_t len = PieceLen(a, me, kP);
            if (me == root) {
                // the peers in an order rotated by the block, so the blocks spread their stores over the links
                auto dst = [&](uint32_t d) {
                    const uint32_t c = (me + 1 + (d + blockIdx.x) % (n - 1)) % n;
                    return static_cast<S*>(a.stgAlt[(epoch + 1) & 1u][c]);
                };
                ForBlockShare(a, len, [&](Range r) { CopyRangeTo<S>(dst, n - 1, buf + kP, r, a.aligned, nt, bt); });
            }
            Stamp(a, me, kTrPhase0);
            const FlagLane fl = LaneFlags(a, me);
            if (!Barrier(a, fl, ++epoch, waitMax)) break;
            Stamp(a, me, kTrBarrier1);
            if (me != root) {
                const S* slot = static_cast<const S*>(a.stgAlt[epoch & 1u][me]);
                ForBlockShare(a, len, [&](Range r) { CopyRange<S>(buf + kP, slot, r, a.aligned, nt, bt); });
            }
            Stamp(a, me, kTrPhase1);
            continue;
        }
        const uint64_t rootLen = PieceLen(a, root, kP);
        S* rootChunk = buf + ChunkStart(a, root) + kP;
        const bool rootVec = ChunkVec<S>(a, root);
        if (me == root) {
            // phase 0: chunk c into slot 0 of rank c, my own chunk into slot 1 of every peer
            for (uint32_t i = 0; i + 1 < n; ++i) {
                const uint32_t c = (me + 1 + (i + blockIdx.x) % (n - 1)) % n;
                ForBlockShare(a, PieceLen(a, c, kP), [&](Range r) {
                    CopyRange<S>(static_cast<S*>(a.stgIn[c]), buf + ChunkStart(a, c) + kP, r, ChunkVec<S>(a, c), nt, bt);
                });
            }
            auto dst = [&](uint32_t d) {
                const uint32_t c = (me + 1 + (d + blockIdx.x) % (n - 1)) % n;
                return static_cast<S*>(a.stgIn[c]) + a.piece;
            };
            ForBlockShare(a, rootLen, [&](Range r) { CopyRangeTo<S>(dst, n - 1, rootChunk, r, rootVec, nt, bt); });
        }
        Stamp(a, me, kTrPhase0);
        const FlagLane fl = LaneFlags(a, me);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier1);
        if (me != root) {
            // phase 1: both slots into my buffer; my chunk on to the result area of every other non-root rank
            const S* slots = static_cast<const S*>(a.stgIn[me]);
            S* mine = buf + ChunkStart(a, me) + kP;
            const bool vec = ChunkVec<S>(a, me);
            // destination 0 is my buffer when it takes the vector path with the staging; an unaligned buffer is
            // copied element-wise on its own, and the staging keeps its vectors
            const uint32_t first = vec ? 0u : 1u;
            auto dst = [&](uint32_t d) {
                if (d + first == 0) return mine;
                const uint32_t p = SkipTwo((d + first - 1 + blockIdx.x) % (n - 2), me, root);
                return static_cast<S*>(a.stgRes[p]) + uint64_t(me) * a.piece;
            };
            ForBlockShare(a, PieceLen(a, me, kP), [&](Range r) {
                if (!vec) CopyRange<S>(mine, slots, r, false, nt, bt);
                if (n - 1 - first != 0) CopyRangeTo<S>(dst, n - 1 - first, slots, r, true, nt, bt);
            });
            ForBlockShare(a, rootLen, [&](Range r) { CopyRange<S>(rootChunk, slots + a.piece, r, rootVec, nt, bt); });
        }
        Stamp(a, me, kTrPhase1);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier2);
        if (me != root) {
            // phase 2: the other non-root ranks' chunks from my own result area
            for (uint32_t j = 0; j + 2 < n; ++j) {
                const uint32_t c = SkipTwo(j, me, root);
                ForBlockShare(a, PieceLen(a, c, kP), [&](Range r) {
                    CopyRange<S>(buf + ChunkStart(a, c) + kP,
                                 static_cast<const S*>(a.stgRes[me]) + uint64_t(c) * a.piece, r, ChunkVec<S>(a, c), nt,
                                 bt);
                });
            }
        }
        Stamp(a, me, kTrPhase2);
    }
    if (a.trace != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        Stamp(a, me, kTrExit);
    }
    PublishWait(a, waitMax);
    EndLaunch(a, arrivedBefore);
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

hipError_t LaunchIpcBcast(uint32_t elemSize, const IpcArgs& a, dim3 grid, hipStream_t s)
{
    if (elemSize != 1 && elemSize != 2 && elemSize != 4 && elemSize != 8) return hipErrorInvalidValue;
    return WithElemSize(elemSize, [&](auto e) {
        hipLaunchKernelGGL((k_ipc_bcast<decltype(e)>), grid, dim3(a.threads), 0, s, a);
        return hipGetLastError();
    });
}

const void* IpcBcastKernel(uint32_t elemSize)
{
    return WithElemSize(elemSize, [](auto e) { return reinterpret_cast<const void*>(&k_ipc_bcast<decltype(e)>); });
}

}  // namespace hccl_amd
