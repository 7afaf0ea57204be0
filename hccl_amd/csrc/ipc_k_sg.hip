// ipc_k_sg.hip — the one-sided Scatter and AllGatherV (IpcKind kIpcScatter, kIpcAllGatherV: HcclScatter,
// HcclAllGatherV) over peer-mapped staging.
//
// A kernel of its own, like the Broadcast's and the all-to-all's: k_ipc_collective keeps its code and occupancy. It moves
// data only, so it is instantiated per element size, and it shares the barrier, the epoch counter, the sticky-bit
// check, the block windows and the copy loops with the other kinds (ipc_kernel_body.h). Every access to a peer is a
// store (PUSH only). Both are single-barrier kinds: their slots lie in the alternate area chosen by the parity of the
// round's barrier epoch, as the other single-barrier kinds' do, and every rank runs every barrier of the launch
// whatever it has to move. The host sets the round count: every rank knows every count. Model-checked among the other
// kinds by tests/test_ipc_protocol_scatter_gatherv.py.
//
// kIpcScatter (kIpcGeomBlock: block c of the root's input is chunk c), per round k with `piece` elements of capacity:
//   push      the root stores piece k of block c into the one slot of rank c's area (a receiver has one sender, so the
//             slot is the whole area: the one-shot Broadcast's layout), the peers in an order rotated by the block
//   barrier
//   copy out  rank c != root copies its slot to recvBuf + k piece; the root copies its own block's piece straight from
//             sendBuf to recvBuf. That copy comes after the barrier so that, in place (recvBuf == sendBuf) on a root
//             other than 0, it never overtakes the push of block 0's piece k, which this same workgroup has read from
//             the same window before its barrier.
//
// kIpcAllGatherV (kIpcGeomV: rank q's block is vLen[q] elements at vStart[q] of every output), per round k:
//   push      piece k of the input into slot `me` of every peer's area, each element loaded once and stored n - 1
//             times; the own block goes straight to recvBuf + vStart[me] unless the input is that very place
//   barrier
//   copy out  the n - 1 slots of my own area to recvBuf + vStart[q] + k piece, lengths from vLen[q]
// User displacements are arbitrary, so the 16-byte vector path is chosen per destination; slots are always aligned.
#include "ipc_kernel_body.h"

namespace hccl_amd {

namespace {

template <typename S>
__global__ __launch_bounds__(kIpcMaxThreads) void k_ipc_sg(IpcArgs a)
{
    const uint32_t n = a.n, root = a.root;  // n >= 2: the operators copy a one-rank call on the host (ops.cc)
    const uint32_t me = a.me >= 0 ? static_cast<uint32_t>(a.me) : blockIdx.y;
    const S* in = static_cast<const S*>(a.in[me]);
    S* out = static_cast<S*>(a.out[me]);
    const bool scatter = a.kind == kIpcScatter;
    const bool nt = a.nt != 0;
    const uint32_t bt = a.threads;
    // the sticky bit and the epoch counter as in k_ipc_collective
    const uint32_t sticky = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint32_t epoch = __hip_atomic_load(a.status + kIpcEpochWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((sticky & 1u) != 0) return;
    Stamp(a, me, kTrEntry);
    const uint32_t arrivedBefore = Arrive(a, epoch);
    uint32_t waitMax = 0;
    constexpr uintptr_t kVecMask = 15;
    auto aligned = [](const void* p, const void* q) {
        return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & kVecMask) == 0;
    };
    for (uint32_t k = 0; k < a.rounds; ++k) {
        const uint64_t kP = uint64_t(k) * a.piece;
        const uint32_t par = (epoch + 1) & 1u;
        Stamp(a, me, kTrRound);
        if (scatter) {
            const uint64_t len = PieceLen(a, me, kP);  // every block holds the same count
            if (me == root) {
                for (uint32_t i = 0; i + 1 < n; ++i) {
                    const uint32_t c = (me + 1 + (i + blockIdx.x) % (n - 1)) % n;
                    const S* src = in + ChunkStart(a, c);
                    S* slot = static_cast<S*>(a.stgAlt[par][c]);
                    const bool vec = aligned(src, slot);
                    ForBlockShare(a, len, [&](Range r) { CopyRange<S>(slot, src + kP, r, vec, nt, bt); });
                }
            }
            Stamp(a, me, kTrPhase0);
            const FlagLane fl = LaneFlags(a, me);
            if (!Barrier(a, fl, ++epoch, waitMax)) break;
            Stamp(a, me, kTrBarrier1);
            // the root's own block from its input (nothing to do in place on root 0), a peer's from its slot
            const S* src = me == root ? in + ChunkStart(a, me) : static_cast<const S*>(a.stgAlt[epoch & 1u][me]);
            if (src != out) {
                const bool vec = aligned(src, out);
                const uint64_t srcOff = me == root ? kP : 0;
                ForBlockShare(a, len, [&](Range r) { CopyRange<S>(out + kP, src + srcOff, r, vec, nt, bt); });
            }
            Stamp(a, me, kTrPhase1);
            continue;
        }
        // elements of a block of `count` elements that round k moves
        auto part = [&](uint64_t count) { return kP >= count ? uint64_t(0) : min(a.piece, count - kP); };
        {
            const uint64_t len = part(a.vLen[me]);
            // the peers in an order rotated by the block, so the blocks spread their stores over the links
            auto dst = [&](uint32_t d) {
                const uint32_t q = (me + 1 + (d + blockIdx.x) % (n - 1)) % n;
                return static_cast<S*>(a.stgAlt[par][q]) + uint64_t(me) * a.piece;
            };
            const bool vec = aligned(in, nullptr);
            ForBlockShare(a, len, [&](Range r) { CopyRangeTo<S>(dst, n - 1, in + kP, r, vec, nt, bt); });
            S* own = out + a.vStart[me];
            if (own != in) {
                const bool ownVec = aligned(in, own);
                ForBlockShare(a, len, [&](Range r) { CopyRange<S>(own + kP, in + kP, r, ownVec, nt, bt); });
            }
        }
        Stamp(a, me, kTrPhase0);
        const FlagLane fl = LaneFlags(a, me);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier1);
        const S* area = static_cast<const S*>(a.stgAlt[epoch & 1u][me]);
        for (uint32_t q = 0; q < n; ++q) {
            if (q == me) continue;
            const S* slot = area + uint64_t(q) * a.piece;
            S* dst = out + a.vStart[q];
            const bool vec = aligned(slot, dst);
            ForBlockShare(a, part(a.vLen[q]), [&](Range r) { CopyRange<S>(dst + kP, slot, r, vec, nt, bt); });
        }
        Stamp(a, me, kTrPhase1);
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

hipError_t LaunchIpcSg(uint32_t elemSize, const IpcArgs& a, dim3 grid, hipStream_t s)
{
    if (elemSize != 1 && elemSize != 2 && elemSize != 4 && elemSize != 8) return hipErrorInvalidValue;
    return WithElemSize(elemSize, [&](auto e) {
        hipLaunchKernelGGL((k_ipc_sg<decltype(e)>), grid, dim3(a.threads), 0, s, a);
        return hipGetLastError();
    });
}

const void* IpcSgKernel(uint32_t elemSize)
{
    return WithElemSize(elemSize, [](auto e) { return reinterpret_cast<const void*>(&k_ipc_sg<decltype(e)>); });
}

}  // namespace hccl_amd
