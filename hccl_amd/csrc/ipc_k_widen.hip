// ipc_k_widen.hip — the one-sided widening FP8 sum (HcclAmdAllReduceWiden, HcclAmdReduceScatterWiden,
// HcclAmdReduceWiden) over peer-mapped staging: the three single-barrier one-shot kinds kIpcAllReduceOneShot,
// kIpcReduceScatter and kIpcReduceOneShot with FP8 operands (E4M3 / E5M2) and an FP32 / BF16 / FP16 result.
//
// A kernel of its own, like the Broadcast's, the all-to-all's and the Scatter's: k_ipc_collective keeps its code and
// occupancy. It shares the barrier, the epoch counter, the sticky-bit check, the block windows, Stamp / PublishWait /
// EndLaunch and the typeless copy loops with the other kinds (ipc_kernel_body.h), and the decode and narrowing with the
// local kernel (widen_elem.h). It adds no protocol: per round of `piece` elements, in FP8 elements throughout (the
// host plans with element size 1; only the output pointer counts in the output type),
//   push      this rank's FP8 bytes of the round into slot `me` of the alternate area (parity of the round's barrier
//             epoch) of every peer (one-shot AllReduce: each element loaded once and stored n - 1 times), of rank c
//             for block c (ReduceScatter), of the root only (one-shot Reduce). The data travels as FP8: a byte copy
//             (CopyRange / CopyRangeTo at element size 1). Every access to a peer is a store. The own operand is
//             not staged.
//   barrier
//   fold      order O1, acc = f32(own input); acc = f32(slot q) + acc for q != me ascending; recvBuf = narrow(acc):
//             every rank the whole piece (AllReduce), rank c block c (ReduceScatter), the root alone (Reduce; the
//             other ranks never write recvBuf). The same arithmetic as the schedule path's fold (k_reduce_widen over
//             the O1 operand list), so the same bits.
//
// The fold. k_reduce_widen sweeps cached HBM streams with a persistent grid. Here n - 1 of the n operands lie in
// uncached, peer-written staging, where every load instruction is a trip to memory, and a workgroup's window is small
// and fixed by the barrier protocol. A lane's unit is one load of W bytes per operand = W elements, a tile is
// 32 elements per lane (32 / W units, `threads` units apart), and:
//   * consecutive lanes own consecutive units, so a load instruction of a wave reads 64 W contiguous bytes of one
//     operand;
//   * all of an operand's loads of the tile are issued before any is decoded, and operand q + 1 is loaded before
//     operand q is folded, so two operands' loads are in flight while one is decoded and added;
//   * 32 FP32 accumulators per lane; loads and stores are non-temporal when IpcArgs::nt says so; no LDS (nothing is
//     reused); plain FP32 adds in operand order (no fast-math, denormals kept, packed FP32 adds off for this file:
//     Makefile).
// The load width W is a template parameter, fixed when the library is built (HCCL_AMD_IPC_WIDEN_LOAD_BYTES). Two
// candidates were measured (tools/probes/ipc_widen_bench.py, profiles/ipc_widen_loopback.jsonl: AllReduce, E4M3, 8-rank
// loopback world on one MI355X, one library per candidate, the candidates alternated over two passes, medians of five
// rounds of ten calls; us per call, pass 1 / pass 2):
//   W = 16, one 16-B load per operand and unit, four 16-B stores (FP32) or two (16-bit) per unit: the design's
//     starting point, since it takes the fewest trips to the uncached staging; 79 VGPRs;
//   W = O::kPer (4 bytes for FP32 output, 8 for 16-bit), one whole 16-B output vector per unit as in the local kernel,
//     so every store instruction of a wave writes 1 KiB of whole lines; 72 / 75 VGPRs.
//                   64 KiB          1 MiB           16 MiB
//   FP32   W = 16   153.8 / 171.9   171.9 / 194.3   1039.2 / 1037.8
//          W = 4    164.8 / 175.5   171.7 / 189.6    831.8 /  825.8
//   BF16   W = 16   146.0 / 178.6   176.6 / 186.0    787.5 /  782.1
//          W = 8    178.2 / 197.3   183.5 / 187.7    772.0 /  766.1
// At 64 KiB and 1 MiB the two are within the spread of a candidate's own rounds (10-20 %: the call is a launch, a
// barrier and the host's rendezvous). At 16 MiB the narrow load is 20 % ahead for FP32 output and 2 % for BF16: with
// W = 16 a lane's FP32 stores lie 64 B apart from its neighbour's, so a store instruction writes a quarter of every
// line it touches (the supposed cause; not profiled). The narrow load is shipped (faster where they differ, and fewer VGPRs).
//
// Alignment. Slots are 16-B aligned, and with element size 1 every block window and tile starts on a multiple of 16
// elements (ipc_plan.cc: piece, blockElems and tileElems are multiples of V = 16 / es), so the slot side is always
// vector-eligible. sendBuf and recvBuf are arbitrary: a window takes the vector path when the own operand's and the
// output's addresses at the window's start are both 16-B aligned, else the element-wise loop (byte loads, the same
// arithmetic: correct and slow). A window's ragged end (fewer than W elements) is element-wise too.
//
// Residency: 72 (FP32 output) or 75 VGPRs, 106 SGPRs, no scratch, 7 or 6 waves per SIMD (amdgpu_waves_per_eu asks
// for 6; the W = 16 build had 81 VGPRs and 5 without it), so the launch cap (ipc_kernels.hip: at most 6 workgroups of
// 256 threads per CU) is k_ipc_collective's for FP32 SUM (63 VGPRs).
#include "ipc_kernel_body.h"
#include "widen_elem.h"

#ifndef HCCL_AMD_IPC_WIDEN_LOAD_BYTES
#define HCCL_AMD_IPC_WIDEN_LOAD_BYTES 0  // 0: O::kPer bytes, one output vector per unit (shipped); or 16
#endif

namespace hccl_amd {

namespace {

constexpr int kTileElems = 32;  // elements per lane and tile, whatever the load width

// A unit's load by its width in bytes, and the dwords of one.
template <int W>
struct LoadOf;
template <>
struct LoadOf<4> {
    using L = uint32_t;
};
template <>
struct LoadOf<8> {
    using L = u32x2;
};
template <>
struct LoadOf<16> {
    using L = u32x4;
};

template <class L>
__device__ __forceinline__ uint32_t Dword(L v, int d)
{
    if constexpr (std::is_same<L, uint32_t>::value) {
        return v;
    } else {
        return v[d];
    }
}

template <int NT, class L>
__device__ __forceinline__ L LoadUnit(const L* p)
{
    if constexpr ((NT & 1) != 0) {
        return __builtin_nontemporal_load(p);
    } else {
        return *p;
    }
}

// acc = f32(x) (kFirst) or f32(x) + acc, the W elements of one unit in memory order.
template <class D, int W, bool kFirst, class L>
__device__ __forceinline__ void FoldUnit(L x, float (&acc)[W])
{
#pragma unroll
    for (int d = 0; d < W / 4; ++d) {
        float f[4];
        Decode<D>(Dword(x, d), f);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * d + e] = kFirst ? f[e] : f[e] + acc[4 * d + e];
    }
}

// The U units of one lane at unit indices v, v + bt, ..: own and slots point at piece coordinate 0, slot q at
// q * piece elements. The loads of the next operand are in flight while the previous one is decoded and added.
template <class D, class O, int W, int U, int NT>
__device__ __forceinline__ void FoldTile(const uint8_t* own, const uint8_t* slots, uint64_t piece, uint32_t n,
                                         uint32_t me, typename O::S* outp, uint64_t v, uint32_t bt)
{
    using L = typename LoadOf<W>::L;
    constexpr int K = O::kPer;
    L cur[U], nxt[U];
    float acc[U][W];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = LoadUnit<NT>(reinterpret_cast<const L*>(own) + v + u * bt);
    uint32_t q = me == 0 ? 1 : 0;  // n >= 2: the first peer
#pragma unroll
    for (int u = 0; u < U; ++u) nxt[u] = LoadUnit<NT>(reinterpret_cast<const L*>(slots + q * piece) + v + u * bt);
#pragma unroll
    for (int u = 0; u < U; ++u) FoldUnit<D, W, true>(cur[u], acc[u]);
    for (;;) {
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        q += q + 1 == me ? 2 : 1;
        const bool more = q < n;
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = LoadUnit<NT>(reinterpret_cast<const L*>(slots + q * piece) + v + u * bt);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) FoldUnit<D, W, false>(cur[u], acc[u]);
        if (!more) break;
    }
    // a unit's W elements are W / K output vectors, contiguous
#pragma unroll
    for (int u = 0; u < U; ++u) {
        u32x4* o = reinterpret_cast<u32x4*>(outp) + (v + u * bt) * (W / K);
#pragma unroll
        for (int s = 0; s < W / K; ++s) {
            float t[K];
#pragma unroll
            for (int i = 0; i < K; ++i) t[i] = acc[u][s * K + i];
            st<NT>(o + s, O::pack(t));
        }
    }
}

// Elements [lo, hi) one per lane: byte loads, the same arithmetic.
template <class D, class O>
__device__ __forceinline__ void FoldElements(const uint8_t* own, const uint8_t* slots, uint64_t piece, uint32_t n,
                                             uint32_t me, typename O::S* outp, uint64_t lo, uint64_t hi, uint32_t bt)
{
    for (uint64_t e = lo + threadIdx.x; e < hi; e += bt) {
        float acc = D::one(own[e]);
        for (uint32_t q = 0; q < n; ++q) {
            if (q != me) acc = D::one(slots[q * piece + e]) + acc;
        }
        outp[e] = O::narrow(acc);
    }
}

// The fold of the window r (piece coordinates) into outp[r].
template <class D, class O, int W>
__device__ __forceinline__ void FoldWindow(const uint8_t* own, const uint8_t* slots, uint64_t piece, uint32_t n,
                                           uint32_t me, typename O::S* outp, Range r, bool nt, uint32_t bt)
{
    constexpr int U = kTileElems / W;
    // r.lo is a multiple of 16 elements unless the window is empty at the end of a piece (lo = hi = len)
    const bool vec = ((reinterpret_cast<uintptr_t>(own + r.lo) | reinterpret_cast<uintptr_t>(slots + r.lo) |
                       reinterpret_cast<uintptr_t>(outp + r.lo)) & 15u) == 0;
    const uint64_t ulo = r.lo / W, uhi = vec ? max(ulo, r.hi / W) : ulo;
    uint64_t v = ulo + threadIdx.x;
    auto body = [&](auto ntTag) {
        constexpr int NT = decltype(ntTag)::value;
        for (; v + uint64_t(U - 1) * bt < uhi; v += uint64_t(U) * bt) {
            FoldTile<D, O, W, U, NT>(own, slots, piece, n, me, outp, v, bt);
        }
        for (; v < uhi; v += bt) FoldTile<D, O, W, 1, NT>(own, slots, piece, n, me, outp, v, bt);
    };
    if (nt) {
        body(std::integral_constant<int, 3>{});
    } else {
        body(std::integral_constant<int, 0>{});
    }
    FoldElements<D, O>(own, slots, piece, n, me, outp, max(uhi * W, r.lo), r.hi, bt);
}

template <class D, class O, int W>
__global__ __launch_bounds__(kIpcMaxThreads) __attribute__((amdgpu_waves_per_eu(6))) void k_ipc_widen(IpcArgs a)
{
    using S = typename O::S;
    const uint32_t n = a.n, kind = a.kind;  // n >= 2: the operators fold a one-rank call on the host (ops.cc)
    const uint32_t me = a.me >= 0 ? static_cast<uint32_t>(a.me) : blockIdx.y;
    const uint8_t* in = static_cast<const uint8_t*>(a.in[me]);
    S* out = static_cast<S*>(a.out[me]);
    const bool nt = a.nt != 0;
    const uint32_t bt = a.threads;
    // the sticky bit and the epoch counter as in k_ipc_collective
    const uint32_t sticky = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint32_t epoch = __hip_atomic_load(a.status + kIpcEpochWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((sticky & 1u) != 0) return;
    Stamp(a, me, kTrEntry);
    const uint32_t arrivedBefore = Arrive(a, epoch);
    uint32_t waitMax = 0;
    auto aligned = [](const void* p, const void* q) {
        return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15u) == 0;
    };
    for (uint32_t k = 0; k < a.rounds; ++k) {
        const uint64_t kP = uint64_t(k) * a.piece;
        const uint32_t par = (epoch + 1) & 1u;
        Stamp(a, me, kTrRound);
        // the peers in an order rotated by the block, so the blocks spread their stores over the links
        auto peer = [&](uint32_t i) { return (me + 1 + (i + blockIdx.x) % (n - 1)) % n; };
        auto slotOn = [&](uint32_t c) { return static_cast<uint8_t*>(a.stgAlt[par][c]) + uint64_t(me) * a.piece; };
        if (kind == kIpcAllReduceOneShot) {
            const uint8_t* src = in + kP;
            const bool vec = aligned(src, nullptr);
            ForBlockShare(a, PieceLen(a, me, kP), [&](Range r) {
                CopyRangeTo<uint8_t>([&](uint32_t d) { return slotOn(peer(d)); }, n - 1, src, r, vec, nt, bt);
            });
        } else {
            for (uint32_t i = 0; i + 1 < n; ++i) {
                const uint32_t c = peer(i);
                if (kind == kIpcReduceOneShot && c != a.root) continue;
                const uint8_t* src = in + ChunkStart(a, c) + kP;
                uint8_t* slot = slotOn(c);
                const bool vec = aligned(src, slot);
                ForBlockShare(a, PieceLen(a, c, kP), [&](Range r) { CopyRange<uint8_t>(slot, src, r, vec, nt, bt); });
            }
        }
        Stamp(a, me, kTrPhase0);
        const FlagLane fl = LaneFlags(a, me);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier1);
        if (!(kind == kIpcReduceOneShot && me != a.root)) {
            const uint8_t* own = in + ChunkStart(a, me) + kP;
            const uint8_t* slots = static_cast<const uint8_t*>(a.stgAlt[epoch & 1u][me]);
            S* dst = kind == kIpcReduceScatter ? out + kP : out + ChunkStart(a, me) + kP;
            ForBlockShare(a, PieceLen(a, me, kP),
                          [&](Range r) { FoldWindow<D, O, W>(own, slots, a.piece, n, me, dst, r, nt, bt); });
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

template <class O>
constexpr int LoadBytes()
{
    return HCCL_AMD_IPC_WIDEN_LOAD_BYTES != 0 ? HCCL_AMD_IPC_WIDEN_LOAD_BYTES : O::kPer;
}

}  // namespace

hipError_t LaunchIpcWiden(HcclDataType inType, HcclDataType outType, const IpcArgs& a, dim3 grid, hipStream_t s)
{
    if (!IsWidenPair(inType, outType)) return hipErrorInvalidValue;
    return WithWidenPair(inType, outType, [&](auto d, auto o) {
        using O = decltype(o);
        hipLaunchKernelGGL((k_ipc_widen<decltype(d), O, LoadBytes<O>()>), grid, dim3(a.threads), 0, s, a);
        return hipGetLastError();
    });
}

const void* IpcWidenKernel(HcclDataType inType, HcclDataType outType)
{
    return WithWidenPair(inType, outType, [](auto d, auto o) {
        using O = decltype(o);
        return reinterpret_cast<const void*>(&k_ipc_widen<decltype(d), O, LoadBytes<O>()>);
    });
}

}  // namespace hccl_amd
