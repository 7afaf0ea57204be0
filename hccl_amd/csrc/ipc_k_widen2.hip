// ipc_k_widen2.hip — the one-sided two-shot widening FP8 AllReduce (HcclAmdAllReduceWiden under
// HCCL_AMD_ALGO_IPC_TWOSHOT): the two-barrier kind kIpcAllReduce in order O2 with FP8 operands (E4M3 / E5M2) and an
// FP32 / BF16 / FP16 result. The owner of a chunk folds it once and every rank receives the owner's bytes, so every
// rank holds the same result, NaN payloads included, and a rank folds 1/n of the elements.
//
// A kernel of its own beside k_ipc_widen (the single-barrier one-shot kinds), so that neither lowers the other's
// occupancy. It shares the barrier, the epoch counter, the sticky-bit check, the block windows, Stamp / PublishWait /
// EndLaunch and the typeless copy loop with the other kinds (ipc_kernel_body.h), and the decode and narrowing with the
// local kernel (widen_elem.h). It adds no protocol: the slots lie in stgIn and the results in stgRes, as in the
// same-type two-shot (k_ipc_collective, kind kIpcAllReduce), and the two barriers per round are that kind's.
//
// The host plans the call as the same-type two-shot AllReduce at the OUTPUT type's element size (ipc.cc), so every
// length below (piece, blockElems, tileElems, the chunk starts) counts elements and is a multiple of
// 16 / sizeof(output) = O::kPer elements. The same number is a byte offset on the FP8 side and an index on the wide
// side. Per round of `piece` elements, rank `me`:
//   push      for every chunk c != me, the FP8 bytes of chunk c's piece into slot `me` of stgIn[c] (slot q at q * piece
//             bytes: the FP8 slots use 1 / sizeof(output) of the area), the peers in an order rotated by the block.
//             A byte copy: the data travels as FP8, every access to a peer is a store, the own chunk is not staged.
//   barrier 1
//   fold      chunk `me` in order O2: acc = f32(x_0); acc = f32(x_q) + acc, q = 1 .. n-1; out = narrow(acc). x_me comes
//             from sendBuf, the others from the slots. The narrowed 16-B vector goes from registers to n places:
//             recvBuf at the chunk's position and stgRes[p] + me * piece (wide elements) on every peer p, rotated by
//             the block. The owner never reads its wide result again.
//   barrier 2
//   copy out  the n - 1 other chunks of the round from stgRes[me] into recvBuf, at the output type's element size.
//
// The fold. A lane's unit is one load of W = O::kPer bytes per operand (4 for FP32 output, 8 for the 16-bit types),
// which is exactly one 16-B output vector, so every one of the n stores of a wave writes 1 KiB of whole lines.
// Consecutive lanes own consecutive units; a tile is kTileElems elements per lane (U = kTileElems / W units, `threads`
// units apart). All of an operand's loads of a tile are issued before any is decoded, and operand q + 1 is loaded
// while operand q is folded (k_ipc_widen's software pipeline). The tile's U vectors are packed once and then stored
// destination by destination, so a destination's stores of a tile are back to back. No LDS (nothing is reused); plain
// FP32 adds in operand order (no fast-math, denormals kept, packed FP32 adds off for this file: Makefile); loads and
// stores are non-temporal when IpcArgs::nt says so.
//
// Alignment. Every window starts on a multiple of W elements: W-byte aligned for the FP8 loads from the slots, 16-B
// aligned for the wide stores into stgRes. sendBuf and recvBuf are arbitrary: a window takes the vector path when the
// own operand's address at the window's start is W-byte aligned and the output's 16-B aligned (a 16-B aligned sendBuf
// and recvBuf give both in every round), else the element-wise loop (byte loads, the same arithmetic, every element
// stored to all n destinations: correct and slow). A window's ragged end (fewer than W elements) is element-wise too.
// The push's windows start W-byte aligned as well, and a slot or a later round's source need not be 16-B aligned (a
// piece cut by the slot capacity is a multiple of W only): PushRange copies 16-B vectors through the shared loop when
// both sides allow it, else W-byte words, else bytes.
//
// Residency (-Rpass-analysis=kernel-resource-usage, gfx950; DESIGN.md §3.5 has the table): 74 VGPRs (FP32 output) or
// 71, 106 SGPRs, no scratch, 6 or 7 waves per SIMD in the six instantiations (amdgpu_waves_per_eu(6) as in
// k_ipc_widen). The launch cap comes from this kernel's own occupancy query (IpcWiden2ResidentBlocks, ipc_kernels.hip).
#include "ipc_kernel_body.h"
#include "widen_elem.h"

namespace hccl_amd {

namespace {

// Elements per lane and tile, from the VGPR report: 32 (k_ipc_widen's) takes 82 / 83 VGPRs here, since the packed
// vectors stay live over the n stores, which under amdgpu_waves_per_eu(6) (80 VGPRs) spills 12 bytes per lane to
// scratch; 24 takes 74 / 71 with none, 16 takes 62 / 61. 24 keeps the most loads in flight at 6 waves per SIMD.
constexpr int kTileElems = 24;

template <int NT, class L>
__device__ __forceinline__ L LoadUnit(const L* p)
{
    if constexpr ((NT & 1) != 0) {
        return __builtin_nontemporal_load(p);
    } else {
        return *p;
    }
}

// The U units of one lane at unit indices v, v + bt, ..: operand q of the O2 fold is `own` for q == me, else slot q
// (slots + q * piece bytes); all at piece coordinate 0. One unit is W bytes in and one 16-B vector out. dst(d), d < n,
// is where the results go (wide elements, piece coordinate 0): recvBuf at the chunk's position for d = 0, then slot
// `me` of every peer's result area. It reads the pointer table in the kernel arguments with a uniform index.
template <class D, class O, int U, int NT, class Dst>
__device__ __forceinline__ void FoldTile(const uint8_t* own, const uint8_t* slots, uint64_t piece, uint32_t n,
                                         uint32_t me, const Dst& dst, uint64_t v, uint32_t bt)
{
    using L = typename O::L;
    constexpr int W = O::kPer;
    auto src = [&](uint32_t q) { return reinterpret_cast<const L*>(q == me ? own : slots + q * piece); };
    L cur[U], nxt[U];
    float acc[U][W];
    {
        const L* s0 = src(0);
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = LoadUnit<NT>(s0 + v + u * bt);
        const L* s1 = src(1);  // n >= 2
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = LoadUnit<NT>(s1 + v + u * bt);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) Decode<D>(cur[u], acc[u]);
    for (uint32_t q = 1;;) {
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        const bool more = ++q < n;
        if (more) {
            const L* s = src(q);
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = LoadUnit<NT>(s + v + u * bt);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float f[W];
            Decode<D>(cur[u], f);
#pragma unroll
            for (int e = 0; e < W; ++e) acc[u][e] = f[e] + acc[u][e];
        }
        if (!more) break;
    }
    u32x4 res[U];
#pragma unroll
    for (int u = 0; u < U; ++u) res[u] = O::pack(acc[u]);
    for (uint32_t d = 0; d < n; ++d) {
        u32x4* o = reinterpret_cast<u32x4*>(dst(d)) + v;
#pragma unroll
        for (int u = 0; u < U; ++u) st<NT>(o + u * bt, res[u]);
    }
}

// Elements [lo, hi) one per lane: byte loads, the same arithmetic, every destination.
template <class D, class O, class Dst>
__device__ __forceinline__ void FoldElements(const uint8_t* own, const uint8_t* slots, uint64_t piece, uint32_t n,
                                             uint32_t me, const Dst& dst, uint64_t lo, uint64_t hi,
                                             uint32_t bt)
{
    for (uint64_t e = lo + threadIdx.x; e < hi; e += bt) {
        float acc = D::one(me == 0 ? own[e] : slots[e]);
        for (uint32_t q = 1; q < n; ++q) acc = D::one(q == me ? own[e] : slots[q * piece + e]) + acc;
        const typename O::S x = O::narrow(acc);
        for (uint32_t d = 0; d < n; ++d) dst(d)[e] = x;
    }
}

// The fold of the window r (piece coordinates) into every destination's [r].
template <class D, class O, class Dst>
__device__ __forceinline__ void FoldWindow(const uint8_t* own, const uint8_t* slots, uint64_t piece, uint32_t n,
                                           uint32_t me, const Dst& dst, Range r, bool nt, uint32_t bt)
{
    constexpr int W = O::kPer, U = kTileElems / W;
    // r.lo is a multiple of W elements unless the window is empty at the end of a piece (lo = hi = len); the slots and
    // the result areas are then W-byte and 16-B aligned there, the user buffers are whatever the caller passed
    const bool vec = r.lo % W == 0 && (reinterpret_cast<uintptr_t>(own + r.lo) & (W - 1)) == 0 &&
                     (reinterpret_cast<uintptr_t>(dst(0) + r.lo) & 15u) == 0;
    const uint64_t ulo = r.lo / W, uhi = vec ? max(ulo, r.hi / W) : ulo;
    uint64_t v = ulo + threadIdx.x;
    auto body = [&](auto ntTag) {
        constexpr int NT = decltype(ntTag)::value;
        for (; v + uint64_t(U - 1) * bt < uhi; v += uint64_t(U) * bt) {
            FoldTile<D, O, U, NT>(own, slots, piece, n, me, dst, v, bt);
        }
        for (; v < uhi; v += bt) FoldTile<D, O, 1, NT>(own, slots, piece, n, me, dst, v, bt);
    };
    if (nt) {
        body(std::integral_constant<int, 3>{});
    } else {
        body(std::integral_constant<int, 0>{});
    }
    FoldElements<D, O>(own, slots, piece, n, me, dst, max(uhi * W, r.lo), r.hi, bt);
}

// dst[e] = src[e] for the bytes e in r, whose start is a multiple of sizeof(L) = W. Both pointers (piece coordinate 0)
// 16-B aligned: up to the next 16-B boundary one by one, then the shared copy loop. Both W-byte aligned: W-byte words.
// Else bytes.
template <class L>
__device__ __forceinline__ void PushRange(uint8_t* dst, const uint8_t* src, Range r, bool nt, uint32_t bt)
{
    constexpr uint64_t W = sizeof(L);
    const uintptr_t both = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
    if ((both & 15u) == 0) {
        const uint64_t mid = min(r.hi, (r.lo + 15) / 16 * 16);
        for (uint64_t e = r.lo + threadIdx.x; e < mid; e += bt) dst[e] = src[e];
        CopyRange<uint8_t>(dst, src, Range{mid, r.hi}, true, nt, bt);
        return;
    }
    const bool words = (both & (W - 1)) == 0 && r.lo % W == 0;
    const uint64_t ulo = r.lo / W, uhi = words ? max(ulo, r.hi / W) : ulo;
    for (uint64_t u = ulo + threadIdx.x; u < uhi; u += bt) reinterpret_cast<L*>(dst)[u] = reinterpret_cast<const L*>(src)[u];
    for (uint64_t e = max(uhi * W, r.lo) + threadIdx.x; e < r.hi; e += bt) dst[e] = src[e];
}

template <class D, class O>
__global__ __launch_bounds__(kIpcMaxThreads) __attribute__((amdgpu_waves_per_eu(6))) void k_ipc_widen2(IpcArgs a)
{
    using S = typename O::S;
    const uint32_t n = a.n;  // n >= 2: the operators fold a one-rank call on the host (ops.cc)
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
    // the peers in an order rotated by the block, so the blocks spread their stores over the links
    auto peer = [&](uint32_t i) { return (me + 1 + (i + blockIdx.x) % (n - 1)) % n; };
    for (uint32_t k = 0; k < a.rounds; ++k) {
        const uint64_t kP = uint64_t(k) * a.piece;
        Stamp(a, me, kTrRound);
        // push: my FP8 bytes of chunk c's piece -> slot `me` of owner c
        for (uint32_t i = 0; i + 1 < n; ++i) {
            const uint32_t c = peer(i);
            const uint8_t* src = in + ChunkStart(a, c) + kP;
            uint8_t* slot = static_cast<uint8_t*>(a.stgIn[c]) + uint64_t(me) * a.piece;
            ForBlockShare(a, PieceLen(a, c, kP), [&](Range r) { PushRange<typename O::L>(slot, src, r, nt, bt); });
        }
        Stamp(a, me, kTrPhase0);
        const FlagLane fl = LaneFlags(a, me);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier1);
        // fold and spread: my chunk's piece, to my recvBuf and to every peer's result area
        {
            const uint8_t* own = in + ChunkStart(a, me) + kP;
            const uint8_t* slots = static_cast<const uint8_t*>(a.stgIn[me]);
            S* first = out + ChunkStart(a, me) + kP;
            auto dst = [&](uint32_t d) {
                return d == 0 ? first : static_cast<S*>(a.stgRes[peer(d - 1)]) + uint64_t(me) * a.piece;
            };
            ForBlockShare(a, PieceLen(a, me, kP),
                          [&](Range r) { FoldWindow<D, O>(own, slots, a.piece, n, me, dst, r, nt, bt); });
        }
        Stamp(a, me, kTrPhase1);
        if (!Barrier(a, fl, ++epoch, waitMax)) break;
        Stamp(a, me, kTrBarrier2);
        // copy out: the other chunks' results from my own result area
        for (uint32_t c = 0; c < n; ++c) {
            if (c == me) continue;
            S* dstC = out + ChunkStart(a, c) + kP;
            const S* res = static_cast<const S*>(a.stgRes[me]) + uint64_t(c) * a.piece;
            const bool vec = aligned(dstC, res);
            ForBlockShare(a, PieceLen(a, c, kP), [&](Range r) { CopyRange<S>(dstC, res, r, vec, nt, bt); });
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

}  // namespace

hipError_t LaunchIpcWiden2(HcclDataType inType, HcclDataType outType, const IpcArgs& a, dim3 grid, hipStream_t s)
{
    if (!IsWidenPair(inType, outType)) return hipErrorInvalidValue;
    return WithWidenPair(inType, outType, [&](auto d, auto o) {
        hipLaunchKernelGGL((k_ipc_widen2<decltype(d), decltype(o)>), grid, dim3(a.threads), 0, s, a);
        return hipGetLastError();
    });
}

const void* IpcWiden2Kernel(HcclDataType inType, HcclDataType outType)
{
    return WithWidenPair(inType, outType, [](auto d, auto o) {
        return reinterpret_cast<const void*>(&k_ipc_widen2<decltype(d), decltype(o)>);
    });
}

}  // namespace hccl_amd
