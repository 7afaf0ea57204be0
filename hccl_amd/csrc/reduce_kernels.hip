// reduce_kernels.hip — the element-wise reduce at the bottom of every HCCL reducing schedule, for CDNA4 (gfx950).
//
// Replaces:
//   AicpuReduceTemplate<T> / AicpuReduceFp16 / AicpuReduce  alg_data_trans_wrapper.cc:1232-1353 (CPU scalar loop)
//   LocalReduce -> HcommLocalReduceOnThread                  alg_data_trans_wrapper.cc:901-928 (external SDMA task)
//   AivCommBase::CpGM2GM(atomic) / Reduce64                  aiv_communication_base_v2.h:527-616 (AIV vector core)
//
// This is a pure HBM stream (1 flop per 12 B for fp32), so the design is about bytes in flight, not math:
//   * every lane moves 16-B vectors (global_load_dwordx4 / global_store_dwordx4), a wave 1 KiB per instruction;
//   * each lane issues all U loads of both operands of a tile before the first combine (2*U*16 B in flight per lane);
//   * a persistent grid of blocksPerCu x CUs workgroups of 256 threads walks the tiles (grid-stride), so the launch
//     is a fixed ~1-2k workgroups whatever the size;
//   * every vector load and store is non-temporal (NT = 3): each stream is touched once;
//   * no LDS: staging a pure stream through LDS adds a round trip and buys no reuse (measured in DESIGN.md).
// Element rules are AicpuReduceTemplate's: dst = src (op) dst with std::max/std::min operand semantics (ties and NaN
// yield src), integer SUM/PROD wrap, fp16/bf16 computed as fp32 then rounded to nearest even. No fast-math: fp32
// denormals are preserved (checked in the code object: .amdhsa_float_denorm_mode_32 = 3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

#include "internal.h"
#include "reduce_elem.h"

namespace hccl_amd {


// Scalar elements outside the 16-B aligned body (head < 16 B before it, tail < 16 B after it): done by one block.
struct Edges {
    uint32_t head;  // elements before the vector body
    uint32_t tail;  // elements after it
    uint64_t tailStart;
};

constexpr int kBlock = 256;

// ------------------------------------------------------------------------------------------------ out = src (op) dst

// Tiles are dealt round-robin to the persistent grid (the chip-wide access front stays a few MiB wide).
template <class E, int OP, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_reduce2(typename E::S* out, const typename E::S* src,
                                                      const typename E::S* dst, uint64_t nvec, Edges edges)
{
    constexpr uint64_t kTile = uint64_t(kBlock) * U;
    // vector body starts after the head elements
    u32x4* vout = reinterpret_cast<u32x4*>(out + edges.head);
    const u32x4* vsrc = reinterpret_cast<const u32x4*>(src + edges.head);
    const u32x4* vdst = reinterpret_cast<const u32x4*>(dst + edges.head);
    const uint64_t fullTiles = nvec / kTile;
    const uint64_t nblocks = gridDim.x;
    for (uint64_t t = blockIdx.x; t < fullTiles; t += nblocks) {
        const uint64_t base = t * kTile + threadIdx.x;
        u32x4 a[U];
        u32x4 b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a[u] = ld<NT>(vsrc + base + u * kBlock);
            b[u] = ld<NT>(vdst + base + u * kBlock);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            st<NT>(vout + base + u * kBlock, combine<E, OP>(a[u], b[u]));
        }
    }
    for (uint64_t i = fullTiles * kTile + uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < nvec;
         i += uint64_t(gridDim.x) * kBlock) {
        st<NT>(vout + i, combine<E, OP>(ld<NT>(vsrc + i), ld<NT>(vdst + i)));
    }
    if (blockIdx.x == 0) {
        uint32_t tid = threadIdx.x;
        if (tid < edges.head) {
            out[tid] = E::template ap<OP>(src[tid], dst[tid]);
        } else if (tid >= 64 && tid - 64 < edges.tail) {
            uint64_t i = edges.tailStart + (tid - 64);
            out[i] = E::template ap<OP>(src[i], dst[i]);
        }
    }
}

// Fallback when the three pointers are not congruent modulo 16 B: one element per lane, grid-stride.
template <class E, int OP>
__global__ __launch_bounds__(kBlock) void k_reduce2_scalar(typename E::S* out, const typename E::S* src,
                                                             const typename E::S* dst, uint64_t count)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += uint64_t(gridDim.x) * kBlock) {
        out[i] = E::template ap<OP>(src[i], dst[i]);
    }
}

// ------------------------------------------------------------------------------------------------ ordered n-ary fold

struct SrcPack {
    const void* p[HCCL_AMD_IR_MAX_SRC];
};

// Vector body of operand j (16-B vectors from the first aligned element).
template <class E>
__device__ __forceinline__ const u32x4* VecSrc(const SrcPack& srcs, int j, const Edges& edges)
{
    return reinterpret_cast<const u32x4*>(static_cast<const typename E::S*>(srcs.p[j]) + edges.head);
}

// Fold of one tile (U vectors per lane at base, base + kBlock, ...) over the operands, in operand order
// (acc = x_j (op) acc). Operand j+1 is loaded once operand j is folded, so a wave has U vectors of loads in flight.
// Measured against a prefetching form and against issuing every operand's loads first
// (profiles/r02_ab_fold_modes.jsonl): neither was faster.
template <class E, int OP, int U, int NT>
__device__ __forceinline__ void FoldTile(u32x4 (&acc)[U], const SrcPack& srcs, int nsrc, const Edges& edges,
                                         uint64_t base)
{
    const u32x4* p0 = VecSrc<E>(srcs, 0, edges);
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = ld<NT>(p0 + base + u * kBlock);
    for (int j = 1; j < nsrc; ++j) {
        const u32x4* pj = VecSrc<E>(srcs, j, edges);
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = ld<NT>(pj + base + u * kBlock);
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = combine<E, OP>(v[u], acc[u]);
    }
}

// The vectors [first, nvec) after a fold's last full tile, one per lane, strided over the `nblocks` workgroups.
template <class E, int OP, int NT>
__device__ __forceinline__ void FoldLeftover(typename E::S* out, const SrcPack& srcs, int nsrc, const Edges& edges,
                                             uint64_t first, uint64_t nvec, uint32_t bid, uint32_t nblocks)
{
    u32x4* vout = reinterpret_cast<u32x4*>(out + edges.head);
    for (uint64_t i = first + uint64_t(bid) * kBlock + threadIdx.x; i < nvec; i += uint64_t(nblocks) * kBlock) {
        u32x4 acc = ld<NT>(VecSrc<E>(srcs, 0, edges) + i);
        for (int j = 1; j < nsrc; ++j) {
            acc = combine<E, OP>(ld<NT>(VecSrc<E>(srcs, j, edges) + i), acc);
        }
        st<NT>(vout + i, acc);
    }
}

// The scalar head and tail of a fold, by the one workgroup that calls this: lanes 0.. take the head elements, lanes
// 64.. (another wave) the tail's.
template <class E, int OP>
__device__ __forceinline__ void FoldEdges(typename E::S* out, const SrcPack& srcs, int nsrc, const Edges& edges)
{
    using S = typename E::S;
    const uint32_t tid = threadIdx.x;
    const bool head = tid < edges.head;
    if (head || (tid >= 64 && tid - 64 < edges.tail)) {
        const uint64_t i = head ? tid : edges.tailStart + (tid - 64);
        S acc = static_cast<const S*>(srcs.p[0])[i];
        for (int j = 1; j < nsrc; ++j) {
            acc = E::template ap<OP>(static_cast<const S*>(srcs.p[j])[i], acc);
        }
        out[i] = acc;
    }
}

// One ordered fold over `nvec` 16-B vectors (plus scalar edges), worked by `nblocks` workgroups, this one `bid`:
// tiles dealt round-robin over the grid.
template <class E, int OP, int U, int NT>
__device__ __forceinline__ void ReduceNBody(typename E::S* out, const SrcPack& srcs, int nsrc, uint64_t nvec,
                                            Edges edges, uint32_t bid, uint32_t nblocks)
{
    constexpr uint64_t kTile = uint64_t(kBlock) * U;
    u32x4* vout = reinterpret_cast<u32x4*>(out + edges.head);
    const uint64_t fullTiles = nvec / kTile;
    const uint64_t tStep = nblocks;
    for (uint64_t t = bid; t < fullTiles; t += tStep) {
        const uint64_t base = t * kTile + threadIdx.x;
        u32x4 acc[U];
        FoldTile<E, OP, U, NT>(acc, srcs, nsrc, edges, base);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            st<NT>(vout + base + u * kBlock, acc[u]);
        }
    }
    FoldLeftover<E, OP, NT>(out, srcs, nsrc, edges, fullTiles * kTile, nvec, bid, nblocks);
    if (bid == 0) FoldEdges<E, OP>(out, srcs, nsrc, edges);
}

template <class E, int OP, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_reduceN(typename E::S* out, SrcPack srcs, int nsrc, uint64_t nvec,
                                                      Edges edges)
{
    ReduceNBody<E, OP, U, NT>(out, srcs, nsrc, nvec, edges, blockIdx.x, gridDim.x);
}

// A batch of independent folds (one schedule step's), in one of two layouts chosen by segment size (RunBatch):
// * flat (k_reduceN_batch): the segments' full tiles are one concatenated tile space that the whole grid strides over,
//   as a single fold would; at any moment the workgroups sit in a window of consecutive tiles, one or two segments
//   wide, so the DRAM sees a few operand streams instead of every segment's at once; each segment's leftover vectors
//   and scalar edges follow, spread over the grid;
// * rows (k_reduceN_batch_rows): a grid row per segment.
// Measured (7 segments; profiles/r02_batch_fold_layout_ab.txt, taken with tools/probes/batch_fold_bench.py, which is in
// git history at bb0e1f4): at 4 and 16 MiB segments flat runs 6.1-6.5 TB/s against rows' 5.5-6.1 (2 and 8 operands); at
// 1-2 MiB rows is as fast or faster, and beside the RCCL kernels of a self-loop MeshChunk program (1.8 MiB sub-slices)
// rows' folds took 0.95-1.0 ms against flat's 1.4.
constexpr uint64_t kBatchFlatSegBytes = 4ull << 20;  // segments this large (on average) take the flat layout

struct BatchPack {
    void* out[kMaxBatchSegs];
    SrcPack srcs[kMaxBatchSegs];
    uint64_t nvec[kMaxBatchSegs];
    Edges edges[kMaxBatchSegs];
    uint64_t tileStart[kMaxBatchSegs + 1];  // prefix sums of the segments' full tiles
    int nseg;
    int nsrc;
};

// The other layout: one grid row (blockIdx.y) per segment, each row striding over its own segment.
template <class E, int OP, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_reduceN_batch_rows(BatchPack pk)
{
    const uint32_t g = blockIdx.y;
    ReduceNBody<E, OP, U, NT>(static_cast<typename E::S*>(pk.out[g]), pk.srcs[g], pk.nsrc, pk.nvec[g], pk.edges[g],
                              blockIdx.x, gridDim.x);
}

template <class E, int OP, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_reduceN_batch(BatchPack pk)
{
    using S = typename E::S;
    constexpr uint64_t kTile = uint64_t(kBlock) * U;
    const uint32_t bid = blockIdx.x, nblocks = gridDim.x;
    int g = 0;
    for (uint64_t t = bid; t < pk.tileStart[pk.nseg]; t += nblocks) {
        while (t >= pk.tileStart[g + 1]) ++g;  // t only grows: the segment index only moves forward
        const uint64_t base = (t - pk.tileStart[g]) * kTile + threadIdx.x;
        u32x4 acc[U];
        FoldTile<E, OP, U, NT>(acc, pk.srcs[g], pk.nsrc, pk.edges[g], base);
        u32x4* vout = reinterpret_cast<u32x4*>(static_cast<S*>(pk.out[g]) + pk.edges[g].head);
#pragma unroll
        for (int u = 0; u < U; ++u) st<NT>(vout + base + u * kBlock, acc[u]);
    }
    for (int h = 0; h < pk.nseg; ++h) {
        S* out = static_cast<S*>(pk.out[h]);
        FoldLeftover<E, OP, NT>(out, pk.srcs[h], pk.nsrc, pk.edges[h], (pk.tileStart[h + 1] - pk.tileStart[h]) * kTile,
                                pk.nvec[h], bid, nblocks);
        // the scalar head and tail of segment h, the segments' edges dealt over the grid
        if (bid == uint32_t(h) % nblocks) FoldEdges<E, OP>(out, pk.srcs[h], pk.nsrc, pk.edges[h]);
    }
}

template <class E, int OP>
__global__ __launch_bounds__(kBlock) void k_reduceN_scalar(typename E::S* out, SrcPack srcs, int nsrc, uint64_t count)
{
    using S = typename E::S;
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += uint64_t(gridDim.x) * kBlock) {
        S acc = static_cast<const S*>(srcs.p[0])[i];
        for (int j = 1; j < nsrc; ++j) {
            acc = E::template ap<OP>(static_cast<const S*>(srcs.p[j])[i], acc);
        }
        out[i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ host launch

int CuCount(bool* ok)
{
    static std::mutex mu;
    static int cached[64] = {0};  // 0 = not answered yet
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        std::lock_guard<std::mutex> lk(mu);
        n = cached[dev];
        if (n == 0) {
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 0) n = 0;
            cached[dev] = n;
        }
    }
    if (ok != nullptr) *ok = n > 0;
    return n > 0 ? n : 256;
}

namespace {

// Launch shape of one kernel family: workgroups per CU in the persistent grid, 16-B vectors per lane per operand per
// iteration (U) and cache policy bits (NT). Fixed at compile time: every (dtype, op) pair has one kernel per family.
struct LaunchCfg {
    uint32_t blocksPerCu;
    uint32_t unroll;
    uint32_t nt;
};

// From the interleaved launch sweep on MI355X (profiles/r01_sweep_local_reduce.jsonl; its driver,
// tools/probes/sweep_local.py, is in git history at bb0e1f4): the HBM stream peaks with ~16 KiB of loads in flight per
// CU (2 workgroups x 256 lanes x 2 operands x 16 B) and nt loads+stores; more bytes in flight lowers throughput.
constexpr LaunchCfg kCfg2{2, 1, 3};
// The n-ary fold's input loop is serial per wave (input j+1 is loaded after input j is folded), so its loads in flight
// per CU are blocksPerCu x waves x U vectors, whatever n is. Two inputs behave like the 2-input kernel (U = 1 best);
// from three inputs up, U = 4 keeps enough bytes in flight (profiles/r01_sweep_fold_launch.jsonl, taken with
// tools/probes/sweep_fold_launch.py, in git history at bb0e1f4; interleaved rounds, fp32 SUM, 1 GiB per input: n = 2
// 498 vs 554 us at U = 2; n = 3 714 vs 745; n = 4 913 vs 927; n = 8 1709 vs 1787).
constexpr LaunchCfg kCfgN{2, 4, 3};

uint32_t GridFor(uint64_t work, uint32_t perBlock, const LaunchCfg& cfg)
{
    uint64_t need = (work + perBlock - 1) / perBlock;
    uint64_t cap = uint64_t(CuCount()) * cfg.blocksPerCu;
    if (need > cap) need = cap;
    if (need == 0) need = 1;
    return static_cast<uint32_t>(need);
}

// Split [0, count) elements of `es` bytes into head / 16-B vector body / tail for pointers that share one alignment
// phase.
bool SplitAligned(const void* const* ptrs, int n, uint64_t count, uint64_t es, Edges* e, uint64_t* nvec)
{
    const uint64_t kVec = 16 / es;
    uintptr_t phase = reinterpret_cast<uintptr_t>(ptrs[0]) & 15u;
    for (int i = 1; i < n; ++i) {
        if ((reinterpret_cast<uintptr_t>(ptrs[i]) & 15u) != phase) return false;
    }
    if (phase % es != 0) return false;
    uint64_t head = phase == 0 ? 0 : (16 - phase) / es;
    if (head > count) head = count;
    uint64_t rest = count - head;
    *nvec = rest / kVec;
    e->head = static_cast<uint32_t>(head);
    e->tailStart = head + *nvec * kVec;
    e->tail = static_cast<uint32_t>(count - e->tailStart);
    return true;
}

template <class E, int OP>
hipError_t Run2(void* out, const void* src, const void* dst, uint64_t count, hipStream_t stream)
{
    using S = typename E::S;
    const void* ptrs[3] = {out, src, dst};
    Edges edges{};
    uint64_t nvec = 0;
    if (!SplitAligned(ptrs, 3, count, sizeof(S), &edges, &nvec)) {
        uint32_t grid = GridFor(count, kBlock * 4, kCfg2);
        hipLaunchKernelGGL((k_reduce2_scalar<E, OP>), dim3(grid), dim3(kBlock), 0, stream, static_cast<S*>(out),
                           static_cast<const S*>(src), static_cast<const S*>(dst), count);
        return hipGetLastError();
    }
    uint32_t grid = GridFor(nvec, kBlock * kCfg2.unroll, kCfg2);
    hipLaunchKernelGGL((k_reduce2<E, OP, kCfg2.unroll, kCfg2.nt>), dim3(grid), dim3(kBlock), 0, stream,
                       static_cast<S*>(out), static_cast<const S*>(src), static_cast<const S*>(dst), nvec, edges);
    return hipGetLastError();
}

// n >= 3: LaunchReduceN sends one operand to the copy kernel and two to Run2.
template <class E, int OP>
hipError_t RunN(void* out, const void* const* srcs, uint32_t n, uint64_t count, hipStream_t stream)
{
    using S = typename E::S;
    SrcPack pk{};
    const void* ptrs[HCCL_AMD_IR_MAX_SRC + 1];
    ptrs[0] = out;
    for (uint32_t j = 0; j < n; ++j) {
        pk.p[j] = srcs[j];
        ptrs[j + 1] = srcs[j];
    }
    Edges edges{};
    uint64_t nvec = 0;
    if (!SplitAligned(ptrs, int(n) + 1, count, sizeof(S), &edges, &nvec)) {
        uint32_t grid = GridFor(count, kBlock * 4, kCfgN);
        hipLaunchKernelGGL((k_reduceN_scalar<E, OP>), dim3(grid), dim3(kBlock), 0, stream, static_cast<S*>(out), pk,
                           int(n), count);
        return hipGetLastError();
    }
    uint32_t grid = GridFor(nvec, kBlock * kCfgN.unroll, kCfgN);
    hipLaunchKernelGGL((k_reduceN<E, OP, kCfgN.unroll, kCfgN.nt>), dim3(grid), dim3(kBlock), 0, stream,
                       static_cast<S*>(out), pk, int(n), nvec, edges);
    return hipGetLastError();
}

template <class E, int OP>
hipError_t RunBatch(const BatchPack& pk, uint32_t nseg, uint64_t maxVec, hipStream_t stream)
{
    BatchPack p = pk;
    p.nseg = int(nseg);
    uint64_t totalVec = 0;
    for (uint32_t g = 0; g < nseg; ++g) totalVec += pk.nvec[g];
    if (totalVec * 16 / nseg < kBatchFlatSegBytes) {  // 16-B vectors: the average segment's bytes
        // rows: the per-CU budget of the single fold's shape split over the segments, each row sized for the longest
        const LaunchCfg& c0 = pk.nsrc <= 2 ? kCfg2 : kCfgN;
        const uint64_t cap = std::max<uint64_t>(1, uint64_t(CuCount()) * c0.blocksPerCu / nseg);
        const uint64_t need = std::max<uint64_t>(1, (maxVec + kBlock * c0.unroll - 1) / (kBlock * c0.unroll));
        const uint32_t gr = static_cast<uint32_t>(std::min(cap, need));
        if (pk.nsrc <= 2) {
            hipLaunchKernelGGL((k_reduceN_batch_rows<E, OP, kCfg2.unroll, kCfg2.nt>), dim3(gr, nseg), dim3(kBlock), 0,
                               stream, p);
        } else {
            hipLaunchKernelGGL((k_reduceN_batch_rows<E, OP, kCfgN.unroll, kCfgN.nt>), dim3(gr, nseg), dim3(kBlock), 0,
                               stream, p);
        }
        return hipGetLastError();
    }
    // flat: one persistent grid over the concatenated tiles, sized like a single fold of the batch's bytes. U = 4 for
    // every operand count: with two operands too the tile walk wants the larger tile (5.0 / 5.6 / 6.1 TB/s at U = 1 /
    // 2 / 4 for 4 MiB segments, 5.7 / 6.3 / 6.4 at 16 MiB).
    const uint64_t tileVec = uint64_t(kBlock) * kCfgN.unroll;
    p.tileStart[0] = 0;
    for (uint32_t g = 0; g < nseg; ++g) p.tileStart[g + 1] = p.tileStart[g] + pk.nvec[g] / tileVec;
    const uint32_t gx = GridFor(totalVec, static_cast<uint32_t>(tileVec), kCfgN);
    hipLaunchKernelGGL((k_reduceN_batch<E, OP, kCfgN.unroll, kCfgN.nt>), dim3(gx), dim3(kBlock), 0, stream, p);
    return hipGetLastError();
}

using EI8 = EInt<int8_t, uint32_t>;
using EI16 = EInt<int16_t, uint32_t>;
using EI32 = EInt<int32_t, uint32_t>;
using EI64 = EInt<int64_t, uint64_t>;
using EU64 = EInt<uint64_t, uint64_t>;
using EF32 = EFp<float>;
using EF64 = EFp<double>;

// f(E{}) for dt's element rules; a dtype the reduce kernels do not have is not supported.
template <class F>
HcclResult WithElem(HcclDataType dt, F&& f)
{
    switch (dt) {
        case HCCL_DATA_TYPE_INT8: return f(EI8{});
        case HCCL_DATA_TYPE_INT16: return f(EI16{});
        case HCCL_DATA_TYPE_INT32: return f(EI32{});
        case HCCL_DATA_TYPE_INT64: return f(EI64{});
        case HCCL_DATA_TYPE_UINT64: return f(EU64{});
        case HCCL_DATA_TYPE_FP16: return f(EF16{});
        case HCCL_DATA_TYPE_BFP16: return f(EBF16{});
        case HCCL_DATA_TYPE_FP32: return f(EF32{});
        case HCCL_DATA_TYPE_FP64: return f(EF64{});
        default: return HCCL_E_NOT_SUPPORT;
    }
}

bool ValidOp(HcclReduceOp op) { return op >= HCCL_REDUCE_SUM && op <= HCCL_REDUCE_MIN; }

HcclResult Launched(hipError_t e, const char* what)
{
    if (e == hipSuccess) return HCCL_SUCCESS;
    HCCL_AMD_ERR("%s launch failed: %s", what, hipGetErrorString(e));
    return HCCL_E_RUNTIME;
}

}  // namespace

HcclResult LaunchReduce2(void* out, const void* src, const void* dst, uint64_t count, HcclDataType dt,
                         HcclReduceOp op, hipStream_t stream)
{
    if (count == 0) return HCCL_SUCCESS;
    if (!ValidOp(op)) return HCCL_E_PARA;
    return WithElem(dt, [&](auto e) {
        return WithOp(op, [&](auto o) {
            return Launched(Run2<decltype(e), decltype(o)::value>(out, src, dst, count, stream), "reduce");
        });
    });
}

HcclResult LaunchReduceN(void* out, const void* const* srcs, uint32_t n, uint64_t count, HcclDataType dt,
                         HcclReduceOp op, hipStream_t stream)
{
    if (count == 0) return HCCL_SUCCESS;
    if (!ValidOp(op) || n == 0 || n > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    if (n == 1) {
        if (out == srcs[0]) return HCCL_SUCCESS;
        uint32_t es = DataTypeSize(dt);
        if (es == 0) return HCCL_E_NOT_SUPPORT;
        return LaunchCopyBytes(out, srcs[0], count * es, stream);
    }
    if (n == 2) {
        // acc = srcs[1] (op) srcs[0]
        return LaunchReduce2(out, srcs[1], srcs[0], count, dt, op, stream);
    }
    return WithElem(dt, [&](auto e) {
        return WithOp(op, [&](auto o) {
            return Launched(RunN<decltype(e), decltype(o)::value>(out, srcs, n, count, stream), "reduceN");
        });
    });
}

HcclResult LaunchReduceNBatch(const FoldSeg* segs, uint32_t nseg, uint32_t nsrc, HcclDataType dt, HcclReduceOp op,
                              hipStream_t stream)
{
    if (!ValidOp(op) || nsrc < 2 || nsrc > HCCL_AMD_IR_MAX_SRC || nseg > kMaxBatchSegs) return HCCL_E_PARA;
    const uint32_t es = DataTypeSize(dt);
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    BatchPack pk{};
    pk.nsrc = int(nsrc);
    uint32_t nb = 0;
    uint64_t maxVec = 0;
    for (uint32_t g = 0; g < nseg; ++g) {
        const FoldSeg& f = segs[g];
        if (f.count == 0) continue;
        const void* ptrs[HCCL_AMD_IR_MAX_SRC + 1];
        ptrs[0] = f.out;
        for (uint32_t j = 0; j < nsrc; ++j) ptrs[j + 1] = f.srcs[j];
        Edges edges{};
        uint64_t nvec = 0;
        // a segment whose pointers do not share a 16-B phase runs on its own (scalar kernel)
        if (!SplitAligned(ptrs, int(nsrc) + 1, f.count, es, &edges, &nvec)) {
            HCCL_CHK(LaunchReduceN(f.out, f.srcs, nsrc, f.count, dt, op, stream));
            continue;
        }
        pk.out[nb] = f.out;
        for (uint32_t j = 0; j < nsrc; ++j) pk.srcs[nb].p[j] = f.srcs[j];
        pk.nvec[nb] = nvec;
        pk.edges[nb] = edges;
        maxVec = std::max(maxVec, nvec);
        ++nb;
    }
    if (nb == 0) return HCCL_SUCCESS;
    return WithElem(dt, [&](auto e) {
        return WithOp(op, [&](auto o) {
            return Launched(RunBatch<decltype(e), decltype(o)::value>(pk, nb, maxVec, stream), "batched reduce");
        });
    });
}


// ------------------------------------------------------------------------------------------------ device copies

namespace {

// dst[0, bytes) = src[0, bytes) in units of W bytes (W = the widest of 16, 8, 4, 2, 1 in which dst and src share their
// alignment phase: every schedule's copy is at least element-aligned, and 16 B whenever its offsets are): kCopyU units
// per lane in flight (loads first, then stores; non-temporal both ways, like the reduce kernels) over a grid of tiles
// dealt round-robin; the ragged head (before dst reaches a W boundary) and tail bytes one by one. A kernel of this
// library, so the copy's stores are ordered before the next kernel of the stream by the ordinary end-of-kernel release
// like every other kernel here (root cause of the stale operands).
constexpr int kCopyU = 4;

template <int W>
struct CopyUnit;
template <>
struct CopyUnit<16> {
    using T = u32x4;
};
template <>
struct CopyUnit<8> {
    using T = uint64_t;
};
template <>
struct CopyUnit<4> {
    using T = uint32_t;
};
template <>
struct CopyUnit<2> {
    using T = uint16_t;
};
template <>
struct CopyUnit<1> {
    using T = unsigned char;
};

template <int W>
__device__ __forceinline__ typename CopyUnit<W>::T CopyLd(const typename CopyUnit<W>::T* p)
{
    if constexpr (W == 16) {
        return ld<3>(p);
    } else {
        return __builtin_nontemporal_load(p);
    }
}

template <int W>
__device__ __forceinline__ void CopySt(typename CopyUnit<W>::T* p, typename CopyUnit<W>::T v)
{
    if constexpr (W == 16) {
        st<3>(p, v);
    } else {
        __builtin_nontemporal_store(v, p);
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_copy_units(unsigned char* dst, const unsigned char* src, uint64_t head,
                                                    uint64_t nunits, uint64_t bytes)
{
    using T = typename CopyUnit<W>::T;
    const T* s = reinterpret_cast<const T*>(src + head);
    T* d = reinterpret_cast<T*>(dst + head);
    constexpr uint64_t kTile = uint64_t(256) * kCopyU;
    const uint64_t fullTiles = nunits / kTile;
    for (uint64_t t = blockIdx.x; t < fullTiles; t += gridDim.x) {
        const uint64_t base = t * kTile + threadIdx.x;
        T x[kCopyU];
#pragma unroll
        for (int u = 0; u < kCopyU; ++u) x[u] = CopyLd<W>(s + base + u * 256);
#pragma unroll
        for (int u = 0; u < kCopyU; ++u) CopySt<W>(d + base + u * 256, x[u]);
    }
    const uint64_t tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = fullTiles * kTile + tid; i < nunits; i += stride) d[i] = s[i];
    for (uint64_t i = tid; i < head; i += stride) dst[i] = src[i];
    for (uint64_t i = head + nunits * W + tid; i < bytes; i += stride) dst[i] = src[i];
}

template <int W>
hipError_t RunCopy(unsigned char* dst, const unsigned char* src, uint64_t bytes, hipStream_t stream)
{
    const uint64_t mis = (W - (reinterpret_cast<uintptr_t>(dst) & (W - 1))) & (W - 1);
    const uint64_t head = std::min<uint64_t>(bytes, mis);
    const uint64_t nunits = (bytes - head) / W;
    // One tile per workgroup up to 16 tiles per CU (latency-bound sizes: 16 MiB ran 8.96 us on a 2-per-CU persistent
    // grid against hipMemcpyAsync's 7.88, profiles/r04_copy_kernel.jsonl); beyond that a persistent grid of two
    // workgroups per CU, the reduce kernels' measured best (1 GiB: 356-410 us against hipMemcpyAsync's 417-455).
    const uint64_t tiles = std::max<uint64_t>(1, (std::max<uint64_t>(nunits, 1) + 256 * kCopyU - 1) / (256 * kCopyU));
    const uint64_t cus = uint64_t(CuCount());
    const uint64_t blocks = tiles <= cus * 16 ? tiles : cus * 2;
    hipLaunchKernelGGL((k_copy_units<W>), dim3(uint32_t(blocks)), dim3(256), 0, stream, dst, src, head, nunits, bytes);
    return hipGetLastError();
}

}  // namespace

HcclResult LaunchCopyBytes(void* dst, const void* src, uint64_t bytes, hipStream_t stream)
{
    if (bytes == 0 || dst == src) return HCCL_SUCCESS;
    auto* d = static_cast<unsigned char*>(dst);
    const auto* sp = static_cast<const unsigned char*>(src);
    const uintptr_t x = reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src);  // phase difference
    hipError_t e;
    if ((x & 15u) == 0) {
        e = RunCopy<16>(d, sp, bytes, stream);
    } else if ((x & 7u) == 0) {
        e = RunCopy<8>(d, sp, bytes, stream);
    } else if ((x & 3u) == 0) {
        e = RunCopy<4>(d, sp, bytes, stream);
    } else if ((x & 1u) == 0) {
        e = RunCopy<2>(d, sp, bytes, stream);
    } else {
        e = RunCopy<1>(d, sp, bytes, stream);
    }
    return Launched(e, "copy");
}

}  // namespace hccl_amd
