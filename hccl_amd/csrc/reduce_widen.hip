// reduce_widen.hip — the widening FP8 sum: out = narrow(f32(srcs[0]) + ... ) for CDNA4 (gfx950).
//
// Replaces the input-type / output-type form of the reference's n-ary local reduce (ccu::LocalReduce(bufs, size,
// dataType, outputDataType, op, ...), ccu_kernel_alg_base.cc:1153-1200; GetReduceExpansionNum,
// ccu_kernel_utils.cc:107-123: a low-precision SUM may name fp32 / bf16 / fp16 as its output, default fp32).
// Inputs are OCP FP8 (E4M3 = e4m3fn, E5M2), the result FP32, BF16 or FP16, never FP8. The fold is
//   acc = f32(srcs[0]); acc = f32(srcs[j]) + acc (j = 1 .. nsrc-1); out = narrow(acc)
// with the exact hardware decode (v_cvt_pk_f32_fp8 / v_cvt_pk_f32_bf8, two elements per instruction), plain FP32 adds
// in operand order and one round-to-nearest-even narrowing. No fast-math, denormals kept.
//
// A 1-byte stream is read nsrc times and a 4- or 2-byte stream is written once, so the load and store geometry of the
// same-type kernels (16-B vectors both ways, reduce_kernels.hip) cannot coincide. The work is split by OUTPUT vector:
//   * a lane's unit is one 16-B output vector: 4 elements (FP32) or 8 (BF16 / FP16), so its load per operand is 4 or
//     8 bytes (global_load_dword / dwordx2);
//   * consecutive lanes own consecutive output vectors: every store instruction of a wave writes 1 KiB of whole lines
//     and every load instruction reads 256 or 512 contiguous bytes;
//   * a tile is U output vectors per lane; the U loads of operand j are issued before any is decoded, and operand j+1 is
//     loaded once operand j is folded (the FoldTile order); the accumulators are U x 4 or U x 8 FP32 VGPRs;
//   * the grid is persistent, tiles dealt round-robin; loads and stores are non-temporal; no LDS (nothing is reused).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "reduce_elem.h"
#include "widen_elem.h"

namespace hccl_amd {

namespace {

constexpr int kBlock = 256;

struct WidenSrcs {
    const unsigned char* p[HCCL_AMD_IR_MAX_SRC];
};

// Scalar elements around the vector body, as reduce_kernels.hip's Edges: done by one workgroup.
struct WidenEdges {
    uint32_t head;  // elements before out reaches a 16-B boundary
    uint32_t tail;  // elements after the last whole output vector
    uint64_t tailStart;
};

// Operand j's loads of the vector body (from the first element at which out is 16-B aligned).
template <class L>
__device__ __forceinline__ const L* VecSrc(const WidenSrcs& srcs, int j, const WidenEdges& edges)
{
    return reinterpret_cast<const L*>(srcs.p[j] + edges.head);
}

// The fold of one output vector's elements, loaded one operand after the other.
template <class D, class O>
__device__ __forceinline__ u32x4 FoldVector(const WidenSrcs& srcs, int nsrc, const WidenEdges& edges, uint64_t i)
{
    using L = typename O::L;
    float acc[O::kPer];
    Decode<D>(__builtin_nontemporal_load(VecSrc<L>(srcs, 0, edges) + i), acc);
    for (int j = 1; j < nsrc; ++j) {
        float x[O::kPer];
        Decode<D>(__builtin_nontemporal_load(VecSrc<L>(srcs, j, edges) + i), x);
#pragma unroll
        for (int e = 0; e < O::kPer; ++e) acc[e] = x[e] + acc[e];
    }
    return O::pack(acc);
}

template <class D, class O>
__device__ __forceinline__ typename O::S FoldElement(const WidenSrcs& srcs, int nsrc, uint64_t i)
{
    float acc = D::one(srcs.p[0][i]);
    for (int j = 1; j < nsrc; ++j) acc = D::one(srcs.p[j][i]) + acc;
    return O::narrow(acc);
}

// ------------------------------------------------------------------------------------------------ kernels

template <class D, class O, int U>
__global__ __launch_bounds__(kBlock) void k_reduce_widen(typename O::S* out, WidenSrcs srcs, int nsrc, uint64_t nvec,
                                                           WidenEdges edges)
{
    using L = typename O::L;
    constexpr int K = O::kPer;
    constexpr uint64_t kTile = uint64_t(kBlock) * U;
    u32x4* vout = reinterpret_cast<u32x4*>(out + edges.head);
    const uint64_t fullTiles = nvec / kTile;
    for (uint64_t t = blockIdx.x; t < fullTiles; t += gridDim.x) {
        const uint64_t base = t * kTile + threadIdx.x;
        float acc[U][K];
        L v[U];
        const L* p0 = VecSrc<L>(srcs, 0, edges);
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(p0 + base + u * kBlock);
#pragma unroll
        for (int u = 0; u < U; ++u) Decode<D>(v[u], acc[u]);
        for (int j = 1; j < nsrc; ++j) {
            const L* pj = VecSrc<L>(srcs, j, edges);
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(pj + base + u * kBlock);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float x[K];
                Decode<D>(v[u], x);
#pragma unroll
                for (int e = 0; e < K; ++e) acc[u][e] = x[e] + acc[u][e];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) st<3>(vout + base + u * kBlock, O::pack(acc[u]));
    }
    // the vectors after the last full tile, one per lane, strided over the grid
    for (uint64_t i = fullTiles * kTile + uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < nvec;
         i += uint64_t(gridDim.x) * kBlock) {
        st<3>(vout + i, FoldVector<D, O>(srcs, nsrc, edges, i));
    }
    // the scalar head and tail by one workgroup: lanes 0.. take the head's elements, lanes 64.. (another wave) the tail's
    if (blockIdx.x == 0) {
        const uint32_t tid = threadIdx.x;
        const bool head = tid < edges.head;
        if (head || (tid >= 64 && tid - 64 < edges.tail)) {
            const uint64_t i = head ? tid : edges.tailStart + (tid - 64);
            out[i] = FoldElement<D, O>(srcs, nsrc, i);
        }
    }
}

// When the operands' phases do not line up with the output's vectors: one element per lane, byte loads, grid-stride.
template <class D, class O>
__global__ __launch_bounds__(kBlock) void k_reduce_widen_scalar(typename O::S* out, WidenSrcs srcs, int nsrc,
                                                                  uint64_t count)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += uint64_t(gridDim.x) * kBlock) {
        out[i] = FoldElement<D, O>(srcs, nsrc, i);
    }
}

// ------------------------------------------------------------------------------------------------ host launch

constexpr uint32_t kBlocksPerCu = 2;  // the persistent grid of the same-type folds (kCfgN)

uint32_t GridFor(uint64_t work, uint64_t perBlock)
{
    const uint64_t need = (work + perBlock - 1) / perBlock;
    const uint64_t cap = uint64_t(CuCount()) * kBlocksPerCu;
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min(need, cap)));
}

// SplitAligned (reduce_kernels.hip) for streams of different element sizes: [0, count) as head / body of 16-B output
// vectors / tail. The body starts at the first element h at which `out` (outSize-byte elements) is 16-B aligned, and
// needs every operand's address at element h aligned to its load of `per` bytes (per 1-byte elements = one output
// vector). False when a body exists and the phases do not line up.
bool SplitWiden(const void* out, const WidenSrcs& srcs, uint32_t n, uint64_t count, uint32_t outSize, uint32_t per,
                WidenEdges* e, uint64_t* nvec)
{
    const uintptr_t phase = reinterpret_cast<uintptr_t>(out) & 15u;
    if (phase % outSize != 0) return false;
    const uint64_t head = std::min<uint64_t>(count, phase == 0 ? 0 : (16 - phase) / outSize);
    *nvec = (count - head) / per;
    e->head = static_cast<uint32_t>(head);
    e->tailStart = head + *nvec * per;
    e->tail = static_cast<uint32_t>(count - e->tailStart);
    if (*nvec == 0) return true;  // the edges alone: nothing is loaded as a vector
    for (uint32_t j = 0; j < n; ++j) {
        if ((reinterpret_cast<uintptr_t>(srcs.p[j]) + head) % per != 0) return false;
    }
    return true;
}

template <class D, class O>
hipError_t RunWiden(void* out, const WidenSrcs& srcs, uint32_t n, uint64_t count, hipStream_t stream)
{
    using S = typename O::S;
    WidenEdges edges{};
    uint64_t nvec = 0;
    if (!SplitWiden(out, srcs, n, count, sizeof(S), O::kPer, &edges, &nvec)) {
        hipLaunchKernelGGL((k_reduce_widen_scalar<D, O>), dim3(GridFor(count, kBlock * 4)), dim3(kBlock), 0, stream,
                           static_cast<S*>(out), srcs, int(n), count);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_reduce_widen<D, O, O::kU>), dim3(GridFor(nvec, uint64_t(kBlock) * O::kU)), dim3(kBlock), 0,
                       stream, static_cast<S*>(out), srcs, int(n), nvec, edges);
    return hipGetLastError();
}

template <class D>
HcclResult RunWidenTo(HcclDataType outType, void* out, const WidenSrcs& srcs, uint32_t n, uint64_t count,
                      hipStream_t stream, hipError_t* e)
{
    switch (outType) {
        case HCCL_DATA_TYPE_FP32: *e = RunWiden<D, OF32>(out, srcs, n, count, stream); return HCCL_SUCCESS;
        case HCCL_DATA_TYPE_BFP16: *e = RunWiden<D, OBF16>(out, srcs, n, count, stream); return HCCL_SUCCESS;
        case HCCL_DATA_TYPE_FP16: *e = RunWiden<D, OF16>(out, srcs, n, count, stream); return HCCL_SUCCESS;
        default: return HCCL_E_NOT_SUPPORT;
    }
}

}  // namespace

bool IsWidenPair(HcclDataType inType, HcclDataType outType)
{
    const bool in = inType == HCCL_DATA_TYPE_FP8E4M3 || inType == HCCL_DATA_TYPE_FP8E5M2;
    const bool out = outType == HCCL_DATA_TYPE_FP32 || outType == HCCL_DATA_TYPE_BFP16 || outType == HCCL_DATA_TYPE_FP16;
    return in && out;
}

HcclResult LaunchReduceNWiden(void* out, const void* const* srcs, uint32_t n, uint64_t count, HcclDataType inType,
                              HcclDataType outType, hipStream_t stream)
{
    if (count == 0) return HCCL_SUCCESS;
    if (n == 0 || n > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    if (!IsWidenPair(inType, outType)) return HCCL_E_NOT_SUPPORT;
    WidenSrcs pk{};
    for (uint32_t j = 0; j < n; ++j) pk.p[j] = static_cast<const unsigned char*>(srcs[j]);
    hipError_t e = hipSuccess;
    HCCL_CHK(inType == HCCL_DATA_TYPE_FP8E4M3 ? RunWidenTo<DE4M3>(outType, out, pk, n, count, stream, &e)
                                              : RunWidenTo<DE5M2>(outType, out, pk, n, count, stream, &e));
    if (e == hipSuccess) return HCCL_SUCCESS;
    HCCL_AMD_ERR("widening reduce launch failed: %s", hipGetErrorString(e));
    return HCCL_E_RUNTIME;
}

}  // namespace hccl_amd
