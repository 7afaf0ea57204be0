// widen_elem.h — the element rules of the widening FP8 sum, shared by the local kernel (reduce_widen.hip) and the
// one-sided kernel (ipc_k_widen.hip): the exact hardware decode of OCP FP8 (E4M3 = e4m3fn, E5M2) to FP32, two elements
// per v_cvt_pk_f32_fp8 / v_cvt_pk_f32_bf8, and the one round-to-nearest-even narrowing to the output type.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.h"
#include "reduce_elem.h"

namespace hccl_amd {

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// Input formats: two elements of a dword's low (HI = false) or high half, and one byte.
struct DE4M3 {
    template <bool HI>
    static __device__ __forceinline__ f32x2 pk(uint32_t w)
    {
        return __builtin_amdgcn_cvt_pk_f32_fp8(w, HI);
    }
    static __device__ __forceinline__ float one(unsigned char b) { return __builtin_amdgcn_cvt_f32_fp8(uint32_t(b), 0); }
};

struct DE5M2 {
    template <bool HI>
    static __device__ __forceinline__ f32x2 pk(uint32_t w)
    {
        return __builtin_amdgcn_cvt_pk_f32_bf8(w, HI);
    }
    static __device__ __forceinline__ float one(unsigned char b) { return __builtin_amdgcn_cvt_f32_bf8(uint32_t(b), 0); }
};

// Output formats: S the stored element, kPer elements per 16-B vector, L the local kernel's load per operand (kPer
// bytes), kU its output vectors per lane per tile.
//
// U: the n-ary fold keeps 2 workgroups x 256 lanes x 4 x 16 B = 32 KiB of loads in flight per CU (kCfgN). A lane's load
// here is 4 or 8 bytes, so the same bytes in flight would take U = 16 (FP32 output) and U = 8 (16-bit output). The
// sweep on MI355X (profiles/widen_fold_u_sweep.jsonl, taken with tools/probes/widen_fold_bench.py on one library per
// candidate, candidates alternated over three passes; E4M3, 256 Mi elements per operand, us at nsrc = 2 / 8, every
// pass's median within +-1 us of the figure) chose half of that:
//   FP32 output   U = 4: 286 / 760   U = 8: 277 / 546   U = 16: 284 / 596   U = 32: 296 / 571
//   BF16 output   U = 4: 177 / 458   U = 8: 176 / 463   U = 16: 187 / 461
struct OF32 {
    using S = float;
    using L = uint32_t;
    static constexpr int kPer = 4;
    static constexpr int kU = 8;
    static __device__ __forceinline__ float narrow(float f) { return f; }
    static __device__ __forceinline__ u32x4 pack(const float (&a)[4])
    {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = __builtin_bit_cast(uint32_t, a[i]);
        return r;
    }
};

// One round to nearest even, two elements per v_cvt_pk_bf16_f32 (EBF16::narrow's conversion).
struct OBF16 {
    using S = uint16_t;
    using L = u32x2;
    static constexpr int kPer = 8;
    static constexpr int kU = 4;
    static __device__ __forceinline__ uint16_t narrow(float f) { return EBF16::narrow(f); }
    static __device__ __forceinline__ u32x4 pack(const float (&a)[8])
    {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 v = {a[2 * i], a[2 * i + 1]};
            r[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
        }
        return r;
    }
};

struct OF16 {
    using S = uint16_t;
    using L = u32x2;
    static constexpr int kPer = 8;
    static constexpr int kU = 4;
    static __device__ __forceinline__ uint16_t narrow(float f)
    {
        return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
    }
    static __device__ __forceinline__ u32x4 pack(const float (&a)[8])
    {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 v = {a[2 * i], a[2 * i + 1]};
            r[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
        }
        return r;
    }
};

// The 4 or 8 elements of one load, in memory order.
template <class D>
__device__ __forceinline__ void Decode(uint32_t w, float (&a)[4])
{
    const f32x2 lo = D::template pk<false>(w), hi = D::template pk<true>(w);
    a[0] = lo[0];
    a[1] = lo[1];
    a[2] = hi[0];
    a[3] = hi[1];
}

template <class D>
__device__ __forceinline__ void Decode(u32x2 w, float (&a)[8])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const f32x2 lo = D::template pk<false>(w[k]), hi = D::template pk<true>(w[k]);
        a[4 * k + 0] = lo[0];
        a[4 * k + 1] = lo[1];
        a[4 * k + 2] = hi[0];
        a[4 * k + 3] = hi[1];
    }
}

// The host's view of a type pair (IsWidenPair holds): f(D{}, O{}).
template <class F>
auto WithWidenPair(HcclDataType inType, HcclDataType outType, F&& f)
{
    auto out = [&](auto d) {
        switch (outType) {
            case HCCL_DATA_TYPE_FP32: return f(d, OF32{});
            case HCCL_DATA_TYPE_BFP16: return f(d, OBF16{});
            default: return f(d, OF16{});
        }
    };
    return inType == HCCL_DATA_TYPE_FP8E4M3 ? out(DE4M3{}) : out(DE5M2{});
}

}  // namespace

}  // namespace hccl_amd
