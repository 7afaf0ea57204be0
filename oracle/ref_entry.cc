/*
 * ref_entry.cc — C entries into the reference's own arithmetic, compiled from the block that oracle/Makefile extracts
 * into oracle/_ref/ref_block.inc. TEST INFRASTRUCTURE ONLY; the product library never links or loads this.
 *
 * Every entry takes and returns bit patterns in caller-owned arrays, so no float crosses the ctypes boundary (a C
 * float passed by value goes through a double there, which quiets a signalling NaN).
 */
#include "ref_shim.h"

namespace ops_hccl {
#include "_ref/ref_block.inc" /* the six functions; the extracted text stops before the namespace's closing brace */
} // namespace ops_hccl

extern "C" {

/* dst = src (op) dst over `bytes` bytes of both, through the reference's AicpuReduce. Returns its HcclResult. */
int ref_reduce(int dtype, int op, void* dst, const void* src, uint64_t bytes)
{
    ops_hccl::ThreadHandle thread = nullptr;
    ops_hccl::DataSlice s = {const_cast<void*>(src), bytes};
    ops_hccl::DataSlice d = {dst, bytes};
    return static_cast<int>(
        ops_hccl::AicpuReduce(thread, s, d, static_cast<HcclDataType>(dtype), static_cast<HcclReduceOp>(op)));
}

void ref_fp16_to_fp32_bits(const uint16_t* in, uint32_t* out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        float f = ops_hccl::Fp16ToFp32(in[i]);
        memcpy(&out[i], &f, sizeof f);
    }
}

void ref_fp32_to_fp16_bits(const uint32_t* in, uint16_t* out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        float f;
        memcpy(&f, &in[i], sizeof f);
        out[i] = ops_hccl::Fp32ToFp16(f);
    }
}

} // extern "C"
