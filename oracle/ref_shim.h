/*
 * ref_shim.h — the names the reference's six arithmetic functions need, and nothing else. TEST INFRASTRUCTURE ONLY.
 *
 * oracle/Makefile cuts Fp16ToFp32, Fp32DenormToFp16, Fp32ToFp16, AicpuReduceFp16, AicpuReduce and
 * AicpuReduceTemplate<T> out of the reference's alg_data_trans_wrapper.cc at build time (into oracle/_ref/, never
 * committed) and compiles that block behind this header. The rest of that file needs the external hcomm headers; the
 * six functions only need what is below. Everything here is this project's own text: stand-ins with the obvious
 * meaning and enum values copied as data from include/hccl_types.h (tests/test_abi.py pins those values).
 */
#ifndef HCCL_AMD_ORACLE_REF_SHIM_H_
#define HCCL_AMD_ORACLE_REF_SHIM_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

typedef uint8_t u8;
typedef uint64_t u64;

/* Unscoped, so that both `HcclResult::HCCL_SUCCESS` and a bare `HCCL_E_INTERNAL` name the same value. */
enum HcclResult { HCCL_SUCCESS = 0, HCCL_E_INTERNAL = 4 };
enum HcclDataType {
    HCCL_DATA_TYPE_INT8 = 0,
    HCCL_DATA_TYPE_INT16 = 1,
    HCCL_DATA_TYPE_INT32 = 2,
    HCCL_DATA_TYPE_FP16 = 3,
    HCCL_DATA_TYPE_FP32 = 4,
    HCCL_DATA_TYPE_INT64 = 5,
    HCCL_DATA_TYPE_UINT64 = 6,
    HCCL_DATA_TYPE_FP64 = 10,
    HCCL_DATA_TYPE_BFP16 = 11,
    HCCL_DATA_TYPE_RESERVED = 255
};
enum HcclReduceOp {
    HCCL_REDUCE_SUM = 0,
    HCCL_REDUCE_PROD = 1,
    HCCL_REDUCE_MAX = 2,
    HCCL_REDUCE_MIN = 3,
    HCCL_REDUCE_RESERVED = 4
};

#define EOK 0
static inline int memcpy_s(void* dst, size_t dstMax, const void* src, size_t n)
{
    if (dst == nullptr || src == nullptr || n > dstMax) {
        return 1;
    }
    memcpy(dst, src, n);
    return EOK;
}

/* Logging is dropped; CHK_PRT_RET keeps its control flow: on `cond`, (log and) return `ret`. */
#define HCCL_ERROR(...) ((void)0)
#define CHK_PRT_RET(cond, print, ret) \
    do {                              \
        if (cond) {                   \
            print;                    \
            return ret;               \
        }                             \
    } while (0)

namespace ops_hccl {

typedef void* ThreadHandle;

struct DataSlice {
    void* addr_;
    u64 size_; /* bytes */
};

static inline void* GetSliceAddr(const DataSlice& s) { return s.addr_; }

template <typename... A>
static inline void TraceDataSlice(A&&...)
{
}

/* The reference's header declares these ahead of their use; the block defines the template last. */
float Fp16ToFp32(uint16_t fp16Bits);
uint16_t Fp32DenormToFp16(uint32_t sign, uint32_t mantissa, int32_t fp16Exp);
uint16_t Fp32ToFp16(float value);
template <typename T>
HcclResult AicpuReduceTemplate(T* dst, u64 dstSize, T* src, u64 srcSize, const HcclReduceOp reduceOp);
HcclResult AicpuReduceFp16(u8* dst, u8* src, u64 size, const HcclReduceOp reduceOp);
HcclResult AicpuReduce(const ThreadHandle& thread, const DataSlice& srcSlice, const DataSlice& dstSlice,
                       const HcclDataType dataType, const HcclReduceOp reduceOp);

} // namespace ops_hccl

#endif /* HCCL_AMD_ORACLE_REF_SHIM_H_ */
