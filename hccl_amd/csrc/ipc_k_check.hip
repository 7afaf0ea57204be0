// ipc_k_check.hip — the cross-rank argument check ahead of a collective (HCCL_DFS_CONFIG=inconsistent_check), the
// reference's CompareOpExchangeInfos (src/common/inconsistent_check.cc:52-206) as a stream-ordered kernel: the host
// never blocks.
//
// Typeless, one instantiation. Launch shape as the barrier's (ipc_k_barrier.hip): one workgroup of one wave per rank,
// blockIdx.y the rank in a loopback world. Lane t < n, t != me:
//   1. stores this rank's record into slot [parity][me] of peer t's check area, each 32-bit word w as one 8-byte atomic
//      store {word, sequence number} (the LL form's idea, ipc_kernel_body.h LlOneShot): a word's data is visible
//      exactly when its sequence number is, so the reader needs no fence and no second flag, and never compares a torn
//      or a stale record;
//   2. polls slot [parity][t] of its own area until every word carries this check's sequence number, bounded by
//      timeoutTicks;
//   3. compares the words with its own record's, in ascending order: the first differing word names the field.
// The lanes that found a difference agree on the lowest peer through one LDS word; that lane writes the report.
//
// Sequence number and parities. The sequence number s lives on the device, in the check's private word kCheckSeq:
// launch s reads s - 1 there, uses parity s & 1 and leaves s, so a captured launch replays with fresh numbers (the
// p2p kernel's rule for its counters). Every rank of a communicator launches the same checks, so the ranks' numbers
// agree. A rank can be one check ahead of a peer that is still reading, and never two: rank i stores check s + 2
// into peer p's slots only from its launch s + 2, which its stream starts after its launch s + 1 has ended, that is
// after it has received p's record of s + 1, which p stored from a launch that began after p's launch s had ended and
// read all it needed. So while p still reads parity s & 1, a peer writes at most parity (s + 1) & 1: two parities are
// needed and suffice. A stale word of the polled parity carries s - 2 or older, equal to s only after 2^32 checks; the
// area starts zeroed, and the first check is number 1.
//
// Outcomes. A difference sets bits 0 and 1 of status word 0 (bit 0 is the sticky bit every one-sided kernel tests at
// entry, so the launches queued behind return at once), stores 2 into the pinned failure word (Comm::PollAsyncError
// makes it HCCL_E_PARA) and writes the report. A wait past the bound is the existing time-out outcome: sticky bit,
// failure word 1. The poll does not leave early when the sticky bit appears meanwhile, as PollFlag does: in a loopback
// world the bit is shared, and a rank that stopped polling because a faster rank had already found the difference
// would have no report of its own. It needs none of that: a rank that has set the bit has received every rank's
// record, so every rank's stores are on their way and each poll ends.
// The kernel touches neither the collectives' epoch counter nor their flag words, so it can stand between any two
// launches: model-checked among the other kinds by tests/test_ipc_protocol_check.py.
//
// Memory ordering: everything handed over is the 8-byte words themselves (relaxed system-scope atomics on uncached
// memory). The report and the private words are read by the host after a synchronisation.
#include "ipc_kernel_body.h"

namespace hccl_amd {

namespace {

constexpr uint32_t kCheckThreads = 64;  // one wave: kIpcMaxRanks lanes hold a peer each
static_assert(kIpcMaxRanks <= int(kCheckThreads), "one lane per peer");
static_assert(kCheckWords <= 32, "the pending words of a lane are one bit mask");

__device__ __forceinline__ uint64_t* CheckSlot(uint64_t* area, uint32_t parity, uint32_t src)
{
    return area + (uint64_t(parity) * kIpcMaxRanks + src) * kCheckWords;
}

__global__ __launch_bounds__(kCheckThreads) void k_ipc_check(IpcCheckArgs a)
{
    const uint32_t me = a.me >= 0 ? static_cast<uint32_t>(a.me) : blockIdx.y;
    const uint32_t t = threadIdx.x;
    uint64_t* priv = a.priv[me];
    const uint32_t sticky = __hip_atomic_load(a.sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t seq =
        static_cast<uint32_t>(__hip_atomic_load(priv + kCheckSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) + 1u;
    if ((sticky & 1u) != 0) return;  // a failed communicator: never wait on its peers again
    const uint32_t parity = seq & 1u;
    __shared__ uint32_t lowest;  // the lowest peer whose record differs
    if (t == 0) lowest = ~0u;
    __syncthreads();
    const CheckRecord& mine = a.rec[me];
    uint32_t got[kCheckWords] = {};
    uint32_t diff = kCheckWords;  // the first differing word
    if (t < a.n && t != me) {
        const auto dst = AsGlobal(CheckSlot(a.area[t], parity, me));
#pragma unroll
        for (uint32_t w = 0; w < kCheckWords; ++w) {
            __hip_atomic_store(dst + w, uint64_t(mine.w[w]) | (uint64_t(seq) << 32), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
        const uint64_t* src = CheckSlot(a.area[me], parity, t);
        uint32_t pending = (1u << kCheckWords) - 1u, polls = 0;
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            uint64_t v[kCheckWords];
#pragma unroll
            for (uint32_t w = 0; w < kCheckWords; ++w) {
                if (pending & (1u << w)) v[w] = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
#pragma unroll
            for (uint32_t w = 0; w < kCheckWords; ++w) {
                if ((pending & (1u << w)) && static_cast<uint32_t>(v[w] >> 32) == seq) {
                    got[w] = static_cast<uint32_t>(v[w]);
                    pending &= ~(1u << w);
                }
            }
            if (pending == 0) break;
            if ((++polls & 63u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > a.timeoutTicks) {
                __hip_atomic_fetch_or(a.sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_fetch_or(a.status[me], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(a.failHost, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (pending == 0) {
#pragma unroll
            for (uint32_t w = kCheckWords; w-- > 0;) {
                if (got[w] != mine.w[w]) diff = w;
            }
            if (diff != kCheckWords) atomicMin(&lowest, t);
        }
    }
    __syncthreads();
    if (diff != kCheckWords && lowest == t) {
        const uint32_t f = CheckFieldOfWord(diff), w0 = CheckFirstWord(f);
        const bool wide = CheckWideField(f);
        uint64_t local = 0, remote = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCheckWords; ++w) {  // constant indices: the words stay in registers
            if (w == w0 || (wide && w == w0 + 1)) {
                local |= uint64_t(mine.w[w]) << (w == w0 ? 0 : 32);
                remote |= uint64_t(got[w]) << (w == w0 ? 0 : 32);
            }
        }
        priv[kCheckPeer] = t;
        priv[kCheckField] = f;
        priv[kCheckLocal] = local;
        priv[kCheckRemote] = remote;
        priv[kCheckHasReport] = 1;
        __hip_atomic_fetch_or(a.sticky, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_fetch_or(a.status[me], 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // after the time-out's 1 of any lane of this wave: the report is what the host should see
        __hip_atomic_store(a.failHost, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (t == 0) __hip_atomic_store(priv + kCheckSeq, uint64_t(seq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t LaunchIpcCheck(const IpcCheckArgs& a, uint32_t worldRanks, hipStream_t s)
{
    hipLaunchKernelGGL(k_ipc_check, dim3(1, worldRanks == 0 ? 1 : worldRanks), dim3(kCheckThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace hccl_amd
