// ipc.cc — host side of the one-sided collectives (ipc_kernel_body.h): peer-mapped staging set-up and launch.
//
// Set-up (collective, on the first IPC call of a communicator): every rank allocates uncached staging and a
// flag array, exports them with hipIpcGetMemHandle, all-gathers the handles over the communicator (ncclAllGather)
// and opens every peer's with hipIpcOpenMemHandle — the reference's channel set-up that hands each rank its peers'
// CCL buffers (ChannelInfo.remoteCclMem, alg_param.h:434-448; AIV GM_IN[r], aiv_communication_base_v2.h:121-150).
// In a loopback world the ranks share a device and the raw pointers are exchanged instead, and the whole world runs
// as one launch (all ranks' blocks must be resident together, which separate per-rank launches on 4 hardware queues
// would not guarantee).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "comm.h"

namespace hccl_amd {

namespace {

// The uncached allocations of the IPC path (the staging tiers; flags and LL area) are kept for the life of the process
// and handed to the next communicator's set-up that asks for the same size on the same device; they are never freed.
// Freeing hipDeviceMallocUncached memory corrupts later GPU work on this stack: the r03 test order's allocation history
// in a loop returned wrong results (ranks' operands missing) in 17 of 217 iterations with these blocks freed after
// every destroy and in 0 of 223 with them kept, and a loop that freed uncached blocks allocated outside the library
// faulted the GPU (memory aperture violation) where the same loop with cached blocks ran clean
// (profiles/r06_release_stress.txt).
struct UncachedPool {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void*> idle;  // (device, bytes) -> allocation
};

UncachedPool& Pool()
{
    static UncachedPool* p = new UncachedPool;  // never destroyed: the runtime frees device memory at exit
    return *p;
}

bool UncachedAlloc(int device, void** ptr, size_t bytes)
{
    {
        UncachedPool& pool = Pool();
        std::lock_guard<std::mutex> lk(pool.mu);
        auto it = pool.idle.find({device, bytes});
        if (it != pool.idle.end()) {
            *ptr = it->second;
            pool.idle.erase(it);
            return true;
        }
    }
    return hipExtMallocWithFlags(ptr, bytes, hipDeviceMallocUncached) == hipSuccess;
}

void UncachedRelease(int device, void* ptr, size_t bytes)
{
    UncachedPool& pool = Pool();
    std::lock_guard<std::mutex> lk(pool.mu);
    pool.idle.insert({{device, bytes}, ptr});
}

}  // namespace

uint64_t IpcIdleBytes()
{
    UncachedPool& pool = Pool();
    std::lock_guard<std::mutex> lk(pool.mu);
    uint64_t b = 0;
    for (const auto& kv : pool.idle) b += kv.first.second;
    return b;
}

namespace {

size_t FlagAllocBytes() { return size_t(kIpcFlagBytes + 2 * kIpcLlParityBytes); }

// Maps one allocation of every rank (collective: every rank takes part whatever its local outcome, and the outcome
// is agreed: either every rank has every peer's allocation mapped, or none keeps a mapping and all report
// HCCL_E_NOT_SUPPORT; a failed host exchange returns the transport's error). peers[r] receives rank r's allocation
// as this rank addresses it (its own at [me]); opened[r] marks the ones opened with hipIpcOpenMemHandle. In a loopback
// world the ranks share the device and exchange raw pointers. ranksOnDevice (rank mode, optional) receives the most
// ranks any one device holds, from every rank's PCI bus id: the same number on every rank.
HcclResult MapPeers(Comm& c, void* mine, bool localOk, void* peers[kIpcMaxRanks], bool opened[kIpcMaxRanks],
                    uint32_t* ranksOnDevice)
{
    const uint32_t n = c.nRanks, me = c.rank;
    if (c.transport->SharedDevice()) {
        struct Raw {
            void* p;
            uint8_t ok;
        };
        const Raw m{mine, static_cast<uint8_t>(localOk ? 1 : 0)};
        std::vector<Raw> all(n);
        HCCL_CHK(c.transport->AllGatherHost(&m, sizeof m, all.data()));
        for (uint32_t r = 0; r < n; ++r) {
            if (all[r].ok == 0) return HCCL_E_NOT_SUPPORT;
        }
        for (uint32_t r = 0; r < n; ++r) peers[r] = all[r].p;
        return HCCL_SUCCESS;
    }
    struct Exported {
        hipIpcMemHandle_t h;
        char busId[32];  // the rank's device: ranks that share one count against its resident blocks together
        uint8_t ok;
    };
    Exported m{};
    bool ok = localOk && hipIpcGetMemHandle(&m.h, mine) == hipSuccess &&
              hipDeviceGetPCIBusId(m.busId, sizeof m.busId - 1, c.device) == hipSuccess;
    m.ok = ok ? 1 : 0;
    std::vector<Exported> all(n);
    HCCL_CHK(c.transport->AllGatherHost(&m, sizeof m, all.data()));
    for (uint32_t r = 0; r < n; ++r) ok = ok && all[r].ok != 0;  // nobody opens a handle some rank could not export
    if (ranksOnDevice != nullptr) {
        *ranksOnDevice = 1;
        for (uint32_t r = 0; r < n; ++r) {
            uint32_t k = 0;
            for (uint32_t q = 0; q < n; ++q) k += std::strncmp(all[r].busId, all[q].busId, sizeof m.busId) == 0;
            *ranksOnDevice = std::max(*ranksOnDevice, k);
        }
    }
    for (uint32_t r = 0; r < n && ok; ++r) {
        if (r == me) {
            peers[r] = mine;
            continue;
        }
        void* p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, all[r].h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            HCCL_AMD_ERR("rank %u: hipIpcOpenMemHandle of rank %u failed: %s", me, r, hipGetErrorString(e));
            ok = false;
            break;
        }
        peers[r] = p;
        opened[r] = true;
    }
    const uint8_t mineOk = ok ? 1 : 0;
    std::vector<uint8_t> allOk(n);
    const HcclResult xr = c.transport->AllGatherHost(&mineOk, 1, allOk.data());
    for (uint32_t r = 0; r < n && xr == HCCL_SUCCESS; ++r) ok = ok && allOk[r] != 0;
    if (xr == HCCL_SUCCESS && ok) return HCCL_SUCCESS;
    for (uint32_t r = 0; r < n; ++r) {
        if (opened[r]) (void)hipIpcCloseMemHandle(peers[r]);
        opened[r] = false;
        peers[r] = nullptr;
    }
    return xr != HCCL_SUCCESS ? xr : HCCL_E_NOT_SUPPORT;
}

// The four areas inside one staging allocation at base (every rank has the same layout).
void AreasOf(const IpcTier& t, void* base, void* areas[kIpcAreas])
{
    char* b = static_cast<char*>(base);
    areas[kIpcAreaIn] = b;
    areas[kIpcAreaRes] = b + t.size.inBytes;
    areas[kIpcAreaAlt0] = b + t.size.inBytes + t.size.resBytes;
    areas[kIpcAreaAlt1] = b + t.size.inBytes + t.size.resBytes + t.size.altBytes;
}

void ReleaseTier(Comm& c, IpcTier& t)
{
    for (uint32_t r = 0; r < kIpcMaxRanks; ++r) {
        if (t.opened[r]) (void)hipIpcCloseMemHandle(t.peerArea[kIpcAreaIn][r]);  // the peer's one allocation
    }
    if (t.area[0] != nullptr) UncachedRelease(c.device, t.area[0], t.size.allocBytes());
    const bool unavailable = t.unavailable;
    t = IpcTier{};
    t.unavailable = unavailable;
}

// The area sizes of staging tier t for c: a function of the rank count and the (=) configuration.
IpcTierBytes TierSizes(const Comm& c, int t)
{
    return IpcTierSizes(c.nRanks, c.cclBytes, c.cfg.ipcStagingBytes, c.cfg.smallIpcBytes, t);
}

// What every one-sided call needs (collective, at the communicator's first one-sided call): the flags and, behind
// them, the LL area (one uncached allocation mapped by every peer, zeroed), the status words, the host-visible failure
// word and the LL unpack area.
HcclResult IpcSetupBase(Comm& c)
{
    IpcState& s = c.ipc;
    if (s.ready) return HCCL_SUCCESS;
    if (s.unavailable) return HCCL_E_NOT_SUPPORT;
    s.blocks = kIpcBlocks;
    const size_t flagBytes = FlagAllocBytes();
    // The fresh uncached pages may carry lines of a freed cached buffer in some XCD's L2: scrub the L2s before the
    // flags are zeroed (ScrubL2), so that no stale line is ever read or written back over them.
    // HCCL_AMD_INJECT_IPC_ALLOC_FAIL (tests): this rank's allocations fail, as under memory pressure
    const bool inject = c.cfg.injectIpcAllocFail == static_cast<int32_t>(c.rank);
    bool ok = !inject && UncachedAlloc(c.device, reinterpret_cast<void**>(&s.flags), flagBytes) &&
              hipMalloc(reinterpret_cast<void**>(&s.status), kIpcStatusBytes) == hipSuccess &&
              hipMalloc(&s.llUnpack, kIpcLlUnpackBytes) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&s.failHost), 64, hipHostMallocCoherent | hipHostMallocMapped) ==
                  hipSuccess &&
              hipHostGetDevicePointer(reinterpret_cast<void**>(&s.failDev), s.failHost, 0) == hipSuccess &&
              hipDeviceSynchronize() == hipSuccess && (!c.cfg.ipcL2Scrub || ScrubL2(c.reduceStream) == HCCL_SUCCESS) &&
              hipMemset(s.flags, 0, flagBytes) == hipSuccess && hipMemset(s.status, 0, kIpcStatusBytes) == hipSuccess &&
              hipDeviceSynchronize() == hipSuccess;
    if (ok && c.cfg.ipcTrace) {
        // phase stamps (diagnostics, HCCL_AMD_IPC_TRACE; HcclAmdCommIpcTrace reads them back): every rank's and
        // block's row, so a loopback world's one launch fits too
        const size_t tb = size_t(kIpcMaxRanks) * kIpcMaxBlocks * kIpcTraceSlots * sizeof(uint64_t);
        ok = hipMalloc(reinterpret_cast<void**>(&s.trace), tb) == hipSuccess && hipMemset(s.trace, 0, tb) == hipSuccess &&
             hipDeviceSynchronize() == hipSuccess;
    }
    if (ok) {
        *s.failHost = 0;
    } else {
        HCCL_AMD_ERR("rank %u: IPC flag or status allocation failed", c.rank);
    }
    const volatile uint32_t* watch = s.failHost;
    uint32_t* wdev = nullptr;
    if (c.transport->SharedDevice()) {
        // The world runs one launch for all ranks (issued by rank 0): its timeouts go to the world's word, which every
        // rank watches and which outlives each rank's communicator.
        uint32_t* word = ok ? c.transport->SharedFailWord(&wdev) : nullptr;
        ok = ok && word != nullptr;
        watch = word;
    }
    void* peers[kIpcMaxRanks] = {};
    const HcclResult r = MapPeers(c, s.flags, ok, peers, s.flagsOpened, &s.ranksOnDevice);
    if (r != HCCL_SUCCESS) {
        IpcRelease(c);
        s.unavailable = true;
        return r;
    }
    for (uint32_t q = 0; q < c.nRanks; ++q) s.peerFlags[q] = static_cast<uint32_t*>(peers[q]);
    if (c.transport->SharedDevice()) s.failDev = wdev;
    c.failWord.store(watch, std::memory_order_release);
    s.ready = true;
    return HCCL_SUCCESS;
}

// Staging tier t (collective, at the first call that needs it): one uncached allocation below 2 GiB holding
// [in][results][alternate 0][alternate 1], mapped by every peer. hipIpcOpenMemHandle never returned for a 2 GiB
// allocation on this stack (r03: the 512 MiB areas in one 2 GiB block hung the rank-mode set-up;
// profiles/r03_probe_ipc_open*.jsonl: up to 2047 MiB opens in < 1 ms, 2048 MiB does not return).
HcclResult IpcSetupTier(Comm& c, int t)
{
    IpcTier& tr = c.ipc.tier[t];
    if (tr.ready) return HCCL_SUCCESS;
    if (tr.unavailable) return HCCL_E_NOT_SUPPORT;
    tr.size = TierSizes(c, t);
    void* base = nullptr;
    bool ok = c.cfg.injectIpcAllocFail != static_cast<int32_t>(c.rank) && UncachedAlloc(c.device, &base, tr.size.allocBytes());
    if (!ok) {
        base = nullptr;
        HCCL_AMD_ERR("rank %u: IPC staging allocation of %llu B failed", c.rank, (unsigned long long)tr.size.allocBytes());
    }
    // no stale line of a freed cached buffer may be written back over the new staging (as for the flags)
    ok = ok && hipDeviceSynchronize() == hipSuccess && (!c.cfg.ipcL2Scrub || ScrubL2(c.reduceStream) == HCCL_SUCCESS);
    void* peers[kIpcMaxRanks] = {};
    const HcclResult r = MapPeers(c, base, ok, peers, tr.opened, nullptr);
    if (r != HCCL_SUCCESS) {
        if (base != nullptr) UncachedRelease(c.device, base, tr.size.allocBytes());
        tr = IpcTier{};
        tr.unavailable = true;
        return r;
    }
    AreasOf(tr, base, tr.area);
    for (uint32_t q = 0; q < c.nRanks; ++q) {
        void* areas[kIpcAreas];
        AreasOf(tr, peers[q], areas);
        for (int k = 0; k < kIpcAreas; ++k) tr.peerArea[k][q] = areas[k];
    }
    tr.ready = true;
    return HCCL_SUCCESS;
}

// The point-to-point area and counters (IpcEnableP2p); the peers' kernels have finished (IpcQuiesce).
void ReleaseP2p(Comm& c)
{
    IpcState::P2p& p = c.ipc.p2p;
    for (uint32_t r = 0; r < kIpcMaxRanks; ++r) {
        if (p.opened[r]) (void)hipIpcCloseMemHandle(p.peerArea[r]);
    }
    if (p.area != nullptr) UncachedRelease(c.device, p.area, p.areaBytes);
    if (p.counters != nullptr) (void)hipFree(p.counters);
    const bool unavailable = p.unavailable;
    p = IpcState::P2p{};
    p.unavailable = unavailable;
}

// The argument check's area and private words (IpcSetupCheck); the peers' kernels have finished (IpcQuiesce).
void ReleaseCheck(Comm& c)
{
    IpcState::Check& k = c.ipc.check;
    for (uint32_t r = 0; r < kIpcMaxRanks; ++r) {
        if (k.opened[r]) (void)hipIpcCloseMemHandle(k.peerArea[r]);
    }
    if (k.area != nullptr) UncachedRelease(c.device, k.area, kCheckAreaBytes);
    if (k.priv != nullptr) (void)hipFree(k.priv);
    const bool unavailable = k.unavailable, logged = k.logged;
    k = IpcState::Check{};
    k.unavailable = unavailable;
    k.logged = logged;
}

bool Aligned16(const void* p, const void* q)
{
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15u) == 0;
}

// Barrier fences (IpcArgs::fence). Every byte a barrier hands over lives in uncached staging, which no L2 holds: the
// storing waves' vmcnt drains order the data before the flag (a store completes at memory), and an agent-scope acquire
// (the CU's L1) suffices for the reader, whose loads go to memory. The user buffers are never handed over inside the
// kernel (each element is read and written by the lane that owns it); across kernels they are ordered by the ordinary
// kernel boundaries, which make plain and non-temporal stores visible to the next kernel on every XCD
// (tools/probes/coherence_probe.hip, profiles/r04_coherence_probe.jsonl). The light fences skip the system-scope
// release and acquire, which write back and invalidate the whole XCD L2 for every block: 3-13 % per call in loopback
// worlds (profiles/r03_ipc_variant_ab_fence.jsonl). Default (CommConfig::ipcLightFence = -1): light in a loopback
// world, where every store goes through the owner's own uncached pointer; system scope in rank mode, whose stores reach
// the peers' staging through hipIpcOpenMemHandle mappings, and an imported mapping need not keep the exporter's uncached
// memory type (imported mappings). HCCL_AMD_IPC_LIGHT_FENCE=1 or 0 forces either. Equal on every rank.
bool IpcLightFence(const Comm& c)
{
    return c.cfg.ipcLightFence < 0 ? c.transport->SharedDevice() : c.cfg.ipcLightFence != 0;
}

}  // namespace

void IpcQuiesce(Comm& c)
{
    if (!c.ipc.ready || c.ipcQuiesced) return;
    c.ipcQuiesced = true;
    // Peers store into this rank's staging and flags: unmapping or freeing them while any peer's kernel may still
    // run would fault that peer. Wait for this device, then for every rank to get here (each has waited for its own).
    (void)hipDeviceSynchronize();
    // A loopback world has no rendezvous here: its ranks are destroyed one after another from any thread (a host
    // exchange would wait for ranks that are destroyed later on the same thread), and every one-sided launch of the
    // world is a single launch on this device, which the device synchronisation above has drained; a world whose ranks
    // are destroyed while others still issue collectives is outside the contract.
    if (c.transport->SharedDevice()) return;
    uint8_t mine = 1;
    std::vector<uint8_t> all(c.nRanks);
    if (c.transport->AllGatherHost(&mine, 1, all.data()) != HCCL_SUCCESS) {
        HCCL_AMD_ERR("rank %u: IPC teardown rendezvous failed; peer mappings are left in place", c.rank);
        c.ipc = IpcState{};  // leak rather than free memory a peer may still write
    }
}

void IpcRelease(Comm& c)
{
    IpcState& s = c.ipc;
    for (IpcTier& t : s.tier) ReleaseTier(c, t);
    ReleaseP2p(c);
    ReleaseCheck(c);
    for (uint32_t r = 0; r < kIpcMaxRanks; ++r) {
        if (s.flagsOpened[r]) (void)hipIpcCloseMemHandle(s.peerFlags[r]);
    }
    if (s.flags != nullptr) UncachedRelease(c.device, s.flags, FlagAllocBytes());
    if (s.status != nullptr) (void)hipFree(s.status);
    if (s.trace != nullptr) (void)hipFree(s.trace);
    if (s.llUnpack != nullptr) (void)hipFree(s.llUnpack);
    for (hipEvent_t e : s.a2aRing.used) {
        if (e != nullptr) (void)hipEventDestroy(e);
    }
    if (s.a2aRing.dev != nullptr) (void)hipFree(s.a2aRing.dev);
    if (s.a2aRing.host != nullptr) (void)hipHostFree(s.a2aRing.host);
    // the word is no longer watched before it is freed (a failure already seen stays in Comm::failCode)
    c.failWord.store(nullptr, std::memory_order_release);
    if (s.failHost != nullptr) (void)hipHostFree(s.failHost);
    const bool unavailable = s.unavailable, p2pUnavailable = s.p2p.unavailable;
    const IpcState::Check check = s.check;  // released above: what is left are its flags
    s = IpcState{};
    s.unavailable = unavailable;
    s.p2p.unavailable = p2pUnavailable;
    s.check = check;
}

uint64_t IpcDeviceBytes(const Comm& c)
{
    const IpcState& s = c.ipc;
    uint64_t b = 0;
    if (s.flags != nullptr) b += FlagAllocBytes();
    if (s.status != nullptr) b += kIpcStatusBytes;
    if (s.llUnpack != nullptr) b += kIpcLlUnpackBytes;
    if (s.a2aRing.dev != nullptr) b += uint64_t(kIpcA2aRingSlots) * kIpcMaxRanks * sizeof(IpcA2aTables);
    if (s.trace != nullptr) b += uint64_t(kIpcMaxRanks) * kIpcMaxBlocks * kIpcTraceSlots * sizeof(uint64_t);
    for (const IpcTier& t : s.tier) {
        if (t.area[0] != nullptr) b += t.size.allocBytes();
    }
    if (s.p2p.area != nullptr) b += s.p2p.areaBytes;
    if (s.p2p.counters != nullptr) b += s.p2p.counterBytes;
    if (s.check.area != nullptr) b += kCheckAreaBytes;
    if (s.check.priv != nullptr) b += kCheckPrivBytes;
    return b;
}

// ------------------------------------------------------------------------------------------------ calls

HcclResult RunIpcCollective(Comm& c, int32_t opType, int32_t family, const void* sendBuf, void* recvBuf,
                            uint64_t count, HcclDataType dt, HcclReduceOp op, uint32_t root, hipStream_t stream)
{
    const uint64_t es = DataTypeSize(dt);
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    IpcPlan plan{};
    HCCL_CHK(IpcPlanForFamily(opType, family, c.nRanks, es, c.cclBytes, &plan));
    return RunIpcPlan(c, opType, plan, sendBuf, recvBuf, count, dt, op, root, stream);
}

HcclResult RunIpcBroadcast(Comm& c, void* buf, uint64_t count, HcclDataType dt, uint32_t root, hipStream_t stream)
{
    const uint64_t es = DataTypeSize(dt);
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    return RunIpcPlan(c, HCCL_AMD_OP_BROADCAST, IpcPlanBroadcast(count, es, c.bcastKind), buf, buf, count, dt,
                      HCCL_REDUCE_SUM, root, stream);
}

HcclResult RunIpcAllToAll(Comm& c, const void* sendBuf, void* recvBuf, const IpcA2aTables& tables, uint64_t maxCount,
                          bool agreed, HcclDataType dt, hipStream_t stream)
{
    if (DataTypeSize(dt) == 0) return HCCL_E_NOT_SUPPORT;
    return RunIpcPlan(c, HCCL_AMD_OP_ALLTOALL, IpcPlanAllToAll(agreed), sendBuf, recvBuf, agreed ? 0 : maxCount, dt,
                      HCCL_REDUCE_SUM, 0, stream, nullptr, nullptr, &tables);
}

HcclResult RunIpcScatter(Comm& c, const void* sendBuf, void* recvBuf, uint64_t recvCount, HcclDataType dt,
                         uint32_t root, hipStream_t stream)
{
    if (DataTypeSize(dt) == 0) return HCCL_E_NOT_SUPPORT;
    return RunIpcPlan(c, HCCL_AMD_OP_SCATTER, IpcPlanScatter(), sendBuf, recvBuf, recvCount, dt, HCCL_REDUCE_SUM, root,
                      stream);
}

HcclResult RunIpcAllGatherV(Comm& c, const void* sendBuf, void* recvBuf, const uint64_t* recvCounts,
                            const uint64_t* recvDispls, HcclDataType dt, hipStream_t stream)
{
    if (DataTypeSize(dt) == 0) return HCCL_E_NOT_SUPPORT;
    return RunIpcPlan(c, HCCL_AMD_OP_ALLGATHER_V, IpcPlanAllGatherV(), sendBuf, recvBuf, recvCounts[c.rank], dt,
                      HCCL_REDUCE_SUM, 0, stream, recvCounts, recvDispls);
}

namespace {

// A call as planned (ipc_plan.h): what the launch loops below need to make each loop's geometry.
struct PlannedCall {
    IpcCall call;
    IpcEnv env;
    bool ll;
    uint32_t blocks;
    std::vector<IpcLoop> loops;
    uint64_t slotCap;
};

// Copies loop k's geometry into the launch arguments: the only place that writes these fields.
void SetGeometry(IpcArgs& a, const PlannedCall& p, size_t k)
{
    const IpcGeometry g = IpcLoopGeometry(p.call, p.env, p.loops[k].cnt, p.slotCap, p.blocks, p.ll);
    a.total = g.total;
    a.chunkStride = g.chunkStride;
    a.chunkLen = g.chunkLen;
    a.rem = g.rem;
    a.group = g.group;
    a.balanced = g.balanced != 0;
    a.vgeom = g.vgeom != 0;
    if (a.vgeom) {
        std::memcpy(a.vStart, g.vStart, sizeof a.vStart);
        std::memcpy(a.vLen, g.vLen, sizeof a.vLen);
    }
    a.piece = g.piece;
    a.blockElems = g.blockElems;
    a.tileElems = g.tileElems;
    a.rounds = g.rounds;
    a.epochSpan = g.epochSpan;
    a.ll = g.ll;
}

// The RHD schedule's parts and relabelling (AllReduceRhd): R instances over Chunk(count, R, j) parts.
HcclResult SetRhdParts(IpcArgs& a, const PlannedCall& p)
{
    const uint32_t n = p.env.n;
    const uint64_t es = p.env.es, count = p.call.count;
    const std::vector<std::vector<uint32_t>> table = RhdTable(n);
    const uint32_t parts = std::min<uint32_t>(static_cast<uint32_t>(table.size()), RhdInstances(n, count * es));
    if (parts == 0 || p.call.plan.loopElems != 0) return HCCL_E_INTERNAL;
    a.rhdParts = parts;
    a.alignElems = static_cast<uint32_t>(std::max<uint64_t>(1, 128 / es));
    const uint64_t stride = (count + parts - 1) / parts;
    a.rhdPartStride = std::max<uint64_t>(1, (stride + a.alignElems - 1) / a.alignElems * a.alignElems);
    for (uint32_t j = 0; j < parts; ++j) {
        for (uint32_t v = 0; v < n; ++v) a.rhdReal[j][v] = static_cast<uint8_t>(table[j][v]);
    }
    return HCCL_SUCCESS;
}

// The staging tier (IpcTier) of a call that is not in the LL form: the small one when every launch of the call fits
// one round there, else the large one (also when the small tier's set-up failed). The choice depends on the call's
// arguments and the configuration at the set-up, equal on every rank, and each tier's availability is agreed, so every
// rank takes the same tier. No collective set-up under capture.
HcclResult SetupTierFor(Comm& c, bool fitsSmall, bool capturing, const IpcTier** tier)
{
    IpcState& s = c.ipc;
    int t = fitsSmall && !s.tier[kIpcTierSmall].unavailable ? kIpcTierSmall : kIpcTierLarge;
    if (capturing && !s.tier[t].ready) return HCCL_E_NOT_SUPPORT;
    HcclResult r = IpcSetupTier(c, t);
    if (r == HCCL_E_NOT_SUPPORT && t == kIpcTierSmall) {
        t = kIpcTierLarge;
        if (capturing && !s.tier[t].ready) return HCCL_E_NOT_SUPPORT;
        r = IpcSetupTier(c, t);
    }
    HCCL_CHK(r);
    *tier = &s.tier[t];
    return HCCL_SUCCESS;
}

char* At(const void* p, uint64_t off, uint64_t es) { return static_cast<char*>(const_cast<void*>(p)) + off * es; }

// Rank mode: this rank's launches, one per loop.
HcclResult LaunchRank(Comm& c, IpcArgs& a, const PlannedCall& p, const void* sendBuf, void* recvBuf, HcclDataType dt,
                      HcclReduceOp op, hipStream_t stream, IpcA2aArgs* x, const IpcA2aTables* tables)
{
    a.me = static_cast<int32_t>(c.rank);
    if (x != nullptr) x->mine = *tables;  // by value: a captured launch carries them
    a.aligned = Aligned16(sendBuf, recvBuf);
    a.llUnpack[c.rank] = c.ipc.llUnpack;
    for (size_t k = 0; k < p.loops.size(); ++k) {
        a.in[c.rank] = At(sendBuf, p.loops[k].off, p.env.es);
        a.out[c.rank] = At(recvBuf, p.loops[k].off, p.env.es);
        SetGeometry(a, p, k);
        HCCL_CHK(LaunchIpcCollective(a, p.blocks, 0, dt, op, stream, x));
    }
    return HCCL_SUCCESS;
}

// Loopback world: one launch per loop for every rank, issued by rank 0 behind every rank's stream. Every rank takes
// part in both exchanges whatever its local outcome (one that returned early would leave the others in the
// rendezvous), and a failure anywhere is every rank's result.
// The slot of the issuing rank's table ring for one all-to-all launch of the world, filled with every rank's tables
// and copied to its device twin on `stream`, ahead of the launch. A slot is reused kIpcA2aRingSlots launches later,
// after the launch that read it has ended (the host waits for its event, which has almost always completed).
HcclResult StageWorldTables(Comm& c, const IpcA2aTables* const* tables, uint32_t n, hipStream_t stream,
                            const IpcA2aTables** dev, uint32_t* slotOut)
{
    IpcState::A2aRing& ring = c.ipc.a2aRing;
    const size_t slotTables = kIpcMaxRanks, bytes = size_t(kIpcA2aRingSlots) * slotTables * sizeof(IpcA2aTables);
    if (ring.host == nullptr) {
        if (hipHostMalloc(reinterpret_cast<void**>(&ring.host), bytes, hipHostMallocDefault) != hipSuccess) {
            ring.host = nullptr;
            return HCCL_E_MEMORY;
        }
        if (hipMalloc(reinterpret_cast<void**>(&ring.dev), bytes) != hipSuccess) {
            ring.dev = nullptr;
            return HCCL_E_MEMORY;
        }
        for (hipEvent_t& e : ring.used) HIP_CHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (ring.dev == nullptr) return HCCL_E_MEMORY;
    const uint32_t slot = ring.next++ % kIpcA2aRingSlots;
    if (ring.recorded[slot]) HIP_CHK(hipEventSynchronize(ring.used[slot]));
    IpcA2aTables* h = ring.host + slot * slotTables;
    for (uint32_t r = 0; r < n; ++r) h[r] = *tables[r];
    HIP_CHK(hipMemcpyAsync(ring.dev + slot * slotTables, h, n * sizeof(IpcA2aTables), hipMemcpyHostToDevice, stream));
    *dev = ring.dev + slot * slotTables;
    *slotOut = slot;
    return HCCL_SUCCESS;
}

HcclResult LaunchWorld(Comm& c, IpcArgs& a, const PlannedCall& p, const void* sendBuf, void* recvBuf, HcclDataType dt,
                       HcclReduceOp op, hipStream_t stream, IpcA2aArgs* x, const IpcA2aTables* tables)
{
    const uint32_t n = p.env.n;
    struct Part {
        const void* in;
        void* out;
        void* unpack;
        hipEvent_t ready;
        int32_t code;
    };
    // an all-to-all's rendezvous carries the rank's tables too: rank 0's one launch needs every rank's
    struct PartA2a : Part {
        IpcA2aTables tables;
    };
    PartA2a mineA2a{};
    Part& mine = mineA2a;
    mine = Part{sendBuf, recvBuf, c.ipc.llUnpack, nullptr, HCCL_SUCCESS};
    if (x != nullptr) mineA2a.tables = *tables;
    c.nextEvent = 0;
    mine.code = c.NextEvent(&mine.ready);
    if (mine.code == HCCL_SUCCESS && hipEventRecord(mine.ready, stream) != hipSuccess) mine.code = HCCL_E_RUNTIME;
    const size_t stride = x != nullptr ? sizeof(PartA2a) : sizeof(Part);
    std::vector<PartA2a> gathered(x != nullptr ? n : (n * sizeof(Part) + sizeof(PartA2a) - 1) / sizeof(PartA2a));
    HCCL_CHK(c.transport->AllGatherHost(&mine, stride, gathered.data()));
    std::vector<Part> all(n);
    for (uint32_t r = 0; r < n; ++r) {
        all[r] = *reinterpret_cast<const Part*>(reinterpret_cast<const char*>(gathered.data()) + r * stride);
    }
    HcclResult code = HCCL_SUCCESS;
    for (uint32_t r = 0; r < n && code == HCCL_SUCCESS; ++r) code = static_cast<HcclResult>(all[r].code);
    struct Done {
        hipEvent_t ev;
        int32_t code;
    };
    Done done{nullptr, code};
    if (c.rank == 0 && code == HCCL_SUCCESS) {
        a.me = -1;
        a.aligned = true;
        for (uint32_t r = 0; r < n && done.code == HCCL_SUCCESS; ++r) {
            a.aligned = a.aligned && Aligned16(all[r].in, all[r].out);
            if (hipStreamWaitEvent(stream, all[r].ready, 0) != hipSuccess) done.code = HCCL_E_RUNTIME;
        }
        uint32_t ringSlot = 0;
        if (x != nullptr && done.code == HCCL_SUCCESS) {
            const IpcA2aTables* every[kIpcMaxRanks];
            for (uint32_t r = 0; r < n; ++r) every[r] = &gathered[r].tables;
            done.code = StageWorldTables(c, every, n, stream, &x->world, &ringSlot);
        }
        for (size_t k = 0; k < p.loops.size() && done.code == HCCL_SUCCESS; ++k) {
            for (uint32_t r = 0; r < n; ++r) {
                a.in[r] = At(all[r].in, p.loops[k].off, p.env.es);
                a.out[r] = At(all[r].out, p.loops[k].off, p.env.es);
                a.llUnpack[r] = all[r].unpack;
            }
            SetGeometry(a, p, k);
            done.code = LaunchIpcCollective(a, p.blocks, n, dt, op, stream, x);
        }
        if (x != nullptr && done.code == HCCL_SUCCESS) {
            IpcState::A2aRing& ring = c.ipc.a2aRing;
            if (hipEventRecord(ring.used[ringSlot], stream) != hipSuccess) done.code = HCCL_E_RUNTIME;
            ring.recorded[ringSlot] = done.code == HCCL_SUCCESS;
        }
        if (done.code == HCCL_SUCCESS) done.code = c.NextEvent(&done.ev);
        if (done.code == HCCL_SUCCESS && hipEventRecord(done.ev, stream) != hipSuccess) done.code = HCCL_E_RUNTIME;
    }
    std::vector<Done> dones(n);
    HCCL_CHK(c.transport->AllGatherHost(&done, sizeof done, dones.data()));
    if (dones[0].code != HCCL_SUCCESS) return static_cast<HcclResult>(dones[0].code);
    if (c.rank != 0) HIP_CHK(hipStreamWaitEvent(stream, dones[0].ev, 0));
    return HCCL_SUCCESS;
}

// The launch arguments that do not depend on the call's data: the flag table, the status and failure words, the wait
// bound, the call's sequence number and the (=) configuration. The set-up (IpcSetupBase) has succeeded.
void SetCallArgs(Comm& c, IpcArgs& a, IpcKind kind)
{
    IpcState& s = c.ipc;
    for (uint32_t r = 0; r < c.nRanks; ++r) a.flags[r] = s.peerFlags[r];
    a.n = c.nRanks;
    a.kind = kind;
    a.timeoutTicks = c.cfg.ipcTimeoutMs * 100000;  // a lost peer ends the kernel with status bit 0, never a hang
    a.status = s.status;
    a.failHost = s.failDev;
    a.callSeq = ++s.callSeq;  // equal on every rank of a loopback world (each runs this once per call)
    a.trace = s.trace;
    a.nt = c.cfg.ipcNt ? 1u : 0u;         // non-temporal loads and stores (HCCL_AMD_IPC_NT)
    a.fence = IpcLightFence(c) ? 1u : 0u;
    a.threads = c.cfg.ipcThreads;         // HCCL_AMD_IPC_THREADS
}

}  // namespace

HcclResult RunIpcBarrier(Comm& c, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_IPC);
    if (c.nRanks > uint32_t(kIpcMaxRanks)) return HCCL_E_NOT_SUPPORT;
    // Capture as in RunIpcPlan: the epoch lives on the device, so a captured barrier replays; the collective set-up and
    // a loopback world's per-call event exchange cannot be captured.
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) return HCCL_E_NOT_SUPPORT;
    const bool world = c.transport->SharedDevice();
    if (capture != hipStreamCaptureStatusNone && (!c.ipc.ready || world)) return HCCL_E_NOT_SUPPORT;
    // the flags, the status words and the failure word: all a barrier needs; no staging tier is set up or asked for
    HCCL_CHK(IpcSetupBase(c));
    PlannedCall p{};
    p.call = IpcCall{HCCL_AMD_OP_BARRIER, IpcPlanBarrier(), 0};
    p.env.n = c.nRanks;
    p.env.es = 1;
    p.env.sharedDevice = world;
    p.ll = false;
    p.blocks = c.ipc.blocks = 1;
    p.loops = IpcLoops(p.call);
    IpcArgs a{};
    SetCallArgs(c, a, kIpcBarrier);
    // no buffers: a loopback world's launch still goes behind every rank's stream and every rank waits for its end
    return world ? LaunchWorld(c, a, p, nullptr, nullptr, HCCL_DATA_TYPE_INT8, HCCL_REDUCE_SUM, stream, nullptr, nullptr)
                 : LaunchRank(c, a, p, nullptr, nullptr, HCCL_DATA_TYPE_INT8, HCCL_REDUCE_SUM, stream, nullptr, nullptr);
}

HcclResult RunIpcPlan(Comm& c, int32_t opType, const IpcPlan& plan, const void* sendBuf, void* recvBuf,
                      uint64_t count, HcclDataType dt, HcclReduceOp op, uint32_t root, hipStream_t stream,
                      const uint64_t* vCounts, const uint64_t* vDispls, const IpcA2aTables* a2aTables)
{
    const HostProfileScope hp(HCCL_AMD_HP_IPC);
    if (plan.geom == kIpcGeomV && (vCounts == nullptr || vDispls == nullptr || plan.loopElems != 0)) {
        return HCCL_E_INTERNAL;
    }
    uint64_t es = DataTypeSize(dt);
    if (es == 0 || c.nRanks > kIpcMaxRanks) return HCCL_E_NOT_SUPPORT;
    if (opType == HCCL_AMD_OP_ALLGATHER) {
        // pure data movement: any dtype runs as the integer type of its size (16-B types as pairs of 8-B words)
        op = HCCL_REDUCE_SUM;
        switch (es) {
            case 1: dt = HCCL_DATA_TYPE_INT8; break;
            case 2: dt = HCCL_DATA_TYPE_INT16; break;
            case 4: dt = HCCL_DATA_TYPE_INT32; break;
            case 8: dt = HCCL_DATA_TYPE_INT64; break;
            case 16: dt = HCCL_DATA_TYPE_INT64; count *= 2; es = 8; break;
            default: return HCCL_E_NOT_SUPPORT;
        }
    }
    const IpcKind kind = static_cast<IpcKind>(plan.kind);
    // the Broadcast's kinds run a typeless kernel of their own, instantiated for element sizes 1, 2, 4 and 8
    const bool bcast = kind == kIpcBroadcast || kind == kIpcBroadcastOneShot;
    // so does the all-to-all; its agreed form (AlltoAllV) decides nothing from the call's counts
    const bool a2a = kind == kIpcAllToAll;
    const bool agreed = a2a && plan.subMode == kIpcA2aAgreed;
    if (a2a && a2aTables == nullptr) return HCCL_E_INTERNAL;
    // and so do the Scatter and the AllGatherV, in a third one
    const bool sg = kind == kIpcScatter || kind == kIpcAllGatherV;
    if ((bcast || a2a || sg) && es > 8) return HCCL_E_NOT_SUPPORT;
    // Stream capture: the barrier epochs live on the device (status word kIpcEpochWord, advanced once per launch by
    // the block that completes its arrival count), so a captured launch replays correctly: each replay takes the
    // next epochs, as a new call would. Two things cannot be captured: the collective set-up of the first call
    // (allocation, host exchange, device synchronisation) and the loopback world, which exchanges events between
    // host threads per call. Those report NOT_SUPPORT under capture; a communicator with RCCL then takes the RCCL
    // schedule of the same family. Every rank of a collective is captured alike, so they all decide the same way.
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) return HCCL_E_NOT_SUPPORT;
    const bool capturing = capture != hipStreamCaptureStatusNone;
    const bool world = c.transport->SharedDevice();
    if (capturing && (!c.ipc.ready || world)) return HCCL_E_NOT_SUPPORT;
    HCCL_CHK(IpcSetupBase(c));
    IpcState& s = c.ipc;
    const uint32_t n = c.nRanks;

    // The form and the workgroups per rank (ipc_plan.h). The residency cap lies between the two: the blocks the device
    // holds at once depend on the kernel, so on the form, and are shared by the ranks on this device (a loopback world
    // puts every rank's blocks on it; in rank mode, the ranks whose processes share it, counted at set-up by PCI bus
    // id). The count depends only on the kernel, the device and the placement, so ranks of a node agree on it.
    PlannedCall p{};
    p.call = IpcCall{opType, plan, count, vCounts, vDispls};
    p.env.n = n;
    p.env.es = es;
    p.env.sharedDevice = world;
    p.env.blocksOverride = c.ipcBlocks;
    p.env.tileBytes = c.cfg.ipcTileBytes;
    p.env.llBytes = c.cfg.ipcLlBytes;
    p.ll = IpcUseLl(p.call, p.env);
    {
        const uint32_t here = world ? n : std::max<uint32_t>(1, s.ranksOnDevice);
        const uint32_t resident =
            bcast ? IpcBcastResidentBlocks(static_cast<uint32_t>(es), c.cfg.ipcThreads)
            : a2a ? IpcA2aResidentBlocks(static_cast<uint32_t>(es), c.cfg.ipcThreads)
            : sg  ? IpcSgResidentBlocks(static_cast<uint32_t>(es), c.cfg.ipcThreads)
                  : IpcResidentBlocks(dt, op, plan.order == kIpcRhd, p.ll, c.cfg.ipcThreads);
        p.env.residentPerRank = resident != 0 ? std::max<uint32_t>(1, resident / here) : 0;
    }
    // (the agreed all-to-all's blocks follow its tier's capacity: below)
    if (!agreed) p.blocks = s.blocks = IpcBlockCount(p.call, p.env, p.ll);

    // With the small tier's capacity: does every launch fit one round there? The agreed all-to-all always takes the
    // small tier: how many rounds it needs is not common knowledge.
    p.loops = IpcLoops(p.call);
    p.slotCap = IpcSlotCap(kind, p.env, TierSizes(c, kIpcTierSmall));
    bool fitsSmall = true;
    for (const IpcLoop& l : p.loops) {
        fitsSmall = fitsSmall &&
                    (agreed || IpcLoopGeometry(p.call, p.env, l.cnt, p.slotCap, p.blocks, p.ll).rounds == 1);
    }
    // The LL form uses no staging area (its words travel through the flags allocation's LL area).
    IpcArgs a{};
    if (!p.ll) {
        const IpcTier* tr = nullptr;
        HCCL_CHK(SetupTierFor(c, fitsSmall, capturing, &tr));
        p.slotCap = IpcSlotCap(kind, p.env, tr->size);
        if (agreed) {
            p.env.a2aAreaBytes = tr->size.altBytes;
            p.blocks = s.blocks = IpcBlockCount(p.call, p.env, p.ll);
        }
        for (uint32_t q = 0; q < n; ++q) {
            a.stgIn[q] = tr->peerArea[kIpcAreaIn][q];
            a.stgRes[q] = tr->peerArea[kIpcAreaRes][q];
            a.stgAlt[0][q] = tr->peerArea[kIpcAreaAlt0][q];
            a.stgAlt[1][q] = tr->peerArea[kIpcAreaAlt1][q];
        }
    }

    // What every launch of the call shares; SetGeometry adds each loop's own.
    SetCallArgs(c, a, kind);
    a.order = plan.order;
    a.subMode = plan.subMode;
    a.root = root;
    a.outStride = count;
    if (plan.order == kIpcRhd) HCCL_CHK(SetRhdParts(a, p));
    IpcA2aArgs x{};
    if (a2a) {
        // a staging area too small for a slot (and the agreed form's header) cannot run the kind
        if (IpcLoopGeometry(p.call, p.env, count, p.slotCap, p.blocks, false).piece == 0) return HCCL_E_NOT_SUPPORT;
        x.slotElems = p.slotCap;
        x.hdrElems = agreed ? static_cast<uint32_t>(kIpcA2aHeaderBytes / es) : 0;
        x.agreed = agreed ? 1u : 0u;
    }

    return world ? LaunchWorld(c, a, p, sendBuf, recvBuf, dt, op, stream, a2a ? &x : nullptr, a2aTables)
                 : LaunchRank(c, a, p, sendBuf, recvBuf, dt, op, stream, a2a ? &x : nullptr, a2aTables);
}

// ------------------------------------------------------------------------------------------------ argument check

namespace {

// The check's area and private words (collective, at the communicator's first checked call; IpcSetupBase has
// succeeded): as IpcEnableP2p sets up the point-to-point area. The area is zeroed before the ranks exchange it: a block
// from the idle pool carries an earlier communicator's sequence numbers, and this one's begin at 1 again.
HcclResult IpcSetupCheck(Comm& c)
{
    IpcState::Check& k = c.ipc.check;
    if (k.ready) return HCCL_SUCCESS;
    if (k.unavailable) return HCCL_E_NOT_SUPPORT;
    const uint32_t n = c.nRanks;
    void* area = nullptr;
    uint64_t* priv = nullptr;
    bool ok = c.cfg.injectIpcAllocFail != static_cast<int32_t>(c.rank) && UncachedAlloc(c.device, &area, kCheckAreaBytes);
    if (!ok) area = nullptr;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&priv), kCheckPrivBytes) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess && (!c.cfg.ipcL2Scrub || ScrubL2(c.reduceStream) == HCCL_SUCCESS) &&
         hipMemset(area, 0, kCheckAreaBytes) == hipSuccess && hipMemset(priv, 0, kCheckPrivBytes) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess;
    if (!ok) HCCL_AMD_ERR("rank %u: argument-check area of %llu B not set up", c.rank, (unsigned long long)kCheckAreaBytes);
    void* peers[kIpcMaxRanks] = {};
    HcclResult r = MapPeers(c, area, ok, peers, k.opened, nullptr);
    struct Words {
        uint64_t* priv;
        uint32_t* status;
    };
    const Words mine{priv, c.ipc.status};
    std::vector<Words> all(n, Words{nullptr, nullptr});
    if (r == HCCL_SUCCESS && c.transport->SharedDevice()) r = c.transport->AllGatherHost(&mine, sizeof mine, all.data());
    if (r != HCCL_SUCCESS) {
        if (area != nullptr) UncachedRelease(c.device, area, kCheckAreaBytes);
        if (priv != nullptr) (void)hipFree(priv);
        const bool logged = k.logged;
        k = IpcState::Check{};
        k.unavailable = true;
        k.logged = logged;
        return r;
    }
    k.area = area;
    k.priv = priv;
    for (uint32_t q = 0; q < n; ++q) {
        k.peerArea[q] = peers[q];
        k.peerPriv[q] = all[q].priv;
        k.peerStatus[q] = all[q].status;
    }
    k.ready = true;
    return HCCL_SUCCESS;
}

// One line, once per communicator, when checked calls run unchecked.
void LogUnchecked(Comm& c, const char* why)
{
    if (c.ipc.check.logged) return;
    c.ipc.check.logged = true;
    HCCL_AMD_ERR("rank %u: inconsistent_check is on but calls run unchecked: %s", c.rank, why);
}

}  // namespace

HcclResult RunIpcCheck(Comm& c, const CheckRecord& rec, hipStream_t stream)
{
    const int32_t mode = c.cfg.inconsistentCheck;
    if (mode < 0) return HCCL_SUCCESS;
    const HostProfileScope hp(HCCL_AMD_HP_IPC);
    IpcState::Check& k = c.ipc.check;
    const uint32_t n = c.nRanks, opBit = 1u << (rec.w[CheckFirstWord(HCCL_AMD_CHECK_OP_TYPE)] & 31u);
    if (mode == 0 && (k.seenOps & opBit) != 0) return HCCL_SUCCESS;  // first: this operator type has been checked
    // Communicators without the one-sided flag mapping: the self loop, more than kIpcMaxRanks ranks, a failed set-up.
    if (c.transport->SelfLoop() || n > uint32_t(kIpcMaxRanks)) {
        LogUnchecked(c, "the communicator has no one-sided flag mapping");
        return HCCL_SUCCESS;
    }
    if (c.ipc.unavailable || k.unavailable) {
        LogUnchecked(c, "the one-sided set-up failed");
        return HCCL_SUCCESS;
    }
    // Capture as in RunIpcPlan: the sequence number lives on the device, so a captured check replays. The collective
    // set-up and a loopback world's per-call event exchange cannot be captured: such a call runs unchecked (every rank
    // of a collective is captured alike, so they all decide the same way), and in `first` mode no capture consumes the
    // operator type's first.
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) return HCCL_E_RUNTIME;
    const bool capturing = capture != hipStreamCaptureStatusNone;
    const bool world = c.transport->SharedDevice();
    if (capturing && (!k.ready || world)) return HCCL_SUCCESS;
    HcclResult r = IpcSetupBase(c);
    if (r == HCCL_SUCCESS) r = IpcSetupCheck(c);
    if (r == HCCL_E_NOT_SUPPORT) {  // agreed: it failed on every rank alike
        LogUnchecked(c, "the one-sided set-up failed");
        return HCCL_SUCCESS;
    }
    HCCL_CHK(r);
    if (!capturing) k.seenOps |= opBit;

    IpcCheckArgs a{};
    a.n = n;
    a.timeoutTicks = c.cfg.ipcTimeoutMs * 100000;
    a.failHost = c.ipc.failDev;
    for (uint32_t q = 0; q < n; ++q) a.area[q] = static_cast<uint64_t*>(k.peerArea[q]);
    if (!world) {
        a.me = static_cast<int32_t>(c.rank);
        a.priv[c.rank] = k.priv;
        a.status[c.rank] = c.ipc.status;
        a.sticky = c.ipc.status;
        a.rec[c.rank] = rec;
        const hipError_t e = LaunchIpcCheck(a, 0, stream);
        if (e != hipSuccess) {
            HCCL_AMD_ERR("argument-check launch failed: %s", hipGetErrorString(e));
            return HCCL_E_RUNTIME;
        }
        return HCCL_SUCCESS;
    }
    // Loopback world, as LaunchWorld: one launch for every rank, issued by rank 0 behind every rank's stream; every
    // rank waits for its end. The rendezvous carries the rank's record.
    struct Part {
        CheckRecord rec;
        hipEvent_t ready;
        int32_t code;
    };
    Part mine{rec, nullptr, HCCL_SUCCESS};
    c.nextEvent = 0;
    mine.code = c.NextEvent(&mine.ready);
    if (mine.code == HCCL_SUCCESS && hipEventRecord(mine.ready, stream) != hipSuccess) mine.code = HCCL_E_RUNTIME;
    std::vector<Part> all(n);
    HCCL_CHK(c.transport->AllGatherHost(&mine, sizeof mine, all.data()));
    HcclResult code = HCCL_SUCCESS;
    for (uint32_t q = 0; q < n && code == HCCL_SUCCESS; ++q) code = static_cast<HcclResult>(all[q].code);
    struct Done {
        hipEvent_t ev;
        int32_t code;
    };
    Done done{nullptr, code};
    if (c.rank == 0 && code == HCCL_SUCCESS) {
        a.me = -1;
        a.sticky = c.ipc.status;  // rank 0 issues every launch of the world: its word is the one they test
        for (uint32_t q = 0; q < n && done.code == HCCL_SUCCESS; ++q) {
            a.priv[q] = k.peerPriv[q];
            a.status[q] = k.peerStatus[q];
            a.rec[q] = all[q].rec;
            if (hipStreamWaitEvent(stream, all[q].ready, 0) != hipSuccess) done.code = HCCL_E_RUNTIME;
        }
        if (done.code == HCCL_SUCCESS && LaunchIpcCheck(a, n, stream) != hipSuccess) done.code = HCCL_E_RUNTIME;
        if (done.code == HCCL_SUCCESS) done.code = c.NextEvent(&done.ev);
        if (done.code == HCCL_SUCCESS && hipEventRecord(done.ev, stream) != hipSuccess) done.code = HCCL_E_RUNTIME;
    }
    std::vector<Done> dones(n);
    HCCL_CHK(c.transport->AllGatherHost(&done, sizeof done, dones.data()));
    if (dones[0].code != HCCL_SUCCESS) return static_cast<HcclResult>(dones[0].code);
    if (c.rank != 0) HIP_CHK(hipStreamWaitEvent(stream, dones[0].ev, 0));
    return HCCL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ point-to-point

HcclResult IpcEnableP2p(Comm& c)
{
    IpcState::P2p& p = c.ipc.p2p;
    if (p.ready || c.nRanks == 1) return HCCL_SUCCESS;  // a one-rank communicator has self pairs only
    if (p.unavailable || c.nRanks > uint32_t(kIpcMaxRanks)) return HCCL_E_NOT_SUPPORT;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c.reduceStream, &capture) != hipSuccess || capture != hipStreamCaptureStatusNone) {
        return HCCL_E_NOT_SUPPORT;
    }
    // what every one-sided call needs: the sticky bit, the failure word, the ranks per device
    HCCL_CHK(IpcSetupBase(c));
    const uint32_t n = c.nRanks;
    const bool world = c.transport->SharedDevice();
    P2pPlan plan{};
    bool ok = P2pPlanFor(0, 1, c.cfg.p2pSlotBytes, n, &plan) == HCCL_SUCCESS;
    // The largest launch, a batch with both directions to every peer, must be resident at once beside those of the
    // ranks that share the device: its lanes wait for the peers' lanes. Decided here, once and on every rank alike,
    // not per call: the two ends of a message see different batches. (A loopback world's launch holds one message.)
    for (uint32_t es = 1; es <= 8 && ok; es *= 2) {
        const uint32_t resident = IpcP2pResidentBlocks(es, c.cfg.ipcThreads);
        const uint32_t lanes = world ? 2 : 2 * (n - 1);
        ok = resident == 0 || uint64_t(kP2pBlocks) * lanes * std::max<uint32_t>(1, c.ipc.ranksOnDevice) <= resident;
    }
    void* area = nullptr;
    uint32_t* counters = nullptr;
    ok = ok && c.cfg.injectIpcAllocFail != static_cast<int32_t>(c.rank) && UncachedAlloc(c.device, &area, plan.areaBytes);
    if (!ok) area = nullptr;
    // zeroed flags and counters, behind the same L2 maintenance as the collectives' flags (IpcSetupBase)
    ok = ok && hipMalloc(reinterpret_cast<void**>(&counters), plan.counterBytes) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess && (!c.cfg.ipcL2Scrub || ScrubL2(c.reduceStream) == HCCL_SUCCESS) &&
         hipMemset(static_cast<char*>(area) + plan.dataBytes, 0, plan.areaBytes - plan.dataBytes) == hipSuccess &&
         hipMemset(counters, 0, plan.counterBytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) HCCL_AMD_ERR("rank %u: point-to-point area of %llu B not set up", c.rank, (unsigned long long)plan.areaBytes);
    void* peers[kIpcMaxRanks] = {};
    HcclResult r = MapPeers(c, area, ok, peers, p.opened, nullptr);
    std::vector<uint32_t*> ctrs(n, nullptr);
    if (r == HCCL_SUCCESS && world) r = c.transport->AllGatherHost(&counters, sizeof counters, ctrs.data());
    if (r != HCCL_SUCCESS) {
        if (area != nullptr) UncachedRelease(c.device, area, plan.areaBytes);
        if (counters != nullptr) (void)hipFree(counters);
        p = IpcState::P2p{};
        p.unavailable = true;
        return r;
    }
    p.area = area;
    p.counters = counters;
    for (uint32_t q = 0; q < n; ++q) {
        p.peerArea[q] = peers[q];
        p.peerCounters[q] = ctrs[q];
    }
    p.slotBytes = c.cfg.p2pSlotBytes;
    p.areaBytes = plan.areaBytes;
    p.counterBytes = plan.counterBytes;
    p.ready = true;
    return HCCL_SUCCESS;
}

namespace {

// What every launch of the point-to-point kernel shares. callSeq stays as it is: the kernel publishes no wait.
HcclResult P2pLaunchArgs(Comm& c, uint64_t es, IpcArgs* a, IpcP2pArgs* x)
{
    P2pPlan plan{};
    HCCL_CHK(P2pPlanFor(0, es, c.ipc.p2p.slotBytes, c.nRanks, &plan));
    a->n = c.nRanks;
    a->me = static_cast<int32_t>(c.rank);
    a->timeoutTicks = c.cfg.ipcTimeoutMs * 100000;
    a->status = c.ipc.status;
    a->failHost = c.ipc.failDev;
    a->trace = c.ipc.trace;
    a->nt = c.cfg.ipcNt ? 1u : 0u;
    a->fence = IpcLightFence(c) ? 1u : 0u;
    a->threads = c.cfg.ipcThreads;
    x->slotBytes = c.ipc.p2p.slotBytes;
    x->slotElems = plan.slotElems;
    x->blockElems = plan.blockElems;
    return HCCL_SUCCESS;
}

HcclResult LaunchP2p(uint64_t es, const IpcArgs& a, const IpcP2pArgs& x, uint32_t lanes, hipStream_t stream)
{
    const hipError_t e = LaunchIpcP2p(static_cast<uint32_t>(es), a, x, dim3(kP2pBlocks, lanes), stream);
    if (e != hipSuccess) {
        HCCL_AMD_ERR("ipc point-to-point launch failed: %s", hipGetErrorString(e));
        return HCCL_E_RUNTIME;
    }
    return HCCL_SUCCESS;
}

}  // namespace

HcclResult RunIpcP2p(Comm& c, const std::vector<P2pOp>& ops, uint64_t es, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_IPC);
    IpcState::P2p& p = c.ipc.p2p;
    if (!p.ready || (es != 1 && es != 2 && es != 4 && es != 8)) return HCCL_E_NOT_SUPPORT;
    if (ops.size() > kP2pMaxItems) return HCCL_E_NOT_SUPPORT;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) return HCCL_E_NOT_SUPPORT;
    const bool world = c.transport->SharedDevice();
    if (world && capture != hipStreamCaptureStatusNone) return HCCL_E_NOT_SUPPORT;
    IpcArgs a{};
    IpcP2pArgs x{};
    HCCL_CHK(P2pLaunchArgs(c, es, &a, &x));
    if (world) {
        // Separate launches from the rank threads would share the process's few hardware queues, and a receiver could
        // sit in front of its own sender. So, as the world's collectives do, a matched message is one launch holding
        // both roles, issued by the receiver's thread after the transport's own rendezvous: lane 0 the sender (its
        // buffer, area and counters), lane 1 this rank.
        const Transport::P2pCopyFn viaSlots = [&](void* dst, const void* src, uint64_t bytes, uint32_t from,
                                                  hipStream_t s) {
            IpcP2pArgs m = x;
            m.item[0] = {const_cast<void*>(src), bytes / es};
            m.item[1] = {dst, bytes / es};
            m.lane[0] = {static_cast<char*>(p.peerArea[from]), static_cast<char*>(p.area), p.peerCounters[from], 1,
                         static_cast<uint8_t>(from), static_cast<uint8_t>(c.rank), 0, 1};
            m.lane[1] = {static_cast<char*>(p.area), static_cast<char*>(p.peerArea[from]), p.counters, 0,
                         static_cast<uint8_t>(c.rank), static_cast<uint8_t>(from), 1, 1};
            return LaunchP2p(es, a, m, 2, s);
        };
        return c.transport->GroupVia(ops, stream, viaSlots);
    }
    // Rank mode: this rank's lanes, in the order their first items appear; a lane's items keep their order.
    uint32_t lanes = 0, items = 0;
    for (const P2pOp& o : ops) {
        uint32_t l = 0;
        while (l < lanes && !(x.lane[l].isSend == (o.isSend ? 1 : 0) && x.lane[l].peerRank == o.peer)) ++l;
        if (l == lanes) {
            if (o.peer >= c.nRanks || o.peer == c.rank) return HCCL_E_INTERNAL;
            x.lane[lanes++] = {static_cast<char*>(p.area), static_cast<char*>(p.peerArea[o.peer]), p.counters,
                               static_cast<uint8_t>(o.isSend ? 1 : 0), static_cast<uint8_t>(c.rank),
                               static_cast<uint8_t>(o.peer), 0, 0};
        }
        ++x.lane[l].num;
    }
    for (uint32_t l = 0; l < lanes; ++l) {
        x.lane[l].first = static_cast<uint8_t>(items);
        for (const P2pOp& o : ops) {
            if (x.lane[l].isSend == (o.isSend ? 1 : 0) && x.lane[l].peerRank == o.peer) {
                x.item[items++] = {o.ptr, o.bytes / es};
            }
        }
    }
    // (IpcEnableP2p has checked that the largest launch is resident beside the other ranks' on this device)
    return LaunchP2p(es, a, x, lanes, stream);
}

}  // namespace hccl_amd

using namespace hccl_amd;

extern "C" HcclResult HcclAmdCommIpcStatus(HcclComm comm, uint32_t* status)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || status == nullptr) return HCCL_E_PTR;
    *status = 0;
    if (!c->ipc.ready) return HCCL_SUCCESS;
    HIP_CHK(hipSetDevice(c->device));
    uint32_t w[4] = {0, 0, 0, 0};
    HIP_CHK(hipMemcpy(w, c->ipc.status, sizeof w, hipMemcpyDeviceToHost));
    const uint32_t wait = w[3] == c->ipc.callSeq ? w[2] : 0;  // an older tag: no block of the last call waited
    uint32_t lg = 0;
    while (lg < 32 && (uint64_t(1) << lg) <= wait) ++lg;  // bit length of the longest wait
    *status = (w[0] & 0xFFu) | (lg << 8);
    return HCCL_SUCCESS;
}

extern "C" HcclResult HcclAmdCommInconsistency(HcclComm comm, HcclAmdInconsistency* info)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || info == nullptr) return HCCL_E_PTR;
    *info = HcclAmdInconsistency{};
    if (!c->ipc.check.ready) return HCCL_E_NOT_FOUND;
    HIP_CHK(hipSetDevice(c->device));
    // the report is written by a kernel: wait for it (behind a failed check the one-sided launches return at once)
    HIP_CHK(hipDeviceSynchronize());
    uint64_t w[kCheckPrivWords] = {};
    HIP_CHK(hipMemcpy(w, c->ipc.check.priv, sizeof w, hipMemcpyDeviceToHost));
    if (w[kCheckHasReport] == 0) return HCCL_E_NOT_FOUND;
    info->peer = static_cast<uint32_t>(w[kCheckPeer]);
    info->field = static_cast<int32_t>(w[kCheckField]);
    const char* name = HcclAmdCheckFieldName(info->field);
    std::snprintf(info->name, sizeof info->name, "%s", name != nullptr ? name : "");
    info->local = w[kCheckLocal];
    info->remote = w[kCheckRemote];
    if (!c->ipc.check.reported) {
        c->ipc.check.reported = true;
        // ReportOpExchangeInfoCheckFailed (inconsistent_check.cc:176-206)
        HCCL_AMD_ERR("rank %u: op information %s check fail. remoteRank[%u] expectValue[%llu] remotePara[%llu]", c->rank,
                     info->name, info->peer, (unsigned long long)info->local, (unsigned long long)info->remote);
    }
    return HCCL_SUCCESS;
}

extern "C" HcclResult HcclAmdCommCheckLaunches(HcclComm comm, uint32_t* launches)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || launches == nullptr) return HCCL_E_PTR;
    *launches = 0;
    if (!c->ipc.check.ready) return HCCL_SUCCESS;
    HIP_CHK(hipSetDevice(c->device));
    HIP_CHK(hipDeviceSynchronize());
    uint64_t seq = 0;
    HIP_CHK(hipMemcpy(&seq, c->ipc.check.priv + kCheckSeq, sizeof seq, hipMemcpyDeviceToHost));
    *launches = static_cast<uint32_t>(seq);
    return HCCL_SUCCESS;
}

extern "C" HcclResult HcclAmdCommEnableP2p(HcclComm comm)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    HCCL_CHK(c->Gate());
    HIP_CHK(hipSetDevice(c->device));
    return IpcEnableP2p(*c);
}

extern "C" HcclResult HcclAmdCommIpcLlLaunches(HcclComm comm, uint32_t* launches)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || launches == nullptr) return HCCL_E_PTR;
    *launches = 0;
    if (!c->ipc.ready) return HCCL_SUCCESS;
    HIP_CHK(hipSetDevice(c->device));
    HIP_CHK(hipMemcpy(launches, c->ipc.status + kIpcLlSeqWord, sizeof *launches, hipMemcpyDeviceToHost));
    return HCCL_SUCCESS;
}

extern "C" HcclResult HcclAmdCommIpcTrace(HcclComm comm, uint64_t* stamps, uint64_t cap, uint32_t* blocks)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || stamps == nullptr || blocks == nullptr) return HCCL_E_PTR;
    *blocks = 0;
    if (!c->ipc.ready || c->ipc.trace == nullptr) return HCCL_E_NOT_SUPPORT;
    const uint64_t want = uint64_t(kIpcMaxRanks) * kIpcMaxBlocks * kIpcTraceSlots;
    if (cap < want) return HCCL_E_PARA;
    HIP_CHK(hipSetDevice(c->device));
    HIP_CHK(hipDeviceSynchronize());
    HIP_CHK(hipMemcpy(stamps, c->ipc.trace, want * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *blocks = c->ipc.blocks;
    return HCCL_SUCCESS;
}
