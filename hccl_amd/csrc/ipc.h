// ipc.h — one-sided AllReduce / ReduceScatter / Reduce / AllGather over peer-mapped staging (host state + launch;
// the kinds, orders, layouts and the planning arithmetic are in ipc_plan.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hccl_types.h"
#include "ipc_plan.h"

namespace hccl_amd {

// Staging areas of a rank, parts of one allocation (one IPC handle): slots, results, and the two alternate slot areas
// of the single-barrier kinds.
constexpr int kIpcAreas = 4;
constexpr int kIpcAreaIn = 0;
constexpr int kIpcAreaRes = 1;
constexpr int kIpcAreaAlt0 = 2;
constexpr int kIpcAreaAlt1 = 3;
constexpr int kIpcBlock = 256;        // threads per workgroup of the one-sided kernel (default)
constexpr int kIpcMaxThreads = 512;   // HCCL_AMD_IPC_THREADS may take 512 (r03 A/B)

// Kernel arguments. In rank mode (me >= 0) only in[me] / out[me] are used; stgIn / stgRes / flags hold every rank's
// mapping (own allocation at [me], peers opened through hipIpcOpenMemHandle). In world mode (me < 0) every table is
// full and blockIdx.y is the rank.
//
// Geometry (elements): chunk c of the input starts at c * chunkStride and holds min(chunkLen, total - c*chunkStride)
// elements (clamped at 0), or, balanced (group * n slices of chunkLen, the first rem one longer; chunk c = slices
// [c*group, (c+1)*group)), as the fields below say; rank c owns chunk c. The one-shot kinds use chunkStride = 0, chunkLen = total: every "chunk"
// is the whole range and every rank owns it. Round k handles piece k of every chunk: chunk elements
// [k*piece, (k+1)*piece). Block b always handles piece coordinates [b*blockElems, (b+1)*blockElems), so every round
// of a launch touches the same slot and result addresses per block and the per-block barrier is sound.
// Staging: owner c's slot q = stgIn[c] + q*piece; results of chunk c at stgRes[p] + c*piece. The single-barrier kinds
// (SingleBarrierKind) put their slots in one of two alternate areas instead, stgAlt[e & 1][c] + q*piece for the round
// whose barrier has epoch e (see k_ipc_collective).
struct IpcArgs {
    const void* in[kIpcMaxRanks];
    void* out[kIpcMaxRanks];
    void* stgIn[kIpcMaxRanks];
    void* stgRes[kIpcMaxRanks];
    void* stgAlt[2][kIpcMaxRanks];
    uint32_t* flags[kIpcMaxRanks];  // [blocks][n] per rank
    uint32_t n;
    int32_t me;
    uint32_t kind;  // IpcKind
    uint32_t order;    // IpcOrder
    uint32_t subMode;  // IpcSubMode (kIpcO6 only)
    uint32_t root;  // kIpcReduce, kIpcReduceOneShot, the Broadcast's kinds, kIpcScatter
    uint64_t total;
    uint64_t chunkStride;
    uint64_t chunkLen;
    uint64_t rem;   // balanced: chunkLen is the slice length, rem the number of one-longer slices
    uint64_t group;  // balanced: slices per chunk; chunk c starts at c*group*chunkLen + min(c*group, rem) and holds
                     // group*chunkLen + min(group, rem - c*group clamped at 0) elements
    bool balanced;
    uint64_t piece;
    uint64_t blockElems;
    uint64_t tileElems;  // 0: block b's share of a piece is one window of blockElems; else tiles of tileElems at
                         // b, b + B, b + 2B, ... (B = blocks): the same piece coordinates in every round either way
    uint32_t nt;         // non-temporal loads and stores in the copy and fold loops
    uint32_t threads;    // threads per workgroup (kIpcBlock, or 512 by HCCL_AMD_IPC_THREADS)
    uint32_t fence;      // barrier fences: 1 = light (default): the waves' drains release the uncached staging, an
                         // agent-scope acquire (L1); 0 = system-scope release (XCD-wide L2 write-back) and acquire
                         // (L2 invalidate): HCCL_AMD_IPC_LIGHT_FENCE=0, and always with cached staging
    uint32_t rounds;
    uint32_t epochSpan;  // barriers per block in this launch: the device epoch counter advances by this much
    uint64_t outStride;  // kIpcAllGather: elements between consecutive ranks' blocks of the output (sendCount)
    uint64_t timeoutTicks;  // per barrier wait, in s_memrealtime ticks (100 MHz)
    uint32_t* failHost;  // host-visible word (pinned, coherent): set to 1 by the block whose barrier times out, read by
                         // the host at every collective entry (Comm::Gate) and by HcclGetCommAsyncError
    uint32_t* status;  // [0] bit 0: a barrier timed out (sticky per communicator); [2..3]: (callSeq << 32) | longest
                       // wait of that call, in polls (64-bit max); [4]: epoch counter (barriers so far, per block);
                       // [5]: blocks of the running launch that have finished (kIpcEpochWord, kIpcDoneWord)
    uint32_t callSeq;  // this call's sequence number on the communicator
    bool aligned;      // every in[] / out[] is 16-B aligned (chunks whose start is not are still element-wise)
    bool vgeom;                          // kIpcGeomV: chunk c is vStart[c], vLen[c] (elements); kIpcAllGatherV: rank c's
                                         // block of every output
    uint64_t vStart[kIpcMaxRanks];
    uint64_t vLen[kIpcMaxRanks];
    uint32_t rhdParts;       // kIpcRhd: RHD instances R (parts of the launch's range)
    uint32_t alignElems;     // kIpcRhd: HCCL_MIN_SLICE_ALIGN (128 B) in elements
    uint64_t rhdPartStride;  // kIpcRhd: elements per part (the last part may be shorter)
    uint8_t rhdReal[kIpcMaxRanks - 1][kIpcMaxRanks];  // kIpcRhd: per instance j, virtual rank -> real rank
    uint64_t* trace;  // HCCL_AMD_IPC_TRACE=1: per rank and block, kIpcTraceSlots s_memrealtime stamps of the phases
                      // (IpcTraceSlot); nullptr = off
    uint32_t ll;      // 1: the one-shot AllReduce through the LL area (flags beside the data, no barrier; LlOneShot)
    void* llUnpack[kIpcMaxRanks];  // ll: each rank's own cached unpack area, slot q at q * piece elements
};

// One rank's all-to-all tables (elements): what it sends to and receives from every peer, and where.
enum IpcA2aRow : uint32_t { kA2aSend = 0, kA2aSdispl = 1, kA2aRecv = 2, kA2aRdispl = 3, kA2aRows = 4 };
struct IpcA2aTables {
    uint64_t v[kA2aRows][kIpcMaxRanks];
};

// The second argument of k_ipc_a2a (kind kIpcAllToAll); IpcArgs keeps its layout, which every other kernel's code
// holds. Rank mode takes this rank's tables by value, so a captured launch carries them. A loopback world's one launch
// needs every rank's: they lie in device memory, in a slot of the issuing rank's ring (IpcState::a2aRing), filled by a
// copy on the launch's stream just ahead of it, so back-to-back calls with different counts never share a slot.
// Slot q of a rank's alternate area starts at q * slotElems elements; its first hdrElems elements are the header of the
// agreed form (one 32-bit word per workgroup: the sender's own round need), the round's data follows.
struct IpcA2aArgs {
    IpcA2aTables mine;          // rank mode (IpcArgs::me >= 0)
    const IpcA2aTables* world;  // world mode: [n]
    uint64_t slotElems;
    uint32_t hdrElems;
    uint32_t agreed;  // 1: IpcArgs::rounds is 0 and the round count is agreed in round 0 (AlltoAllV)
};
static_assert(sizeof(IpcA2aArgs) == 536, "k_ipc_a2a's second argument: 512 B of tables and three words");
static_assert(sizeof(IpcArgs) + sizeof(IpcA2aArgs) <= 3072, "kernel arguments of k_ipc_a2a stay well below 4 KiB");

// The second argument of k_ipc_p2p (ipc_k_p2p.hip): the lanes of one launch and their items, by value, so a captured
// launch carries them. A lane is one (direction, peer) pair, owned by one blockIdx.y; its items run in order. Of
// IpcArgs the kernel takes only what concerns no collective: status word 0 (the sticky bit), failHost, timeoutTicks,
// fence, nt, threads and trace.
struct IpcP2pLane {
    char* mine;      // the area of the rank whose lane this is: it polls the flag words there, a receiver reads its slots
    char* peer;      // the peer's area as this rank maps it: every access to it is a store (slots or flag words)
    uint32_t* ctr;   // that rank's private counters: sent[n][kP2pBlocks], then rcvd[n][kP2pBlocks]
    uint8_t isSend;
    uint8_t me;      // the lane's rank (rank mode: this rank; a loopback world's launch holds both roles)
    uint8_t peerRank;
    uint8_t first;   // items [first, first + num) of IpcP2pArgs::item
    uint32_t num;
};
struct IpcP2pItem {
    void* buf;
    uint64_t count;
};
struct IpcP2pArgs {
    IpcP2pLane lane[kP2pMaxLanes];
    IpcP2pItem item[kP2pMaxItems];
    uint64_t slotBytes;
    uint64_t slotElems;
    uint64_t blockElems;
};
static_assert(sizeof(IpcP2pLane) == 32 && sizeof(IpcP2pArgs) == 32 * kP2pMaxLanes + 16 * kP2pMaxItems + 24, "k_ipc_p2p");
static_assert(sizeof(IpcArgs) + sizeof(IpcP2pArgs) <= 4096, "kernel arguments of k_ipc_p2p fit the 4 KiB segment");

// The argument of k_ipc_check (ipc_k_check.hip), the cross-rank argument check ahead of a collective. It shares no
// word with the collectives but the sticky status bit and the failure word. Rank mode (me >= 0) uses rec[me], priv[me]
// and status[me]; a loopback world's one launch holds every rank's (blockIdx.y is the rank). The records travel by
// value: kIpcMaxRanks of them are 704 bytes, so a world's launch needs no table ring, and a captured launch carries
// its record.
struct IpcCheckArgs {
    uint64_t* area[kIpcMaxRanks];    // every rank's check area (ipc_plan.h kCheckAreaBytes) as the launch addresses it
    uint64_t* priv[kIpcMaxRanks];    // the ranks' private words (CheckPrivWord)
    uint32_t* status[kIpcMaxRanks];  // the ranks' status words (IpcArgs::status): bits 0 and 1 of word 0 on a difference
    uint32_t* sticky;                // the status word 0 the communicator's launches test: of the rank that issues them
    uint32_t* failHost;              // IpcArgs::failHost: 1 = a wait passed its bound, 2 = inconsistent arguments
    uint64_t timeoutTicks;
    uint32_t n;
    int32_t me;
    CheckRecord rec[kIpcMaxRanks];
};
static_assert(sizeof(IpcCheckArgs) <= 2048, "kernel arguments of k_ipc_check");

constexpr uint32_t kIpcA2aRingSlots = 8;  // all-to-all launches of a loopback world in flight (IpcState::a2aRing)

// Phase stamps of one block (HCCL_AMD_IPC_TRACE, HcclAmdCommIpcTrace): 100 MHz s_memrealtime ticks, lane 0 of the
// block. The round stamps are those of the launch's last round. "issued" = lane 0's wave has issued the phase's last
// access (a barrier's own drain counts toward the barrier).
enum IpcTraceSlot : uint32_t {
    kTrEntry = 0,       // kernel entry (after the failed-communicator check)
    kTrRound = 1,       // start of the round
    kTrPhase0 = 2,      // phase 0 issued
    kTrBarrier1 = 3,    // first barrier passed
    kTrPhase1 = 4,      // phase 1 issued
    kTrBarrier2 = 5,    // second barrier passed (two-barrier kinds)
    kTrPhase2 = 6,      // phase 2 issued
    kTrExit = 7,        // lane 0's stores drained, before the launch's end count
    kIpcTraceSlots = 8,
};

// a2a: the second argument of kind kIpcAllToAll (required for it, unused otherwise).
HcclResult LaunchIpcCollective(const IpcArgs& a, uint32_t blocks, uint32_t worldRanks, HcclDataType dt,
                              HcclReduceOp op, hipStream_t stream, const IpcA2aArgs* a2a = nullptr);

// Per-dtype entry points of the kernels (ipc_k_*.hip, one translation unit per dtype group): the launch by op, and the
// kernel's address for the occupancy query (rhd: the kIpcRhd instantiation; ll: the LL kernel).
#define HCCL_AMD_IPC_DTYPE_DECL(NAME)                                                          \
    hipError_t LaunchIpc_##NAME(int op, const IpcArgs& a, dim3 grid, hipStream_t s); \
    const void* IpcKernel_##NAME(int op, bool rhd, bool ll);
HCCL_AMD_IPC_DTYPE_DECL(Int8)
HCCL_AMD_IPC_DTYPE_DECL(Int16)
HCCL_AMD_IPC_DTYPE_DECL(Int32)
HCCL_AMD_IPC_DTYPE_DECL(Int64)
HCCL_AMD_IPC_DTYPE_DECL(Uint64)
HCCL_AMD_IPC_DTYPE_DECL(Fp16)
HCCL_AMD_IPC_DTYPE_DECL(Bf16)
HCCL_AMD_IPC_DTYPE_DECL(Fp32)
HCCL_AMD_IPC_DTYPE_DECL(Fp64)
#undef HCCL_AMD_IPC_DTYPE_DECL

// The Broadcast's kernel (ipc_k_bcast.hip; kinds kIpcBroadcast and kIpcBroadcastOneShot): it moves data only, so it is
// instantiated per element size (1, 2, 4, 8 bytes), not per dtype and op. LaunchIpcCollective sends those kinds there.
hipError_t LaunchIpcBcast(uint32_t elemSize, const IpcArgs& a, dim3 grid, hipStream_t s);
const void* IpcBcastKernel(uint32_t elemSize);
// IpcResidentBlocks for that kernel (its own occupancy).
uint32_t IpcBcastResidentBlocks(uint32_t elemSize, uint32_t threads);

// The all-to-all's kernel (ipc_k_a2a.hip; kind kIpcAllToAll), typeless like the Broadcast's, and its occupancy.
hipError_t LaunchIpcA2a(uint32_t elemSize, const IpcArgs& a, const IpcA2aArgs& x, dim3 grid, hipStream_t s);
const void* IpcA2aKernel(uint32_t elemSize);
uint32_t IpcA2aResidentBlocks(uint32_t elemSize, uint32_t threads);

// Scatter's and AllGatherV's kernel (ipc_k_sg.hip; kinds kIpcScatter and kIpcAllGatherV), typeless too, and its
// occupancy.
hipError_t LaunchIpcSg(uint32_t elemSize, const IpcArgs& a, dim3 grid, hipStream_t s);
const void* IpcSgKernel(uint32_t elemSize);
uint32_t IpcSgResidentBlocks(uint32_t elemSize, uint32_t threads);

// The barrier's kernel (ipc_k_barrier.hip; kind kIpcBarrier): one workgroup of one wave per rank (worldRanks of them in a
// loopback world's launch, else one), so no launch cap applies and it has no occupancy query.
hipError_t LaunchIpcBarrier(const IpcArgs& a, uint32_t worldRanks, hipStream_t s);

// The argument check's kernel (ipc_k_check.hip), launched like the barrier's.
hipError_t LaunchIpcCheck(const IpcCheckArgs& a, uint32_t worldRanks, hipStream_t s);

// The point-to-point kernel (ipc_k_p2p.hip), typeless too, and its occupancy. grid = (kP2pBlocks, lanes).
hipError_t LaunchIpcP2p(uint32_t elemSize, const IpcArgs& a, const IpcP2pArgs& x, dim3 grid, hipStream_t s);
const void* IpcP2pKernel(uint32_t elemSize);
uint32_t IpcP2pResidentBlocks(uint32_t elemSize, uint32_t threads);

// Workgroups of the IPC kernel for (dt, op) that the device holds at once (occupancy x CUs; 0 if unknown). Every
// block of a launch waits at barriers for its peers' blocks, so the blocks that share a device must all be resident.
uint32_t IpcResidentBlocks(HcclDataType dt, HcclReduceOp op, bool rhd, bool ll, uint32_t threads);

// Writes back and invalidates every XCD's L2 at system scope (one maintenance block per CU); synchronous on `stream`.
HcclResult ScrubL2(hipStream_t stream);

// One staging tier of a communicator (ipc_plan.h describes the two tiers).
struct IpcTier {
    bool ready = false;
    bool unavailable = false;  // its set-up failed on some rank: calls that need it report NOT_SUPPORT
    void* area[kIpcAreas] = {};  // own areas, parts of one uncached allocation at area[0]
    void* peerArea[kIpcAreas][kIpcMaxRanks] = {};
    bool opened[kIpcMaxRanks] = {};  // rank mode: the peer's allocation was opened with hipIpcOpenMemHandle
    IpcTierBytes size;  // of the areas (IpcTierSizes)
};

// Per-communicator state of the IPC path. `ready` covers what every call needs: the flags and LL area (one uncached
// allocation mapped by every peer), the status words, the failure word and the LL unpack area.
struct IpcState {
    bool ready = false;
    bool unavailable = false;      // set-up failed on some rank: every later call reports NOT_SUPPORT
    uint32_t* flags = nullptr;     // own flags, uncached, zeroed
    uint32_t* status = nullptr;    // device words: [0] bit 0 = barrier timeout, [2..3] = tagged longest wait (IpcArgs)
    uint32_t callSeq = 0;          // IPC calls issued on the communicator (tags the wait diagnostic)
    uint32_t* failHost = nullptr;  // pinned host word the kernel sets on a barrier timeout (hipHostMalloc, coherent)
    uint32_t* failDev = nullptr;   // the device address the launches write (IpcArgs::failHost): of failHost, or in a
                                   // loopback world of the world's word (Transport::SharedFailWord)
    uint32_t* peerFlags[kIpcMaxRanks] = {};
    bool flagsOpened[kIpcMaxRanks] = {};
    IpcTier tier[kIpcTiers];
    uint32_t blocks = 0;
    uint32_t ranksOnDevice = 1;    // rank mode: the most ranks that share one device (by PCI bus id), same on all ranks
    uint64_t* trace = nullptr;     // HCCL_AMD_IPC_TRACE=1 at set-up: [kIpcMaxRanks][kIpcMaxBlocks][kIpcTraceSlots]
    void* llUnpack = nullptr;      // own unpack area of the LL path (cached, kIpcLlUnpackBytes)
    // Loopback world, on the rank that issues the world's launches: every rank's all-to-all tables for the launches in
    // flight. kIpcA2aRingSlots slots of kIpcMaxRanks tables, pinned host memory and its device twin; a slot is filled
    // on the host, copied on the launch's stream and reused only once the launch that read it has ended (its event).
    struct A2aRing {
        IpcA2aTables* host = nullptr;
        IpcA2aTables* dev = nullptr;
        hipEvent_t used[kIpcA2aRingSlots] = {};
        bool recorded[kIpcA2aRingSlots] = {};
        uint32_t next = 0;
    } a2aRing;
    // The point-to-point path (HcclAmdCommEnableP2p): one more uncached allocation mapped by every peer (ipc_plan.h
    // has its layout) and the private counters. In a loopback world, whose one launch per message holds both roles,
    // the ranks know each other's counters too.
    struct P2p {
        bool ready = false;
        bool unavailable = false;  // its set-up failed on some rank: the operators keep the transport path
        void* area = nullptr;
        void* peerArea[kIpcMaxRanks] = {};
        bool opened[kIpcMaxRanks] = {};
        uint32_t* counters = nullptr;
        uint32_t* peerCounters[kIpcMaxRanks] = {};  // loopback world only
        uint64_t slotBytes = 0;
        uint64_t areaBytes = 0;
        uint64_t counterBytes = 0;
    } p2p;
    // The cross-rank argument check (CommConfig::inconsistentCheck): one more uncached allocation mapped by every peer
    // (kCheckAreaBytes) and the private words (kCheckPrivBytes), set up collectively by the first checked call. In a
    // loopback world, whose one launch holds every rank, the ranks know each other's private and status words too.
    struct Check {
        bool ready = false;
        bool unavailable = false;  // its set-up failed on some rank: calls run unchecked
        bool logged = false;       // the one line about unchecked calls has been written
        void* area = nullptr;
        void* peerArea[kIpcMaxRanks] = {};
        bool opened[kIpcMaxRanks] = {};
        uint64_t* priv = nullptr;
        uint64_t* peerPriv[kIpcMaxRanks] = {};    // loopback world only
        uint32_t* peerStatus[kIpcMaxRanks] = {};  // loopback world only
        uint32_t seenOps = 0;      // `first` mode: bit k = an operator of record type k has been checked
        bool reported = false;     // the report's line has been logged
    } check;
};

constexpr size_t kIpcStatusBytes = 32;  // status words (IpcArgs::status)
constexpr int kIpcEpochWord = 4;
constexpr int kIpcDoneWord = 5;
constexpr int kIpcLlSeqWord = 6;  // LL launches so far (each advances it by one; the flag of launch s is s + 1)
// Flag words of a rank: [kIpcMaxBlocks][kIpcMaxRanks], at the start of its flag allocation.
constexpr uint64_t kIpcFlagBytes = uint64_t(kIpcMaxBlocks) * kIpcMaxRanks * sizeof(uint32_t);
// LL area (HCCL_AMD_IPC_LL_BYTES): behind the flags in the same uncached allocation (one IPC handle), two parities of
// kIpcMaxRanks source slots; a slot holds a call's input as 8-byte words {4 data bytes, 32-bit flag}, so twice the
// bytes of the largest LL call. The unpack area (own, cached) holds the n operands in the fold's slot layout.
constexpr uint64_t kIpcLlSlotBytes = 2 * kIpcLlMaxBytes;
constexpr uint64_t kIpcLlParityBytes = uint64_t(kIpcMaxRanks) * kIpcLlSlotBytes;
constexpr uint64_t kIpcLlUnpackBytes = uint64_t(kIpcMaxRanks) * (kIpcLlMaxBytes + 256);

}  // namespace hccl_amd
