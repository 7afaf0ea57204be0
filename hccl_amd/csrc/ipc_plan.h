// ipc_plan.h — the host-side arithmetic of the one-sided collectives: which kind, order and chunk layout a call takes,
// its form (LL or staged), workgroups, executor loops and the launch geometry of each loop. Host-only integer logic,
// like schedule.h: no HIP, no communicator, so the CPU layout models and the sanitizer sweep (tests/test_ipc_layout.py,
// tests/sanitize/ipc_plan_sweep.cc) run the very code RunIpcPlan (ipc.cc) runs.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/hccl_amd.h"

// SingleBarrierKind is asked by the kernel too: device-callable where the HIP headers came first (ipc.h).
#if defined(__host__) && defined(__device__)
#define HCCL_AMD_IPC_HD __host__ __device__
#else
#define HCCL_AMD_IPC_HD
#endif

namespace hccl_amd {

constexpr int kIpcMaxRanks = HCCL_AMD_IPC_MAX_RANKS;

enum IpcKind : uint32_t {
    kIpcAllReduce = 0,         // two-shot: owner c folds chunk c, every rank gets every chunk
    kIpcReduceScatter = 1,     // owner c folds block c into its recvBuf
    kIpcReduce = 2,            // two-shot Reduce: owner c folds chunk c, only the root gets the result
    kIpcAllReduceOneShot = 3,  // every rank receives every peer's whole piece and folds all of it (no phase 2)
    kIpcReduceOneShot = 4,     // the peers push their whole piece to the root, which folds it
    kIpcAllGather = 5,         // every rank pushes its whole piece to every peer; each copies the n pieces out
    // The Broadcast's kinds run in a kernel of their own (k_ipc_bcast, ipc_k_bcast.hip), never in k_ipc_collective.
    kIpcBroadcast = 6,         // two-shot: the root scatters chunk c (and its own) to rank c, the others exchange theirs
    kIpcBroadcastOneShot = 7,  // the root pushes its whole piece to every peer; each copies it out (one barrier)
    // The all-to-all family runs in a kernel of its own too (k_ipc_a2a, ipc_k_a2a.hip).
    kIpcAllToAll = 8,          // every rank pushes pair (me, q) into slot `me` of peer q; each copies its n slots out
    // Scatter and AllGatherV share a third typeless kernel (k_ipc_sg, ipc_k_sg.hip).
    kIpcScatter = 9,           // the root pushes block c into the one slot of rank c's area; rank c copies it out
    kIpcAllGatherV = 10,       // every rank pushes its block into slot `me` of every peer; each copies the n - 1 slots
                               // out to the blocks' displacements (kIpcGeomV: block q = vLen[q] elements at vStart[q])
    // The barrier is a fourth typeless kernel (k_ipc_barrier, ipc_k_barrier.hip).
    kIpcBarrier = 11,          // HcclBarrier: one workgroup per rank, one flag exchange, no staging and no user buffer
};

// IpcPlan::subMode of kIpcAllToAll: who knows the round count.
enum IpcA2aMode : uint32_t {
    kIpcA2aKnown = 0,   // AlltoAll / AlltoAllVC: every rank knows the whole count matrix, the host sets the rounds
    kIpcA2aAgreed = 1,  // AlltoAllV: a rank knows its own row and column only; the kernel agrees the rounds (rounds 0)
};
// kIpcA2aAgreed: the head of every slot holds one 32-bit word per workgroup, the sender's own round need; sized for
// kIpcMaxBlocks (512) whatever the launch's blocks, so that the slot capacity does not depend on them.
constexpr uint64_t kIpcA2aHeaderBytes = 2048;

// A Broadcast of at most this many bytes runs as kIpcBroadcastOneShot: one barrier instead of two, for n - 1 times the
// root's stores. Measured on one GPU (tools/probes/bcast_loopback.py, profiles/bcast_loopback_one_gpu.jsonl), the
// one-shot is ahead at every size up to the largest measured, 64 MiB, in the 8-rank loopback world (481.9 against
// 605.8 us there) and in the 2-process pair (65.0 against 80.5 us): no crossover lies inside the measured range, so the
// bound is that range's end and the two-shot takes what is larger. On one GPU the root's n - 1 copies cost HBM
// bandwidth only; over xGMI each of them occupies a link for the whole piece, where the two-shot sends 2/n of it, so
// the first multi-GPU run is expected to lower this.
constexpr uint64_t kIpcBcastOneShotMaxBytes = 64ull << 20;
// Operand order of a fold of chunk t.
enum IpcOrder : uint32_t {
    kIpcO2 = 0,  // x_0, x_1, .., x_{n-1}                          two-shot AllReduce; AIV one-shot, small-core
                 //                                                 two-shot, big-data ReduceScatter
    kIpcO1 = 1,  // x_t, then ascending q != t                      one-shot, mesh ReduceScatter, Reduce; AIV
                 //                                                 large-core two-shot
    kIpcO6 = 2,  // sub-slice j: x_t, then x_{t+o}, o = j+1..n-1, 1..j   MeshChunk AllReduce / ReduceScatter
    kIpcO4 = 3,  // pow-2 tree over the source ranks (rank-independent): M = largest power of two below n,
                 // x_j = x_{j+M} (op) x_j for j + M < n, then pairwise halving  AIV local-tree ReduceScatter
                 // (aiv_reduce_scatter_local_tree.h:138-172) = the STRICT order-preserved tree
    kIpcRhd = 4,  // one-shot kind only: the RHD AllReduce's bits (schedule.cc AllReduceRhd), per element the O4 tree
                  // over virtual ranks v ^ q of its RHD instance, v = the owner of its chunk (RhdFold)
};

// Chunk layout of one launch (input coordinates, elements; rank c owns chunk c).
enum IpcGeom : uint32_t {
    kIpcGeomAlignedCeil = 0,  // ceil(cnt / n) rounded up to 128 B (two-shot AllReduce, CalcSliceInfo)
    kIpcGeomCeil = 1,         // ceil(cnt / n), no alignment (MeshChunk CalcSliceInfoVec; AIV small-core two-shot)
    kIpcGeomBalanced = 2,     // g * n balanced slices (the first cnt % (g*n) one longer), chunk c = slices
                              // [c*g, (c+1)*g): Reduce two-shot (g = 1, reduce_mesh_1D_two_shot.cc:108-131) and
                              // the AIV large-core two-shot (g = groupSize, aiv_all_reduce_mesh_1d_twoshot.h:21-58)
    kIpcGeomBlock = 3,        // ReduceScatter: chunk c = input block c (reduce_scatter_op.cc:158-159)
    kIpcGeomWhole = 4,        // one-shot kinds and AllGather: every chunk is the whole range
    kIpcGeomV = 5,            // ReduceScatterV: chunk c = counts[c] elements at displs[c] (per-rank, any alignment)
};

// Everything that decides a one-sided call's bits: the kind, the fold order, the chunk layout and the executor loop
// that the layout is applied to (the reference slices every loop on its own).
struct IpcPlan {
    uint32_t kind;       // IpcKind
    uint32_t order;      // IpcOrder
    uint32_t geom;       // IpcGeom
    uint32_t group = 1;  // kIpcGeomBalanced: slices per chunk
    uint32_t subMode = 0;  // IpcSubMode (kIpcO6)
    uint64_t loopElems = 0;  // elements per executor loop (per block for ReduceScatter); 0 = one loop
};

// Sub-slices of a chunk for kIpcO6 (chunk coordinates): the MeshChunk AllReduce's even split (the first L % (n-1)
// one longer) or the MeshChunk ReduceScatter's 4-KiB split (schedule.cc SubSlicesEven / SubSlicesRs).
enum IpcSubMode : uint32_t {
    kIpcSubEven = 0,
    kIpcSubRs4K = 1,
};

// Kinds whose fold reads only slots and writes only the rank's own output (no result push, no phase 2). They need
// one barrier per round: their slots alternate between two areas that no other kind touches, so the next round's
// stores never meet this round's fold (k_ipc_collective). The others keep two (results must be complete before phase 2).
HCCL_AMD_IPC_HD constexpr bool SingleBarrierKind(uint32_t kind)
{
    return kind == kIpcReduceScatter || kind == kIpcAllReduceOneShot || kind == kIpcReduceOneShot ||
           kind == kIpcAllGather;
}

// The same question on the host side, where the Broadcast's kinds appear too: its one-shot kind keeps one barrier and
// the alternate areas like the others. (k_ipc_collective never sees a Broadcast kind, so its own test stays as it is.)
constexpr bool HostSingleBarrierKind(uint32_t kind)
{
    return SingleBarrierKind(kind) || kind == kIpcBroadcastOneShot || kind == kIpcAllToAll || kind == kIpcScatter ||
           kind == kIpcAllGatherV;
}

constexpr uint32_t kIpcBlocks = 128;     // workgroups per rank and launch in a loopback world (cap)
constexpr uint32_t kIpcMaxBlocks = 512;  // flags are sized for this many (HcclAmdCommSetIpcBlocks)
// The largest call of the LL form (HCCL_AMD_IPC_LL_BYTES' bound; the LL area is sized for it, ipc.h).
constexpr uint64_t kIpcLlMaxBytes = 64ull << 10;
// The staging allocation of a rank (slot, result and two alternate areas) stays below 2 GiB: hipIpcOpenMemHandle never
// returned for a 2 GiB allocation on this stack (IpcSetupTier). The area size is CommConfig::ipcStagingBytes.
constexpr uint64_t kIpcStagingMaxBytes = 2047ull << 20;
// One staging area (HCCL_AMD_IPC_STAGING_MIB's range, and the cap of HCCL_BUFFSIZE / 2): two such areas leave the
// alternate areas 23.5 MiB each within kIpcStagingMaxBytes.
constexpr uint64_t kIpcStagingAreaMaxBytes = 1000ull << 20;

// Staging of the one-sided kernel comes in two tiers, each one uncached allocation per rank holding the four areas
// (kIpcAreaIn, kIpcAreaRes, kIpcAreaAlt0, kIpcAreaAlt1), mapped by every peer, and each set up collectively by the
// first call that needs it:
//   kIpcTierSmall — areas of n x HCCL_AMD_SMALL_IPC_BYTES (at least n x 64 KiB): every call whose staging fits one
//                   round there (the small-call rule's calls and any other small one-sided call);
//   kIpcTierLarge — areas of HCCL_BUFFSIZE / 2, so the four hold 2 x HCCL_BUFFSIZE, the reference's CCL buffer pair
//                   (HCCL_BUFFSIZE.md; aiv_defines.h:44), unless HCCL_AMD_IPC_STAGING_MIB sets the area size.
// A communicator that only makes small calls therefore holds MiBs, not the large tier.
constexpr int kIpcTierSmall = 0;
constexpr int kIpcTierLarge = 1;
constexpr int kIpcTiers = 2;

struct IpcTierBytes {
    uint64_t inBytes = 0;
    uint64_t resBytes = 0;
    uint64_t altBytes = 0;  // each of the two alternate slot areas of the single-barrier kinds
    uint64_t allocBytes() const { return inBytes + resBytes + 2 * altBytes; }
};

// The area sizes of staging tier t for nRanks ranks: a function of the rank count, HCCL_BUFFSIZE (cclBytes) and the
// (=) configuration (CommConfig::ipcStagingBytes, smallIpcBytes), so equal on every rank.
IpcTierBytes IpcTierSizes(uint32_t nRanks, uint64_t cclBytes, uint64_t ipcStagingBytes, uint64_t smallIpcBytes, int t);

// ---- plans: what a call's operation and family (or AIV variant) make of the kernel
HcclResult IpcPlanRhd(uint32_t n, IpcPlan* pl);
// n >= 2 (it divides by n - 1; a one-rank call never gets here).
HcclResult IpcPlanForFamily(int32_t opType, int32_t family, uint32_t n, uint64_t es, uint64_t cclBytes, IpcPlan* pl);
// The one-sided Broadcast's plan: kIpcBroadcastOneShot up to kIpcBcastOneShotMaxBytes and kIpcBroadcast above it
// (bcastKind 0), or the kind Comm::bcastKind fixes (1 = two-shot, 2 = one-shot).
IpcPlan IpcPlanBroadcast(uint64_t count, uint64_t es, int32_t bcastKind);
// The one-sided all-to-all's plan. agreed = false (AlltoAll, AlltoAllVC): IpcCall::count is the largest entry of the
// count matrix, which every rank knows, and the call is planned from n x count x es like the other kinds. agreed = true
// (AlltoAllV): no rank knows another's counts, so nothing the host decides may depend on them: the small staging tier
// (the large one only if the small one's set-up failed, which the ranks agree on), workgroups from the tier's
// capacity, never the LL form, and rounds = 0: the kernel agrees the round count in its first round.
IpcPlan IpcPlanAllToAll(bool agreed);
// The one-sided Scatter's plan (IpcCall::count = recvCount; block c of the root's input is chunk c, kIpcGeomBlock) and
// the one-sided AllGatherV's (kIpcGeomV over recvCounts / recvDispls, which every rank knows: the host sets the rounds
// from the largest block). One launch each: the rounds cover any count.
IpcPlan IpcPlanScatter();
IpcPlan IpcPlanAllGatherV();
// The one-sided barrier's plan (HCCL_AMD_OP_BARRIER, IpcCall::count = 0): one launch of one workgroup per rank, one
// round of one barrier epoch and no data, so every length of its geometry is 0 and it needs no staging tier.
IpcPlan IpcPlanBarrier();

// The reference's AIV engine (HCCL_OP_EXPANSION_MODE=AIV): SelectAivAlgo's rules and the variant its kernel takes
// for the vector-core count `coreLimit` (aivCoreLimit / the device's vector cores). es = dt's element size. Returns
// the variant (HcclAmdAivVariant, include/hccl_amd.h), HCCL_AMD_AIV_NOT_MATCHED when the selector would fall back to
// the AICPU engine; *plan receives the one-sided kernel's plan for a matched variant.
int32_t SelectAivPlan(int32_t opType, uint32_t n, uint64_t count, HcclDataType dt, uint64_t es, HcclReduceOp op,
                      bool strict, bool aivOnly, uint64_t cclBytes, uint32_t coreLimit, IpcPlan* plan, uint32_t* group);

uint32_t DefaultIpcBlocks(uint64_t bytes);  // workgroups per launch when the communicator sets none
uint32_t LlIpcBlocks(uint32_t n, uint64_t bytes, bool rhd);  // the same for a launch in the LL form

// ---- launch geometry: the four decisions of a call, in the order RunIpcPlan makes them. Every rank passes the same
// arguments (the call's, and the (=) configuration), so every rank decides alike.

// The call: its plan and the operator's arguments, after the AllGather's dtype remapping (es <= 8).
struct IpcCall {
    int32_t opType;
    IpcPlan plan;
    uint64_t count;
    const uint64_t* vCounts = nullptr;  // kIpcGeomV: every rank's block (n entries each)
    const uint64_t* vDispls = nullptr;
};

// Where it runs.
struct IpcEnv {
    uint32_t n;                    // ranks, 2 .. kIpcMaxRanks
    uint64_t es;                   // element size: 1, 2, 4 or 8 (16-B vectors of V = 16 / es elements)
    bool sharedDevice = false;     // loopback world: one launch on one device holds every rank's blocks
    uint32_t blocksOverride = 0;   // Comm::ipcBlocks, 0 = the default rules
    uint32_t residentPerRank = 0;  // blocks of the call's kernel the device holds at once, per rank on it; 0 = unknown
    uint64_t tileBytes = 0;        // CommConfig::ipcTileBytes (0 = one window per block)
    uint64_t llBytes = 0;          // CommConfig::ipcLlBytes
    uint64_t a2aAreaBytes = 0;     // kIpcA2aAgreed: one alternate area of the tier the call runs in (sizes its blocks)
};

using IpcGeometry = HcclAmdIpcGeometry;  // what one launch's IpcArgs take (ipc.h describes the fields)

struct IpcLoop {
    uint64_t off, cnt;
};

// 1. The LL form (HCCL_AMD_IPC_LL_BYTES; LlOneShot): a one-shot AllReduce of at most that many bytes per rank (and
// kIpcLlMaxBytes), one launch of one round. The ReduceScatter takes it too (equal blocks of `count`, each at most that
// many bytes): like the one-shot, every rank receives from every peer in every launch.
bool IpcUseLl(const IpcCall& call, const IpcEnv& env);

// 2. Workgroups per rank (block b pairs with block b of each peer): the override, or LlIpcBlocks / DefaultIpcBlocks by
// the call's bytes; a loopback world keeps at most kIpcBlocks per rank unless overridden. Then the co-residency cap:
// every block waits at barriers for its peers' blocks, so all blocks on a device must be resident at once. With
// env.residentPerRank == 0 this is the count before the cap (the residency depends on the kernel, so on `ll`).
uint32_t IpcBlockCount(const IpcCall& call, const IpcEnv& env, bool ll);

// 3. One launch per executor loop [off, off + cnt) of the reference template whose order the fold follows: its
// slicing is per loop (schedule.cc RefLoopElems and the MeshChunk loops). A ReduceScatter loop takes elements
// [off, off + cnt) of every block. kIpcGeomV: one launch on every rank, whatever this rank's own block.
std::vector<IpcLoop> IpcLoops(const IpcCall& call);

// Slot capacity in elements for areas of these sizes: a round's piece of every chunk must fit n slots of an area (the
// one-shot Broadcast and the Scatter fill one slot per area: a receiver has one sender); the single-barrier kinds' slots
// lie in the alternate areas.
uint64_t IpcSlotCap(uint32_t kind, const IpcEnv& env, const IpcTierBytes& areas);

// 4. The geometry of one loop of cnt elements for a slot capacity and block count. `ll` is the call's decision; the
// geometry keeps it only for a launch of one round.
IpcGeometry IpcLoopGeometry(const IpcCall& call, const IpcEnv& env, uint64_t cnt, uint64_t slotCap, uint32_t blocks,
                            bool ll);

// The whole sequence for a caller that knows the residency and the area sizes up front (HcclAmdIpcPlan and the
// sanitizer sweep; RunIpcPlan asks the device and sets up the tier in between). es = the element size of q.dataType;
// with q.areaBytes == q.altBytes == 0 the tier is chosen as RunIpcPlan chooses it, from IpcTierSizes of the last three
// arguments. Validates q (HCCL_E_PARA) before any plan is made.
HcclResult IpcPlanQuery(const HcclAmdIpcPlanQuery& q, uint64_t es, uint64_t cclBytes, uint64_t ipcStagingBytes,
                        uint64_t smallIpcBytes, HcclAmdIpcPlanResult* res, std::vector<IpcGeometry>* launches);

// ---- point-to-point (k_ipc_p2p, ipc_k_p2p.hip): HcclSend / HcclRecv / HcclBatchSendRecv over a p2p area of their own.
// A rank's area holds, for every source rank p, kP2pSlots data slots of slotBytes, then the flag words filled[p][b]
// (stored by sender p) and drained[q][b] (stored by receiver q: the credit for this rank's sends to q), one per
// workgroup b < kP2pBlocks. A message of `count` elements travels in pieces of slotElems = slotBytes / es elements;
// workgroup b moves the window [b * blockElems, (b + 1) * blockElems) of every piece, clipped to the piece. Both ends
// derive all of it from (count, es, slotBytes) alone.
constexpr uint32_t kP2pSlots = 2;
constexpr uint32_t kP2pBlocks = 4;   // workgroups per lane: fixed, so both ends of any message agree without a word
constexpr uint32_t kP2pMaxLanes = 2 * HCCL_AMD_IPC_MAX_RANKS;  // (direction, peer) pairs of one launch
constexpr uint32_t kP2pMaxItems = 32;                          // remote items of one launch (kernel arguments)
constexpr uint64_t kP2pSlotBytesDefault = 256ull << 10;  // HCCL_AMD_P2P_SLOT_BYTES: a design default, not measured
constexpr uint64_t kP2pSlotBytesMin = 128, kP2pSlotBytesMax = 16ull << 20;  // a multiple of 128 in this range

using P2pPlan = HcclAmdP2pPlanResult;
// The plan of one message, and the layout of an n-rank area. HCCL_E_PARA for an element size other than 1, 2, 4, 8, a
// slot size outside the range above or no multiple of 128, or n outside 1 .. kIpcMaxRanks.
HcclResult P2pPlanFor(uint64_t count, uint64_t es, uint64_t slotBytes, uint32_t n, P2pPlan* plan);
// Byte offsets inside an area of the plan's layout.
constexpr uint64_t P2pSlotOffset(uint64_t slotBytes, uint32_t src, uint32_t slot)
{
    return (uint64_t(src) * kP2pSlots + slot) * slotBytes;
}
constexpr uint64_t P2pFilledOffset(uint64_t slotBytes, uint32_t n, uint32_t src, uint32_t b)
{
    return uint64_t(n) * kP2pSlots * slotBytes + (uint64_t(src) * kP2pBlocks + b) * sizeof(uint32_t);
}
constexpr uint64_t P2pDrainedOffset(uint64_t slotBytes, uint32_t n, uint32_t dst, uint32_t b)
{
    return P2pFilledOffset(slotBytes, n, n, 0) + (uint64_t(dst) * kP2pBlocks + b) * sizeof(uint32_t);
}

// HcclBatchSendRecv's list handling (ins_v2_batch_send_recv_executor.cc:106-208): drops the items of count 0, orders
// the sends and the receives as the reference does and pairs the self items. order (itemNum entries) receives indices
// into items: the remote sends, the remote receives, then the self pairs as (send, receive). HCCL_E_PTR for a kept
// item without a buffer, HCCL_E_PARA for a type that is neither send nor receive, an unmatched self item or a self pair
// whose counts or element sizes differ.
HcclResult BatchSendRecvOrder(const HcclSendRecvItem* items, uint32_t itemNum, uint32_t rank, uint32_t rankSize,
                              uint32_t* order, uint32_t* numSends, uint32_t* numRecvs, uint32_t* numSelfPairs);

// ---- the cross-rank argument check (k_ipc_check, ipc_k_check.hip): the call record every rank publishes ahead of a
// checked collective, the reference's OpExchangeInfo (alg_param.h:751; FillOpExchangeInfo and
// FillOpExchangeInfoWithDataDes, op_common.cc:1259-1322) without its group and tag strings: one communicator is one
// group, and calls match in order. A fixed layout of 32-bit words (include/hccl_amd.h has the fields); a 64-bit field
// takes two words, low word first.
constexpr uint32_t kCheckWords = HCCL_AMD_CHECK_WORDS;
using CheckRecord = HcclAmdCheckRecordWords;
constexpr uint32_t kCheckNoRoot = 0xFFFFFFFFu;  // INVALID_VALUE_RANKID (hccl_common.h:37)
// The field (HcclAmdCheckField) word w belongs to: words 0-1 the buffer size, 7-8 the count, one word each otherwise.
// Ascending words are ascending fields, so the first differing word names the first differing field.
HCCL_AMD_IPC_HD constexpr uint32_t CheckFieldOfWord(uint32_t w)
{
    return w < 2 ? 0u : w < 7 ? w - 1 : w < 9 ? 6u : w - 2;
}
// The first word of field f; the two 64-bit fields continue in the next one.
HCCL_AMD_IPC_HD constexpr uint32_t CheckFirstWord(uint32_t f) { return f == 0 ? 0u : f < 6 ? f + 1 : f == 6 ? 7u : f + 2; }
HCCL_AMD_IPC_HD constexpr bool CheckWideField(uint32_t f) { return f == 0 || f == 6; }
static_assert(CheckFieldOfWord(kCheckWords - 1) == HCCL_AMD_CHECK_FIELDS - 1 && CheckFirstWord(8) == 10 &&
                  CheckFieldOfWord(8) == 6 && CheckFirstWord(6) == 7 && CheckFieldOfWord(6) == 5,
              "the record's layout");
// The check's area of a rank: two parities of kIpcMaxRanks records, each word as 8 bytes {word, sequence number}.
constexpr uint64_t kCheckRecordBytes = uint64_t(kCheckWords) * 8;
constexpr uint64_t kCheckAreaBytes = 2 * uint64_t(HCCL_AMD_IPC_MAX_RANKS) * kCheckRecordBytes;
// The check's private device words of a rank, 64-bit each: [0] the sequence counter (check launches so far), [1] 1 once
// a report is recorded, [2] the peer, [3] the field, [4] the local value, [5] the remote value.
enum CheckPrivWord : uint32_t { kCheckSeq = 0, kCheckHasReport = 1, kCheckPeer = 2, kCheckField = 3, kCheckLocal = 4,
                                kCheckRemote = 5, kCheckPrivWords = 6 };
constexpr uint64_t kCheckPrivBytes = uint64_t(kCheckPrivWords) * 8;
// Fills *rec for one call; opType is HcclAmdOpType or HCCL_AMD_CHECK_OP_ALLTOALLV / _VC. HCCL_E_PARA for an operator
// that is not checked.
HcclResult FillCheckRecord(int32_t opType, uint32_t root, HcclReduceOp op, HcclDataType dt, uint64_t count,
                           uint64_t bufferBytes, bool expansionAiv, bool strict, uint32_t aivCoreLimit,
                           CheckRecord* rec);
// Field f of a record as one 64-bit value.
uint64_t CheckFieldValue(const CheckRecord& rec, uint32_t field);

}  // namespace hccl_amd
