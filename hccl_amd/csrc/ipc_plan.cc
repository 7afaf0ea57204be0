// ipc_plan.cc — the one-sided collectives' plans and launch geometry (ipc_plan.h): pure functions of the call's
// arguments and the configuration, which every rank shares, so every rank decides alike.
#include "ipc_plan.h"

#include <algorithm>

#include "schedule.h"

namespace hccl_amd {

IpcTierBytes IpcTierSizes(uint32_t nRanks, uint64_t cclBytes, uint64_t ipcStagingBytes, uint64_t smallIpcBytes, int t)
{
    constexpr uint64_t kGranule = 64ull << 10;
    const auto up = [](uint64_t b) { return (b + kGranule - 1) / kGranule * kGranule; };
    // the large tier: HCCL_BUFFSIZE / 2 per area (2 x HCCL_BUFFSIZE for the four), or HCCL_AMD_IPC_STAGING_MIB
    uint64_t large = ipcStagingBytes != 0 ? ipcStagingBytes : cclBytes / 2 / kGranule * kGranule;
    large = std::min<uint64_t>(std::max<uint64_t>(large, 1ull << 20), kIpcStagingAreaMaxBytes);
    uint64_t area = large;
    if (t == kIpcTierSmall) {
        area = std::min(large, up(uint64_t(std::max<uint32_t>(nRanks, 1)) * std::max<uint64_t>(smallIpcBytes, 64ull << 10)));
    }
    IpcTierBytes s{};
    s.inBytes = area;
    s.resBytes = area;  // results of a whole round, in round coordinates
    // slots of the single-barrier kinds, two areas used alternately: as large as the others, within the one
    // allocation's bound (1000 MiB areas leave them 23.5 MiB)
    s.altBytes = std::min<uint64_t>(area, (kIpcStagingMaxBytes - 2 * area) / 2 / kGranule * kGranule);
    return s;
}

// Default workgroups per launch by the bytes of one rank's input. Every block runs its own cross-rank barrier (a
// system-scope release, one flag store per peer, a poll), so small calls pay per block: 16 blocks run a 1 KiB
// AllReduce in 11 us where 128 take 25 us and 256 take 42 us; large calls want the whole chip (1 GiB: 256 blocks
// 10 % ahead of 128). Rank-mode sweep on one GPU, n = 2 and 4 (tools/probes/sweep_ipc_blocks.py,
// profiles/r01_sweep_ipc_blocks.jsonl); the best count agreed between n = 2 and 4 at every size. Below 16 blocks (r05,
// profiles/r05_sweep_small_blocks.jsonl): up to 64 KiB, 4 blocks are 0.2-0.5 us faster than 16 at n = 2 (1 KiB
// 10.26 vs 10.71 us) and no slower at n = 4; from 256 KiB on, fewer than 16 lose bandwidth.
// Workgroups of an LL launch: about two polled words per thread, (n - 1) x bytes / 4 words over 256-thread blocks. A
// block's pull, unpack and fold are serial latencies, so the LL form wants many small blocks where the staged kernel
// wants few: rank mode, n = 2 and 4 on one GPU (tools/probes/sweep_ipc_blocks.py with HCCL_AMD_IPC_LL_BYTES,
// profiles/r05_ll_sweep_blocks.jsonl): 1 KiB best at 1-2 blocks (7.4 us), 64 KiB at 32 (9.4 us; 55.5 us with 1).
// RHD's order folds a tree per part and chunk, so its blocks want about one word per thread, and never fewer than two
// blocks (n = 2, eager: 1 KiB 14.5 us on one block, 13.4 on two; 4 KiB 13.2 on four; profiles/r05_ll_rhd_blocks.jsonl).
uint32_t LlIpcBlocks(uint32_t n, uint64_t bytes, bool rhd)
{
    const uint64_t items = uint64_t(n > 1 ? n - 1 : 1) * ((bytes + 3) / 4);
    const uint64_t per = rhd ? 256 : 512;
    return static_cast<uint32_t>(std::min<uint64_t>(128, std::max<uint64_t>(2, (items + per - 1) / per)));
}

uint32_t DefaultIpcBlocks(uint64_t bytes)
{
    if (bytes <= (64ull << 10)) return 4;
    if (bytes <= (512ull << 10)) return 16;
    if (bytes <= (2ull << 20)) return 32;
    if (bytes <= (32ull << 20)) return 64;
    if (bytes <= (64ull << 20)) return 128;
    return 256;
}

// ------------------------------------------------------------------------------------------------ plans

namespace {

uint64_t LoopElems(uint64_t loopBytes, uint64_t es) { return std::max<uint64_t>(1, loopBytes / es); }

uint64_t RoundDown128(uint64_t b) { return b / 128 * 128; }

constexpr uint64_t kUbMaxDataSize = 256ull << 20;  // UB_MAX_DATA_SIZE, alg_param.h:37

}  // namespace

// The AICPU template whose order the kernel follows, by schedule family (the auto selector's families).
HcclResult IpcPlanForFamily(int32_t opType, int32_t family, uint32_t n, uint64_t es, uint64_t cclBytes, IpcPlan* pl)
{
    IpcPlan p{};
    switch (opType) {
        case HCCL_AMD_OP_ALLREDUCE:
            if (family == HCCL_AMD_ALGO_MESH_ONESHOT) {
                p.kind = kIpcAllReduceOneShot;
                p.order = kIpcO1;
                p.geom = kIpcGeomWhole;
            } else if (family == HCCL_AMD_ALGO_MESH_CHUNK) {
                // MeshChunk CalcSliceInfoVec (…mesh_chunk.cc:79-97), loops of min(ccl, ccl / 2) rounded down to
                // 128 B (scratch multiple 2)
                p.kind = kIpcAllReduce;
                p.order = kIpcO6;
                p.geom = kIpcGeomCeil;
                p.loopElems = LoopElems(std::min<uint64_t>(cclBytes, RoundDown128(cclBytes / 2)), es);
            } else {
                p.kind = kIpcAllReduce;  // two-shot: O2 does not depend on the slicing or the loops
                p.order = kIpcO2;
                p.geom = kIpcGeomAlignedCeil;
            }
            break;
        case HCCL_AMD_OP_REDUCE_SCATTER:
            p.kind = kIpcReduceScatter;
            p.geom = kIpcGeomBlock;
            if (family == HCCL_AMD_ALGO_MESH_CHUNK) {
                // ReduceScatter MeshChunk: loops of min(ccl - 1 MiB, (ccl - 1 MiB) / (n-1)) rounded down to 128 B
                const uint64_t tmp = cclBytes > (1ull << 20) ? cclBytes - (1ull << 20) : cclBytes;
                p.order = kIpcO6;
                p.subMode = kIpcSubRs4K;
                p.loopElems = LoopElems(std::min<uint64_t>(tmp, RoundDown128(tmp / (n - 1))), es);
            } else {
                p.order = kIpcO1;
            }
            break;
        case HCCL_AMD_OP_REDUCE:
            p.order = kIpcO1;
            if (family == HCCL_AMD_ALGO_MESH_ONESHOT) {
                p.kind = kIpcReduceOneShot;
                p.geom = kIpcGeomWhole;
            } else {
                // ReduceSoleExecutor loops (reduce_sole_executor.cc:120-170): min(UB_MAX_DATA_SIZE, ccl / n) rounded
                // down to 128 B, each sliced by ReduceMesh1DTwoShot::CalcSlice on its own
                p.kind = kIpcReduce;
                p.geom = kIpcGeomBalanced;
                p.group = 1;
                p.loopElems = LoopElems(std::min<uint64_t>(kUbMaxDataSize, RoundDown128(cclBytes / n)), es);
            }
            break;
        case HCCL_AMD_OP_ALLGATHER:
            p.kind = kIpcAllGather;  // data movement only: no order
            p.order = kIpcO1;
            p.geom = kIpcGeomWhole;
            break;
        default: return HCCL_E_NOT_SUPPORT;
    }
    *pl = p;
    return HCCL_SUCCESS;
}

// RHD's bits on the one-sided kernel (HCCL_AMD_ALGO_IPC_RHD): the one-shot kind in order kIpcRhd over the whole
// range. AllReduceRhd has no executor loops (it is not a reference template), so neither does this: its slicing is
// a function of the count alone.
HcclResult IpcPlanRhd(uint32_t n, IpcPlan* pl)
{
    if (RhdTable(n).empty() || n < 2) return HCCL_E_NOT_SUPPORT;
    IpcPlan p{};
    p.kind = kIpcAllReduceOneShot;
    p.order = kIpcRhd;
    p.geom = kIpcGeomWhole;
    *pl = p;
    return HCCL_SUCCESS;
}

// The slicing of a Broadcast is unobservable: chunks of ceil(count / n) rounded up to 128 B keep every chunk start
// vector-aligned (kIpcGeomAlignedCeil); the one-shot kind has the whole range as its one "chunk". No executor
// loops: the rounds of one launch cover any count. The kind depends on the call's arguments alone (and on
// bcastKind, which a caller sets on every rank alike), so every rank takes the same one.
IpcPlan IpcPlanBroadcast(uint64_t count, uint64_t es, int32_t bcastKind)
{
    const bool oneShot = bcastKind == 0 ? count * es <= kIpcBcastOneShotMaxBytes : bcastKind == 2;
    IpcPlan plan{};
    plan.kind = oneShot ? kIpcBroadcastOneShot : kIpcBroadcast;
    plan.order = kIpcO1;  // no fold: unused
    plan.geom = oneShot ? kIpcGeomWhole : kIpcGeomAlignedCeil;
    return plan;
}

// The all-to-all moves data only and every pair has a slot of its own: one kind, no order, no executor loops (the
// rounds of one launch cover any count). subMode says who knows the round count (IpcA2aMode).
IpcPlan IpcPlanAllToAll(bool agreed)
{
    IpcPlan plan{};
    plan.kind = kIpcAllToAll;
    plan.order = kIpcO1;  // no fold: unused
    plan.geom = kIpcGeomWhole;
    plan.subMode = agreed ? kIpcA2aAgreed : kIpcA2aKnown;
    return plan;
}

// Scatter and AllGatherV move data only, like the two above: one kind each, no order, no executor loops.
IpcPlan IpcPlanScatter()
{
    IpcPlan plan{};
    plan.kind = kIpcScatter;
    plan.order = kIpcO1;  // no fold: unused
    plan.geom = kIpcGeomBlock;
    return plan;
}

IpcPlan IpcPlanAllGatherV()
{
    IpcPlan plan{};
    plan.kind = kIpcAllGatherV;
    plan.order = kIpcO1;  // no fold: unused
    plan.geom = kIpcGeomV;
    return plan;
}

IpcPlan IpcPlanBarrier()
{
    IpcPlan plan{};
    plan.kind = kIpcBarrier;
    plan.order = kIpcO1;  // no fold: unused
    plan.geom = kIpcGeomWhole;  // no data: unused
    return plan;
}

int32_t SelectAivPlan(int32_t opType, uint32_t n, uint64_t count, HcclDataType dt, uint64_t es, HcclReduceOp op,
                      bool strict, bool aivOnly, uint64_t cclBytes, uint32_t coreLimit, IpcPlan* plan, uint32_t* group)
{
    // Common rejections of AllReduceAutoSelector / ReduceScatterAutoSelector::SelectAivAlgo
    // (all_reduce_auto_selector.cc:591-683, reduce_scatter_auto_selector.cc:537-600): the order-preserved (STRICT)
    // mode, PROD, UINT64 / FP64 and more than MAX_RANK_SIZE ranks fall back to the AICPU engine; so does data of
    // AIV_MAX_PER_RANK_DATA_SIZE (8 MiB, auto_selector_base.h:24) x rankSize or more, or above 16 CCL buffers
    // (AIV_MAX_CCL_LOOP_NUM, hccl_aiv_utils.h:33). ReduceAutoSelector has no AIV selection: Reduce stays AICPU.
    // AIV_ONLY (OpExecuteConfig::AIV_ONLY) lifts the 8 MiB x rankSize bound, not the CCL one
    // (all_reduce_auto_selector.cc:650-661, reduce_scatter_auto_selector.cc:597-610).
    if (es == 0 || n < 2 || n > 512) return HCCL_AMD_AIV_NOT_MATCHED;
    if (opType != HCCL_AMD_OP_ALLREDUCE && opType != HCCL_AMD_OP_REDUCE_SCATTER) return HCCL_AMD_AIV_NOT_MATCHED;
    if (strict || op == HCCL_REDUCE_PROD || dt == HCCL_DATA_TYPE_UINT64 || dt == HCCL_DATA_TYPE_FP64) {
        return HCCL_AMD_AIV_NOT_MATCHED;
    }
    const uint64_t maxPerRank = 8ull << 20;
    IpcPlan p{};
    uint32_t g = 1;
    int32_t variant;
    if (opType == HCCL_AMD_OP_ALLREDUCE) {
        const uint64_t dataSize = count * es;
        if ((!aivOnly && dataSize >= maxPerRank * n) || dataSize > cclBytes * 16) return HCCL_AMD_AIV_NOT_MATCHED;
        // n <= AR_AIV_BOARD_SIZE (8): one-shot below AR_AIV_SMALL_DATA_SIZE_IN_BOARD (128 KiB); above 8 ranks
        // IsSmallData (< 512 KiB, auto_selector_base.cc:94)
        const bool oneShot = n <= 8 ? dataSize < (128ull << 10) : dataSize < (512ull << 10);
        if (oneShot) {
            // aiv_all_reduce_mesh_1d_oneshot.h:33-48: out = slot 0, then out (op)= slot r, r = 1 .. n-1 (O2);
            // executor loops of min(UB_MAX_DATA_SIZE, ccl / n) (scratch multiple n), which do not change O2
            variant = HCCL_AMD_AIV_AR_ONESHOT;
            p.kind = kIpcAllReduceOneShot;
            p.order = kIpcO2;
            p.geom = kIpcGeomWhole;
            p.loopElems = LoopElems(std::min<uint64_t>(kUbMaxDataSize, RoundDown128(cclBytes / n)), es);
        } else {
            // AivTempAllReduceMesh1DTwoShot::CalNumBlocks (aiv_temp_all_reduce_mesh_1D_twoshot.cc:88-100) and the
            // kernel's split (aiv_all_reduce_mesh_1d_twoshot.h:330-346): 2n blocks or more take Prepare/Process,
            // fewer the small-core path. Executor loops of min(UB_MAX_DATA_SIZE, ccl / 4) (scratch multiple 4).
            const uint32_t blocks = coreLimit >= n + 1 ? coreLimit / (n + 1) * (n + 1) : coreLimit;
            p.loopElems = LoopElems(std::min<uint64_t>(kUbMaxDataSize, RoundDown128(cclBytes / 4)), es);
            p.kind = kIpcAllReduce;
            if (blocks >= 2 * n) {
                // ReduceScatterLocalReduce (:145-181): groupSize = (blocks - n) / n consumer slices per rank, the
                // loop split into groupSize * n balanced slices, rank r owning slices [r * g, (r + 1) * g); each
                // is folded own copy first, then the other ranks ascending (O1)
                g = (blocks - n) / n;
                variant = HCCL_AMD_AIV_AR_TWOSHOT_LARGE;
                p.order = kIpcO1;
                p.geom = kIpcGeomBalanced;
                p.group = g;
            } else {
                // SmallCoreReduceScatter (:224-271): chunks of ceil(count / n); slot 0 (op)= slot i, i = 1 .. n-1 (O2)
                variant = HCCL_AMD_AIV_AR_TWOSHOT_SMALL;
                p.order = kIpcO2;
                p.geom = kIpcGeomCeil;
            }
        }
    } else {
        const uint64_t totalSize = count * es * n;
        if ((!aivOnly && totalSize >= maxPerRank * n) || totalSize > cclBytes * 16) return HCCL_AMD_AIV_NOT_MATCHED;
        // AivTempReduceScatterMesh1D::CalNumBlocks (aiv_temp_reduce_scatter_mesh_1D.cc:87-97): the core limit, at most
        // 2n below 512 KiB of output; aiv_reduce_scatter_op.h:23-37 takes the big-data kernel above 2n blocks (out =
        // rank 0's copy, then (op)= rank 1 .. n-1: O2, aiv_reduce_scatter_mesh_1d_bigdata.h:85-101), the local tree
        // (O4, aiv_reduce_scatter_local_tree.h:138-172, and its core-control twin) otherwise. Executor loops of
        // min(UB_MAX_DATA_SIZE, ccl / 2n) per block (scratch multiple 2n); neither order depends on them.
        uint32_t blocks = coreLimit;
        if (count * es < (512ull << 10)) blocks = std::min(blocks, 2 * n);
        p.kind = kIpcReduceScatter;
        p.geom = kIpcGeomBlock;
        p.loopElems = LoopElems(std::min<uint64_t>(kUbMaxDataSize, RoundDown128(cclBytes / (2ull * n))), es);
        if (blocks > 2 * n) {
            variant = HCCL_AMD_AIV_RS_BIGDATA;
            p.order = kIpcO2;
        } else {
            variant = HCCL_AMD_AIV_RS_LOCAL_TREE;
            p.order = kIpcO4;
        }
    }
    if (plan != nullptr) *plan = p;
    if (group != nullptr) *group = g;
    return variant;
}

// ------------------------------------------------------------------------------------------------ launch geometry

bool IpcUseLl(const IpcCall& call, const IpcEnv& env)
{
    const IpcPlan& p = call.plan;
    const bool llKind =
        (p.kind == kIpcAllReduceOneShot && call.opType == HCCL_AMD_OP_ALLREDUCE && p.geom == kIpcGeomWhole) ||
        (p.kind == kIpcReduceScatter && call.opType == HCCL_AMD_OP_REDUCE_SCATTER && p.geom == kIpcGeomBlock);
    return llKind && (p.loopElems == 0 || call.count <= p.loopElems) &&
           call.count * env.es <= std::min<uint64_t>(env.llBytes, kIpcLlMaxBytes);
}

uint32_t IpcBlockCount(const IpcCall& call, const IpcEnv& env, bool ll)
{
    uint32_t blocks = env.blocksOverride;
    if (blocks == 0) {
        const bool blockLayout = call.opType == HCCL_AMD_OP_REDUCE_SCATTER || call.opType == HCCL_AMD_OP_ALLGATHER ||
                                 call.opType == HCCL_AMD_OP_SCATTER;
        // RS input / AG output / the Scatter root's input
        uint64_t callBytes = (blockLayout ? uint64_t(env.n) : 1u) * call.count * env.es;
        if (call.plan.kind == kIpcAllToAll) {
            // n pairs of at most `count` elements when every rank knows the matrix; an AlltoAllV's counts are not
            // common knowledge, so its blocks follow the capacity of the tier it runs in (equal on every rank)
            callBytes = call.plan.subMode == kIpcA2aAgreed ? env.a2aAreaBytes : uint64_t(env.n) * call.count * env.es;
        }
        if (call.plan.geom == kIpcGeomV) {
            callBytes = 0;
            for (uint32_t q = 0; q < env.n; ++q) callBytes += call.vCounts[q] * env.es;
        }
        blocks = ll ? LlIpcBlocks(env.n, call.count * env.es, call.plan.order == kIpcRhd) : DefaultIpcBlocks(callBytes);
        if (env.sharedDevice) blocks = std::min(blocks, kIpcBlocks);
    }
    if (env.residentPerRank != 0) blocks = std::min(blocks, env.residentPerRank);
    return blocks;
}

std::vector<IpcLoop> IpcLoops(const IpcCall& call)
{
    std::vector<IpcLoop> loops;
    if (call.plan.kind == kIpcBarrier) {
        loops.push_back({0, 0});  // one launch, no elements
        return loops;
    }
    if (call.plan.geom == kIpcGeomV) {
        // the launch is collective (every block meets its peers at the barriers), and a rank whose block is empty
        // still pushes its share of the others' blocks
        loops.push_back({0, 0});
        return loops;
    }
    if (call.plan.kind == kIpcAllToAll) {
        // one launch whatever the counts: a rank with nothing to move still meets its peers at the barriers
        loops.push_back({0, call.count});
        return loops;
    }
    const uint64_t loopElems = call.plan.loopElems != 0 ? call.plan.loopElems : call.count;
    for (uint64_t off = 0; off < call.count; off += loopElems) {
        loops.push_back({off, std::min(loopElems, call.count - off)});
    }
    return loops;
}

uint64_t IpcSlotCap(uint32_t kind, const IpcEnv& env, const IpcTierBytes& areas)
{
    const uint64_t V = 16 / env.es;
    const uint64_t slotsPerArea = kind == kIpcBroadcastOneShot || kind == kIpcScatter ? 1 : env.n;
    return ((HostSingleBarrierKind(kind) ? areas.altBytes : areas.inBytes) / env.es / slotsPerArea) / V * V;
}

IpcGeometry IpcLoopGeometry(const IpcCall& call, const IpcEnv& env, uint64_t cnt, uint64_t slotCap, uint32_t blocks,
                            bool ll)
{
    const IpcPlan& plan = call.plan;
    const uint64_t n = env.n, es = env.es, V = 16 / es;
    IpcGeometry g{};
    if (plan.kind == kIpcBarrier) {
        // one barrier epoch on workgroup 0's flag words and nothing else (k_ipc_barrier): every length stays 0
        g.rounds = 1;
        g.epochSpan = 1;
        return g;
    }
    g.group = 1;
    g.total = cnt;
    if (plan.kind == kIpcAllToAll) {
        // Slot q of a rank's alternate area holds the round's part of pair (q, rank): slotCap elements apart, the
        // agreed form's header first. cnt is the largest pair count (kIpcA2aKnown) and unused otherwise. piece = 0
        // says that the area is too small for the header (the caller refuses the call).
        const bool agreed = plan.subMode == kIpcA2aAgreed;
        const uint64_t hdr = agreed ? kIpcA2aHeaderBytes / es : 0;
        const uint64_t cap = slotCap > hdr ? slotCap - hdr : 0;
        g.chunkLen = cnt;
        g.tileElems = env.tileBytes / es / V * V;
        if (cap < V) return g;
        if (agreed) {
            g.piece = cap;  // rounds 0: agreed on the device; epochSpan has no meaning then (EndLaunchSpan)
        } else {
            g.piece = std::max<uint64_t>(V, std::min(cap, (cnt + V - 1) / V * V));
            g.rounds = static_cast<uint32_t>(
                std::min<uint64_t>(UINT32_MAX, std::max<uint64_t>(1, (cnt + g.piece - 1) / g.piece)));
            g.epochSpan = g.rounds;
        }
        const uint64_t nb = std::max<uint32_t>(blocks, 1);
        g.blockElems = ((g.piece + nb - 1) / nb + V - 1) / V * V;
        return g;
    }
    switch (plan.geom) {
        case kIpcGeomV:
            // ReduceScatterV: rank c's block is counts[c] elements at displs[c] of every input (one launch: the
            // mesh order O1 does not depend on executor loops)
            g.vgeom = 1;
            for (uint32_t q = 0; q < n; ++q) {
                g.vStart[q] = call.vDispls[q];
                g.vLen[q] = call.vCounts[q];
                g.chunkLen = std::max(g.chunkLen, call.vCounts[q]);
            }
            break;
        case kIpcGeomBlock:
            // block c of the input (recvCount elements, stride recvCount) is chunk c (reduce_scatter_op.cc:158-159)
            g.chunkStride = call.count;
            g.chunkLen = cnt;
            g.total = (n - 1) * call.count + cnt;
            break;
        case kIpcGeomBalanced: {
            const uint64_t slices = uint64_t(plan.group) * n;
            g.balanced = 1;
            g.group = plan.group;
            g.chunkLen = cnt / slices;  // slice length; the first cnt % slices slices hold one more
            g.rem = cnt % slices;
            break;
        }
        case kIpcGeomWhole:
            // every rank holds (and, for the AllReduce, folds) the whole range; AllGather: its whole input
            g.chunkLen = cnt;
            break;
        case kIpcGeomCeil:
            g.chunkStride = g.chunkLen = (cnt + n - 1) / n;
            break;
        default: {
            const uint64_t align = 128 / es;  // HCCL_MIN_SLICE_ALIGN
            g.chunkStride = g.chunkLen = ((cnt + n - 1) / n + align - 1) / align * align;
            break;
        }
    }
    const uint64_t widest = g.balanced != 0 ? g.group * g.chunkLen + std::min<uint64_t>(g.group, g.rem) : g.chunkLen;
    g.piece = std::max<uint64_t>(V, std::min(slotCap, (widest + V - 1) / V * V));
    g.blockElems = ((g.piece + blocks - 1) / blocks + V - 1) / V * V;
    g.tileElems = env.tileBytes / es / V * V;  // 0: contiguous windows (HCCL_AMD_IPC_TILE_KIB)
    g.rounds = static_cast<uint32_t>((widest + g.piece - 1) / g.piece);
    g.epochSpan = (HostSingleBarrierKind(plan.kind) ? 1 : 2) * g.rounds;
    if (ll && g.rounds == 1) {  // one window per block, no barrier epochs (the LL sequence advances)
        g.ll = 1;
        g.tileElems = 0;
        g.epochSpan = 0;
    }
    return g;
}

HcclResult IpcPlanQuery(const HcclAmdIpcPlanQuery& q, uint64_t es, uint64_t cclBytes, uint64_t ipcStagingBytes,
                        uint64_t smallIpcBytes, HcclAmdIpcPlanResult* res, std::vector<IpcGeometry>* launches)
{
    // what the operators' callers guarantee (RunCollective returns one-rank calls earlier; IpcPlanForFamily divides
    // by n - 1)
    if (q.nRanks < 2 || q.nRanks > uint32_t(kIpcMaxRanks)) return HCCL_E_PARA;
    if (q.opType == HCCL_AMD_OP_BARRIER) {
        // any family, no count and no data type: what RunIpcBarrier launches, which asks for no tier (areas 0)
        const IpcCall barrier{q.opType, IpcPlanBarrier(), 0};
        IpcEnv env{};
        env.n = q.nRanks;
        env.es = 1;
        *res = HcclAmdIpcPlanResult{};
        res->blocks = 1;
        res->numLaunches = 1;
        if (launches != nullptr) launches->assign(1, IpcLoopGeometry(barrier, env, 0, 0, 1, false));
        return HCCL_SUCCESS;
    }
    if (es != 1 && es != 2 && es != 4 && es != 8) return HCCL_E_PARA;
    IpcCall call{q.opType, IpcPlan{}, q.count, q.counts, q.displs};
    HcclResult r = HCCL_SUCCESS;
    if (q.family < 0) {
        call.plan = IpcPlan{q.kind, q.order, q.geom, q.group, q.subMode, q.loopElems};
    } else if (q.opType == HCCL_AMD_OP_BROADCAST) {
        if (q.family == HCCL_AMD_ALGO_AUTO) {
            call.plan = IpcPlanBroadcast(q.count, es, 0);
        } else if (q.family == HCCL_AMD_ALGO_MESH_TWOSHOT) {
            call.plan = IpcPlanBroadcast(q.count, es, 1);
        } else if (q.family == HCCL_AMD_ALGO_MESH_ONESHOT) {
            call.plan = IpcPlanBroadcast(q.count, es, 2);
        } else {
            r = HCCL_E_NOT_SUPPORT;
        }
    } else if (q.opType == HCCL_AMD_OP_ALLTOALL) {
        // AlltoAll / AlltoAllVC (count = the matrix's largest entry); AlltoAllV is the explicit plan with
        // subMode = kIpcA2aAgreed
        call.plan = IpcPlanAllToAll(false);
    } else if (q.opType == HCCL_AMD_OP_SCATTER) {
        call.plan = IpcPlanScatter();
    } else if (q.opType == HCCL_AMD_OP_ALLGATHER_V) {
        call.plan = IpcPlanAllGatherV();
    } else if (q.family == HCCL_AMD_ALGO_IPC_RHD) {
        r = q.opType == HCCL_AMD_OP_ALLREDUCE ? IpcPlanRhd(q.nRanks, &call.plan) : HCCL_E_NOT_SUPPORT;
    } else {
        r = IpcPlanForFamily(q.opType, q.family, q.nRanks, es, cclBytes, &call.plan);
    }
    if (r != HCCL_SUCCESS) return r;
    const IpcPlan& p = call.plan;
    if (p.kind > kIpcAllGatherV || p.order > kIpcRhd || p.geom > kIpcGeomV || p.group < 1) return HCCL_E_PARA;
    if (p.geom == kIpcGeomV && (q.counts == nullptr || q.displs == nullptr || p.loopElems != 0)) return HCCL_E_PARA;
    const bool a2a = p.kind == kIpcAllToAll;
    if (a2a && (p.subMode > kIpcA2aAgreed || p.geom == kIpcGeomV || p.loopElems != 0)) return HCCL_E_PARA;
    const bool agreed = a2a && p.subMode == kIpcA2aAgreed;

    IpcEnv env{};
    env.n = q.nRanks;
    env.es = es;
    env.sharedDevice = q.sharedDevice != 0;
    env.blocksOverride = q.blocks;
    env.residentPerRank = q.residentPerRank;
    env.tileBytes = q.tileBytes;
    env.llBytes = q.llBytes;
    const bool ll = IpcUseLl(call, env);
    const std::vector<IpcLoop> loops = IpcLoops(call);

    IpcTierBytes areas{q.areaBytes, q.areaBytes, q.altBytes};
    if (agreed) {
        // count-free: the small tier, and the blocks from its capacity (RunIpcPlan takes the large tier only when the
        // small one's set-up failed)
        if (q.areaBytes == 0 && q.altBytes == 0) {
            areas = IpcTierSizes(env.n, cclBytes, ipcStagingBytes, smallIpcBytes, kIpcTierSmall);
        }
        env.a2aAreaBytes = areas.altBytes;
    }
    const uint32_t blocks = IpcBlockCount(call, env, ll);
    if (!agreed && q.areaBytes == 0 && q.altBytes == 0) {
        // the small tier when every launch of the call fits one round there, else the large one
        areas = IpcTierSizes(env.n, cclBytes, ipcStagingBytes, smallIpcBytes, kIpcTierSmall);
        const uint64_t smallCap = IpcSlotCap(p.kind, env, areas);
        for (const IpcLoop& l : loops) {
            if (IpcLoopGeometry(call, env, l.cnt, smallCap, blocks, ll).rounds != 1) {
                areas = IpcTierSizes(env.n, cclBytes, ipcStagingBytes, smallIpcBytes, kIpcTierLarge);
                break;
            }
        }
    }
    const uint64_t slotCap = IpcSlotCap(p.kind, env, areas);
    if (a2a && IpcLoopGeometry(call, env, q.count, slotCap, blocks, false).piece == 0) return HCCL_E_PARA;
    res->blocks = blocks;
    res->ll = ll ? 1u : 0u;
    res->areaBytes = areas.inBytes;
    res->altBytes = areas.altBytes;
    res->numLaunches = loops.size();
    if (launches != nullptr) {
        launches->clear();
        for (const IpcLoop& l : loops) launches->push_back(IpcLoopGeometry(call, env, l.cnt, slotCap, blocks, ll));
    }
    return HCCL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ point-to-point

HcclResult P2pPlanFor(uint64_t count, uint64_t es, uint64_t slotBytes, uint32_t n, P2pPlan* plan)
{
    if (plan == nullptr) return HCCL_E_PTR;
    if (es != 1 && es != 2 && es != 4 && es != 8) return HCCL_E_PARA;
    if (slotBytes < kP2pSlotBytesMin || slotBytes > kP2pSlotBytesMax || slotBytes % 128 != 0) return HCCL_E_PARA;
    if (n < 1 || n > uint32_t(kIpcMaxRanks)) return HCCL_E_PARA;
    const uint64_t V = 16 / es;
    P2pPlan p{};
    p.slotElems = slotBytes / es;
    // every window but the last starts and ends on a 16-byte vector of the slot
    p.blockElems = ((p.slotElems + kP2pBlocks - 1) / kP2pBlocks + V - 1) / V * V;
    p.pieces = count / p.slotElems + (count % p.slotElems != 0 ? 1 : 0);
    p.blocks = kP2pBlocks;
    p.slots = kP2pSlots;
    p.dataBytes = uint64_t(n) * kP2pSlots * slotBytes;
    const uint64_t flagBytes = 2 * uint64_t(n) * kP2pBlocks * sizeof(uint32_t);  // filled[n][B], then drained[n][B]
    p.areaBytes = (p.dataBytes + flagBytes + 4095) / 4096 * 4096;
    p.counterBytes = flagBytes;  // sent[n][B], then rcvd[n][B]
    *plan = p;
    return HCCL_SUCCESS;
}

HcclResult BatchSendRecvOrder(const HcclSendRecvItem* items, uint32_t itemNum, uint32_t rank, uint32_t rankSize,
                              uint32_t* order, uint32_t* numSends, uint32_t* numRecvs, uint32_t* numSelfPairs)
{
    if (items == nullptr || order == nullptr || numSends == nullptr || numRecvs == nullptr || numSelfPairs == nullptr) {
        return HCCL_E_PTR;
    }
    std::vector<uint32_t> sends, recvs;
    for (uint32_t i = 0; i < itemNum; ++i) {
        if (items[i].count == 0) continue;
        if (items[i].buf == nullptr) return HCCL_E_PTR;
        if (items[i].sendRecvType == HCCL_SEND) {
            sends.push_back(i);
        } else if (items[i].sendRecvType == HCCL_RECV) {
            recvs.push_back(i);
        } else {
            return HCCL_E_PARA;
        }
    }
    // SortSendItems / SortRecvItems: the sends from this rank downwards, the receives from it upwards (both cyclic, the
    // self items first), duplicates of a pair by count, then data type, both descending
    const auto bySize = [&](uint32_t a, uint32_t b) {
        if (items[a].count != items[b].count) return items[a].count > items[b].count;
        return items[a].dataType > items[b].dataType;
    };
    const auto sendKey = [&](uint32_t i) { return items[i].remoteRank <= rank ? items[i].remoteRank + rankSize : items[i].remoteRank; };
    const auto recvKey = [&](uint32_t i) { return items[i].remoteRank < rank ? items[i].remoteRank + rankSize : items[i].remoteRank; };
    std::stable_sort(sends.begin(), sends.end(), [&](uint32_t a, uint32_t b) {
        return sendKey(a) != sendKey(b) ? sendKey(a) > sendKey(b) : bySize(a, b);
    });
    std::stable_sort(recvs.begin(), recvs.end(), [&](uint32_t a, uint32_t b) {
        return recvKey(a) != recvKey(b) ? recvKey(a) < recvKey(b) : bySize(a, b);
    });
    size_t selfSends = 0, selfRecvs = 0;
    while (selfSends < sends.size() && items[sends[selfSends]].remoteRank == rank) ++selfSends;
    while (selfRecvs < recvs.size() && items[recvs[selfRecvs]].remoteRank == rank) ++selfRecvs;
    if (selfSends != selfRecvs) return HCCL_E_PARA;  // a self item without its partner
    for (size_t k = 0; k < selfSends; ++k) {
        if (items[sends[k]].count != items[recvs[k]].count) return HCCL_E_PARA;
    }
    uint32_t w = 0;
    for (size_t k = selfSends; k < sends.size(); ++k) order[w++] = sends[k];
    for (size_t k = selfRecvs; k < recvs.size(); ++k) order[w++] = recvs[k];
    for (size_t k = 0; k < selfSends; ++k) {
        order[w++] = sends[k];
        order[w++] = recvs[k];
    }
    *numSends = static_cast<uint32_t>(sends.size() - selfSends);
    *numRecvs = static_cast<uint32_t>(recvs.size() - selfRecvs);
    *numSelfPairs = static_cast<uint32_t>(selfSends);
    return HCCL_SUCCESS;
}

HcclResult FillCheckRecord(int32_t opType, uint32_t root, HcclReduceOp op, HcclDataType dt, uint64_t count,
                           uint64_t bufferBytes, bool expansionAiv, bool strict, uint32_t aivCoreLimit,
                           CheckRecord* rec)
{
    bool hasRoot = false, hasOp = false, hasType = true, hasCount = true;
    switch (opType) {
        case HCCL_AMD_OP_ALLREDUCE:
        case HCCL_AMD_OP_REDUCE_SCATTER: hasOp = true; break;
        case HCCL_AMD_OP_REDUCE: hasOp = hasRoot = true; break;
        case HCCL_AMD_OP_ALLGATHER:
        case HCCL_AMD_OP_ALLTOALL: break;  // AlltoAll: count = sendCount
        case HCCL_AMD_OP_BROADCAST:
        case HCCL_AMD_OP_SCATTER: hasRoot = true; break;
        // counts that legitimately differ per rank: the data type only
        case HCCL_AMD_OP_REDUCE_SCATTER_V: hasOp = true; hasCount = false; break;
        case HCCL_AMD_OP_ALLGATHER_V:
        case HCCL_AMD_CHECK_OP_ALLTOALLV:
        case HCCL_AMD_CHECK_OP_ALLTOALLVC: hasCount = false; break;
        case HCCL_AMD_OP_BARRIER: hasType = hasCount = false; break;
        default: return HCCL_E_PARA;
    }
    const uint64_t cnt = hasCount ? count : 0;
    *rec = CheckRecord{};
    rec->w[0] = static_cast<uint32_t>(bufferBytes);
    rec->w[1] = static_cast<uint32_t>(bufferBytes >> 32);
    rec->w[2] = hasRoot ? root : kCheckNoRoot;
    rec->w[3] = static_cast<uint32_t>(opType);
    rec->w[4] = expansionAiv ? 1u : 0u;
    rec->w[5] = static_cast<uint32_t>(hasOp ? op : HCCL_REDUCE_RESERVED);
    rec->w[6] = static_cast<uint32_t>(hasType ? dt : HCCL_DATA_TYPE_RESERVED);
    rec->w[7] = static_cast<uint32_t>(cnt);
    rec->w[8] = static_cast<uint32_t>(cnt >> 32);
    rec->w[9] = aivCoreLimit;
    rec->w[10] = strict ? 1u : 0u;
    return HCCL_SUCCESS;
}

uint64_t CheckFieldValue(const CheckRecord& rec, uint32_t field)
{
    if (field >= HCCL_AMD_CHECK_FIELDS) return 0;
    const uint32_t w = CheckFirstWord(field);
    return uint64_t(rec.w[w]) | (CheckWideField(field) ? uint64_t(rec.w[w + 1]) << 32 : 0);
}

}  // namespace hccl_amd
