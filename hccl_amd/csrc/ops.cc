// ops.cc — the operator surface of include/hccl.h plus the communicator extensions of include/hccl_amd.h.
//
// Each entry point keeps the reference's validation order and return codes:
//   HcclAllReduce      all_reduce_op.cc:23-52, AllReduceInitAndCheck :107-133, CheckAllReduceInputPara :135-157
//   HcclReduceScatter  reduce_scatter_op.cc:23-72, CheckReduceScatterInputPara
//   HcclReduce         reduce_op.cc:23-54, ReduceInitAndCheck, CheckReduceInputPara :106-127
//   CheckCount / CheckDataType / CheckReduceOp / SingleRankProc   op_common.cc:2902-3098
// then build this rank's schedule (schedule.cc) and run it (executor.cc).
#include <strings.h>

#include <algorithm>

#include <cstring>

#include "comm.h"

namespace hccl_amd {

namespace {

constexpr uint64_t kSysMaxCount = 0x7FFFFFFFFull;  // SYS_MAX_COUNT, hccl_common.h:42

HcclResult CheckCount(uint64_t count) { return count > kSysMaxCount ? HCCL_E_PARA : HCCL_SUCCESS; }

// CheckDataType(dataType, needReduce = true), op_common.cc:2913-2950
HcclResult CheckReduceDataType(HcclDataType dt) { return IsReduceDataType(dt) ? HCCL_SUCCESS : HCCL_E_NOT_SUPPORT; }

// CheckReduceOp, op_common.cc:2977-2998: PROD only on INT8/INT32/INT64/UINT64/FP16/FP32/FP64. An op outside
// {SUM, PROD, MAX, MIN} has no reference check at the entry (it fails deep in the template); it is HCCL_E_PARA here.
HcclResult CheckReduceOp(HcclDataType dt, HcclReduceOp op)
{
    if (op == HCCL_REDUCE_PROD) {
        switch (dt) {
            case HCCL_DATA_TYPE_INT8:
            case HCCL_DATA_TYPE_INT32:
            case HCCL_DATA_TYPE_INT64:
            case HCCL_DATA_TYPE_UINT64:
            case HCCL_DATA_TYPE_FP16:
            case HCCL_DATA_TYPE_FP32:
            case HCCL_DATA_TYPE_FP64: return HCCL_SUCCESS;
            default: return HCCL_E_NOT_SUPPORT;
        }
    }
    if (op != HCCL_REDUCE_SUM && op != HCCL_REDUCE_MAX && op != HCCL_REDUCE_MIN) return HCCL_E_PARA;
    return HCCL_SUCCESS;
}

// HCCL_DETERMINISTIC=strict (alg_env_config.cc:1036-1076; CommConfig::strict) with fp16/fp32/bf16/fp64, SUM/PROD and
// more than two ranks selects the order-preserved tree (IsNeedStrictModeForOrderPreserved, order_preserved_common.h:
// 63-73). At n <= 8 the reference runs it as InsTempReduceScatterOrderPreservedLevel1 (reduce_scatter_auto_selector.cc:
// 406-413), whose tree is the same O4 (schedule.cc ReduceScatterTree).
bool NeedStrictOrder(const Comm& c, int32_t opType, HcclDataType dt, HcclReduceOp op)
{
    const uint32_t nRanks = c.nRanks;
    if (!c.cfg.strict) return false;
    if (opType != HCCL_AMD_OP_ALLREDUCE && opType != HCCL_AMD_OP_REDUCE_SCATTER) return false;
    const bool fp = dt == HCCL_DATA_TYPE_FP16 || dt == HCCL_DATA_TYPE_FP32 || dt == HCCL_DATA_TYPE_BFP16 ||
                    dt == HCCL_DATA_TYPE_FP64;
    return fp && (op == HCCL_REDUCE_SUM || op == HCCL_REDUCE_PROD) && nRanks > 2;
}

// isDataTypeOrReduceTypeSpecial of the selectors (all_reduce_auto_selector.cc:525-528,
// reduce_scatter_auto_selector.cc:477): 64-bit data or PROD.
bool IsSpecialForSelector(HcclDataType dt, HcclReduceOp op)
{
    return dt == HCCL_DATA_TYPE_INT64 || dt == HCCL_DATA_TYPE_UINT64 || dt == HCCL_DATA_TYPE_FP64 ||
           op == HCCL_REDUCE_PROD;
}

// Pipelining granule of a call: the communicator's (HcclAmdCommSetPieceBytes) if set. Otherwise the schedule's default
// for the two-stream executor, and one piece per slice (as far as the staging holds) for the single-stream one, where
// pieces cannot overlap anything and each costs a transport group (about 10 us of host time per group, RCCL self-loop
// programs: profiles/r02_rccl_selfloop_latency*.jsonl). Pieces never change a fold order: every order is fixed per
// executor loop and slice, and a piece only splits a slice's elements.
uint64_t PieceBytesFor(const Comm& c, bool singleStream, uint64_t payload)
{
    if (c.pieceBytes != 0) return c.pieceBytes;
    return singleStream ? std::max<uint64_t>(payload, 128) : 0;  // no slice is larger than the payload
}

// A pointer a kernel of this device may dereference: device memory, or host memory registered and mapped for it.
bool DeviceAccessible(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an unregistered host pointer reports an error: clear it
        return false;
    }
    // registered host memory counts only where the device addresses it at the host pointer itself (the copy kernel is
    // handed that pointer); a registration mapped elsewhere goes to hipMemcpyAsync
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged ||
           (a.type == hipMemoryTypeHost && a.devicePointer == p);
}

// The one-rank collective's copy (SingleRankProc). The library's copy kernel when both buffers are device-accessible;
// hipMemcpyAsync otherwise, which resolves pageable host memory where a kernel would fault the GPU.
HcclResult CopyUserBuffer(void* dst, const void* src, uint64_t bytes, hipStream_t stream)
{
    if (bytes == 0 || dst == src) return HCCL_SUCCESS;
    if (DeviceAccessible(dst) && DeviceAccessible(src)) return LaunchCopyBytes(dst, src, bytes, stream);
    HIP_CHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, stream));
    return HCCL_SUCCESS;
}

// Runs the schedule of p on the communicator: the caller has set the operation's own fields (opType, algo, count,
// root, special, counts / displs); `payload` is the bytes of this rank's input that the call moves.
HcclResult RunSchedule(Comm& c, ScheduleParams& p, uint64_t payload, void* sendBuf, void* recvBuf, HcclDataType dt,
                       HcclReduceOp op, hipStream_t stream)
{
    const uint32_t es = DataTypeSize(dt);
    // a Broadcast's program stages nothing: it allocates no staging either (DDP broadcasts once HBM is full); nor do
    // an all-to-all's, a Scatter's and an AllGatherV's, nor a barrier's (its tokens are its INPUT and OUTPUT)
    const bool moveOnly = p.opType == HCCL_AMD_OP_ALLTOALL || p.opType == HCCL_AMD_OP_SCATTER ||
                          p.opType == HCCL_AMD_OP_ALLGATHER_V || p.opType == HCCL_AMD_OP_BARRIER;
    if (p.opType != HCCL_AMD_OP_BROADCAST && !moveOnly) HCCL_CHK(c.EnsureScratch());
    p.nRanks = c.nRanks;
    p.rank = c.rank;
    p.elemSize = es;
    p.scratchCapBytes = c.scratchBytes;
    p.cclBytes = c.cclBytes;
    void* bufs[3] = {sendBuf, recvBuf, c.scratch};
    const bool single = c.nRanks == 1 || payload <= c.cfg.singleStreamBytes;
    p.pieceBytes = PieceBytesFor(c, single, payload);
    // an all-to-all's payload differs from rank to rank, and both ends of a pair must cut it alike: only the
    // communicator's explicit granule (equal on every rank) applies, and 0 is its one-group default. The same holds
    // for a Scatter (the root's payload is n times a peer's) and an AllGatherV (every rank's block has its own size)
    if (moveOnly) p.pieceBytes = c.pieceBytes;
    const CompiledSchedule* cs = nullptr;
    HCCL_CHK(CompileCollective(c, p, bufs, !single, &cs));
    const Schedule& s = cs->sched;
    if (s.scratchElems * es > c.scratchBytes) {
        HCCL_AMD_ERR("schedule needs %llu B of staging, communicator has %llu B",
                     (unsigned long long)(s.scratchElems * es), (unsigned long long)c.scratchBytes);
        return HCCL_E_INTERNAL;
    }
    c.lastAlgo = s.algo;
    HCCL_AMD_LOG("rank %u op %d algo %d count %llu ops %zu", c.rank, p.opType, s.algo, (unsigned long long)p.count,
                 s.ops.size());
    // single-stream programs replay from the executor graph cache too (RCCL path, the key's second call on)
    return RunCompiled(c, *cs, bufs, dt, op, stream, single);
}

// The cross-rank argument check ahead of a checked collective (HCCL_DFS_CONFIG=inconsistent_check; ipc.cc RunIpcCheck):
// behind the local argument checks, the status gate and the one-rank return, before the data path is chosen. It runs on
// the caller's stream whatever path the data then takes. Nothing happens with the switch off.
HcclResult CheckArgs(Comm& c, int32_t opType, uint32_t root, HcclReduceOp op, HcclDataType dt, uint64_t count,
                     hipStream_t stream)
{
    if (c.cfg.inconsistentCheck < 0) return HCCL_SUCCESS;
    CheckRecord rec{};
    HCCL_CHK(FillCheckRecord(opType, root, op, dt, count, c.cclBytes, c.cfg.expansionAiv, c.cfg.strict,
                             c.cfg.aivCoreLimit, &rec));
    return RunIpcCheck(c, rec, stream);
}

HcclResult RunCollective(Comm& c, int32_t opType, void* sendBuf, void* recvBuf, uint64_t count, HcclDataType dt,
                         HcclReduceOp op, uint32_t root, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());  // a failed communicator takes no more work (op_common.cc:89-97)
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    const uint32_t es = DataTypeSize(dt);
    if (c.nRanks == 1) {
        // SingleRankProc (op_common.cc:3042-3098): copy in -> out unless they are the same buffer.
        c.lastAlgo = HCCL_AMD_ALGO_AUTO;
        return CopyUserBuffer(recvBuf, sendBuf, count * es, stream);
    }
    HCCL_CHK(CheckArgs(c, opType, root, op, dt, count, stream));
    ScheduleParams p;
    p.opType = opType;
    p.algo = c.algoOverride;
    if (opType == HCCL_AMD_OP_BROADCAST) {
        // Data movement only, so no family has bits of its own: the one-sided kernel on an IPC-only communicator, when
        // a one-sided family is asked for, and for small calls (the small-call rule below, extended to this op); the
        // mesh two-shot schedule (the reference's single-node choice, broadcast_auto_selector.cc:233-246) otherwise,
        // and when the kernel cannot run (no peer mappings, a capture before the set-up).
        const bool ipcOnly = !c.transport->HasSendRecv();
        const bool asked = p.algo == HCCL_AMD_ALGO_IPC || p.algo == HCCL_AMD_ALGO_IPC_TWOSHOT ||
                           p.algo == HCCL_AMD_ALGO_AIV || p.algo == HCCL_AMD_ALGO_AIV_ONLY;
        const bool small = p.algo == HCCL_AMD_ALGO_AUTO && !c.ipc.unavailable && count * es <= c.cfg.smallIpcBytes;
        if (ipcOnly || asked || small) {
            const HcclResult r = RunIpcBroadcast(c, recvBuf, count, dt, root, stream);
            if (r != HCCL_E_NOT_SUPPORT) {
                c.lastAlgo = HCCL_AMD_ALGO_IPC;
                return r;
            }
            if (ipcOnly) return HCCL_E_NOT_SUPPORT;
        }
        p.algo = HCCL_AMD_ALGO_MESH_TWOSHOT;
        p.count = count;
        p.root = root;
        return RunSchedule(c, p, count * es, sendBuf, recvBuf, dt, op, stream);
    }
    // The AIV engine (HCCL_OP_EXPANSION_MODE=AIV, or forced per communicator): SelectAivAlgo's choice and its
    // kernels' orders on the one-sided kernel. What it does not match, or cannot run (no peer mappings, a capture
    // before the set-up), takes the AICPU engine's selection below, as the reference falls back
    // (AutoSelectorBase::ProcessAivConfig, auto_selector_base.cc:353-371).
    // AIV_ONLY (the reference's OpExecuteConfig::AIV_ONLY, a communicator's configured expansion mode) takes no
    // fallback: an operation the AIV engine does not match returns HCCL_E_NOT_SUPPORT (op_common.cc:115-122).
    const bool aivOnly = p.algo == HCCL_AMD_ALGO_AIV_ONLY;
    if (aivOnly || p.algo == HCCL_AMD_ALGO_AIV || (p.algo == HCCL_AMD_ALGO_AUTO && c.cfg.expansionAiv)) {
        IpcPlan plan{};
        const int32_t v = SelectAivPlan(opType, c.nRanks, count, dt, es, op, NeedStrictOrder(c, opType, dt, op),
                                        aivOnly, c.cclBytes, c.cfg.aivCoreLimit, &plan, nullptr);
        if (v != HCCL_AMD_AIV_NOT_MATCHED) {
            const HcclResult r = RunIpcPlan(c, opType, plan, sendBuf, recvBuf, count, dt, op, root, stream);
            if (r != HCCL_E_NOT_SUPPORT) {
                c.lastAlgo = aivOnly ? HCCL_AMD_ALGO_AIV_ONLY : HCCL_AMD_ALGO_AIV;
                return r;
            }
        }
        if (aivOnly) return HCCL_E_NOT_SUPPORT;
        p.algo = HCCL_AMD_ALGO_AUTO;
    }
    // RHD's bits from one launch of the one-sided kernel (AllReduce, power-of-two n). An IPC-only communicator asked for
    // RHD takes it too, so it keeps RHD's order. Anything else runs the RHD schedule (or its own fallbacks).
    if (p.algo == HCCL_AMD_ALGO_RHD && !c.transport->HasSendRecv()) p.algo = HCCL_AMD_ALGO_IPC_RHD;
    if (p.algo == HCCL_AMD_ALGO_IPC_RHD) {
        IpcPlan plan{};
        if (opType == HCCL_AMD_OP_ALLREDUCE && IpcPlanRhd(c.nRanks, &plan) == HCCL_SUCCESS) {
            const HcclResult r = RunIpcPlan(c, opType, plan, sendBuf, recvBuf, count, dt, op, root, stream);
            if (r != HCCL_E_NOT_SUPPORT) {
                c.lastAlgo = HCCL_AMD_ALGO_IPC_RHD;
                return r;
            }
        }
        p.algo = HCCL_AMD_ALGO_RHD;
    }
    // an IPC-only communicator (bootstrap transport without send/recv) runs every reducing op on the IPC kernel in
    // the auto family, whatever schedule family was asked for
    if (!c.transport->HasSendRecv() && p.algo != HCCL_AMD_ALGO_IPC_TWOSHOT) p.algo = HCCL_AMD_ALGO_IPC;
    if (p.algo == HCCL_AMD_ALGO_AUTO && NeedStrictOrder(c, opType, dt, op)) {
        p.algo = HCCL_AMD_ALGO_ORDER_PRESERVED;
    }
    // Small collectives take the one-sided kernel (HCCL_AMD_SMALL_IPC_BYTES, default 1 MiB per rank): one launch with
    // one or two cross-rank barriers instead of the transport groups of a schedule, each of which costs a group launch
    // (1 KiB one-shot over RCCL: 29-32 us, an 8-rank RHD: 81.5 us; profiles/r03_host_cost_rccl_selfloop.jsonl,
    // r02_rccl_selfloop_latency.jsonl). The reference runs small data on its vector cores the same way
    // (all_reduce_auto_selector.cc:591-683; a task costs it 1-2 us, cost_model.cc:240-245). The bits do not change: the
    // auto family runs in the auto family's order (HCCL_AMD_ALGO_IPC), RHD in RHD's (HCCL_AMD_ALGO_IPC_RHD). Every rank
    // decides alike (count, dtype and the (=) config are equal on every rank); a call the kernel cannot take (no peer
    // mappings, a capture before the set-up) runs the schedule.
    // ReduceScatter and Reduce take the rule too (r05), in the auto family's order only (the one-sided kernel has no
    // RHD form of them); the threshold applies to the rank's input (ReduceScatter: n blocks).
    const bool reducing = opType == HCCL_AMD_OP_ALLREDUCE || opType == HCCL_AMD_OP_REDUCE_SCATTER ||
                          opType == HCCL_AMD_OP_REDUCE;
    const uint64_t inBytes = count * es * (opType == HCCL_AMD_OP_REDUCE_SCATTER ? c.nRanks : 1);
    if (reducing && c.transport->HasSendRecv() && !c.ipc.unavailable && inBytes <= c.cfg.smallIpcBytes &&
        (p.algo == HCCL_AMD_ALGO_AUTO || (opType == HCCL_AMD_OP_ALLREDUCE && p.algo == HCCL_AMD_ALGO_RHD))) {
        IpcPlan plan{};
        HcclResult r = HCCL_E_NOT_SUPPORT;
        int32_t ran = HCCL_AMD_ALGO_IPC;
        if (p.algo == HCCL_AMD_ALGO_RHD) {
            ran = HCCL_AMD_ALGO_IPC_RHD;
            if (IpcPlanRhd(c.nRanks, &plan) == HCCL_SUCCESS) {
                r = RunIpcPlan(c, opType, plan, sendBuf, recvBuf, count, dt, op, root, stream);
            }
        } else {
            const int32_t family = SelectAlgo(opType, c.nRanks, count * es, IsSpecialForSelector(dt, op));
            r = RunIpcCollective(c, opType, family, sendBuf, recvBuf, count, dt, op, root, stream);
        }
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = ran;
            return r;
        }
    }
    if (p.algo == HCCL_AMD_ALGO_IPC_TWOSHOT || p.algo == HCCL_AMD_ALGO_IPC) {
        // the order family of the one-sided kernel: IPC_TWOSHOT fixes AllReduce two-shot (O2), mesh ReduceScatter
        // and two-shot Reduce; IPC takes whatever the auto selector takes, so its bits are the auto path's
        // (AllGather moves data only: the family does not matter)
        const uint64_t bytes = count * es;
        const int32_t family =
            p.algo == HCCL_AMD_ALGO_IPC
                ? SelectAlgo(opType, c.nRanks, bytes, IsSpecialForSelector(dt, op))
                : (opType == HCCL_AMD_OP_REDUCE_SCATTER ? HCCL_AMD_ALGO_MESH_ONESHOT : HCCL_AMD_ALGO_MESH_TWOSHOT);
        HcclResult r = RunIpcCollective(c, opType, family, sendBuf, recvBuf, count, dt, op, root, stream);
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = p.algo;
            return r;
        }
        // no peer mappings, or a capturing stream: the RCCL schedule with the same order, if there is RCCL
        if (!c.transport->HasSendRecv()) return HCCL_E_NOT_SUPPORT;
        p.algo = opType == HCCL_AMD_OP_ALLGATHER ? HCCL_AMD_ALGO_MESH_ONESHOT : family;
    }
    p.count = count;
    p.root = root;
    p.special = IsSpecialForSelector(dt, op);
    return RunSchedule(c, p, inBytes, sendBuf, recvBuf, dt, op, stream);
}

// ReduceScatterV (reduce_scatter_v_op.cc:24-83, ReduceScatterVOutPlaceCommon :285-330): the mesh template's order
// over per-rank blocks; the output holds counts[rank] elements.
HcclResult RunReduceScatterV(Comm& c, void* sendBuf, const uint64_t* counts, const uint64_t* displs, void* recvBuf,
                             HcclDataType dt, HcclReduceOp op, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    // ReduceScatterVAutoSelector::SelectAicpuAlgo (reduce_scatter_v_auto_selector.cc:180-197): UINT64 and FP64 have
    // no algorithm
    if (dt == HCCL_DATA_TYPE_UINT64 || dt == HCCL_DATA_TYPE_FP64) return HCCL_E_NOT_SUPPORT;
    if (c.nRanks > 1) HCCL_CHK(CheckArgs(c, HCCL_AMD_OP_REDUCE_SCATTER_V, 0, op, dt, 0, stream));
    // The one-sided kernel runs it over per-rank blocks (kIpcGeomV) in the same order O1 (own block first, then the
    // other ranks ascending): on an IPC-only communicator, which has no send/recv path, and when the communicator's
    // family is IPC / IPC_TWOSHOT. Without peer mappings an IPC-only communicator answers NOT_SUPPORT.
    const bool ipcOnly = !c.transport->HasSendRecv();
    if (c.nRanks > 1 &&
        (ipcOnly || c.algoOverride == HCCL_AMD_ALGO_IPC || c.algoOverride == HCCL_AMD_ALGO_IPC_TWOSHOT)) {
        IpcPlan plan{};
        plan.kind = kIpcReduceScatter;
        plan.order = kIpcO1;
        plan.geom = kIpcGeomV;
        const HcclResult r = RunIpcPlan(c, HCCL_AMD_OP_REDUCE_SCATTER, plan, sendBuf, recvBuf, counts[c.rank], dt, op,
                                        0, stream, counts, displs);
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = ipcOnly ? HCCL_AMD_ALGO_IPC : c.algoOverride;
            return r;
        }
        if (ipcOnly) return HCCL_E_NOT_SUPPORT;
    }
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_REDUCE_SCATTER_V;
    p.counts.assign(counts, counts + c.nRanks);
    p.displs.assign(displs, displs + c.nRanks);
    p.count = counts[c.rank];
    uint64_t payload = 0;
    for (uint32_t q = 0; q < c.nRanks; ++q) payload += counts[q] * DataTypeSize(dt);
    return RunSchedule(c, p, payload, sendBuf, recvBuf, dt, op, stream);
}

// The all-to-all family behind its three entry points: the V form with this rank's four arrays (elements). `known`:
// every rank knows the whole count matrix (AlltoAll, AlltoAllVC) and maxCount is its largest entry; otherwise
// (AlltoAllV) a rank knows its own row and column only. Selection uses only what is equal on every rank. Known matrix:
// the Broadcast's rule, with n x maxCount x es as the call's size. AlltoAllV: sizes are not common knowledge, so under
// AUTO the one-sided kernel runs whenever it is available (measured on one GPU only: DESIGN.md §5g). Data movement
// only, so no family has bits of its own: the schedule path is the one mesh schedule, also the fallback when the
// kernel cannot run (no peer mappings, a capture before the set-up).
HcclResult RunAlltoAll(Comm& c, const void* sendBuf, void* recvBuf, const uint64_t* sendCounts, const uint64_t* sdispls,
                       const uint64_t* recvCounts, const uint64_t* rdispls, HcclDataType dt, bool known,
                       uint64_t maxCount, int32_t checkOp, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    const uint32_t n = c.nRanks;
    const uint64_t es = DataTypeSize(dt);
    auto at = [es](const void* p, uint64_t off) { return static_cast<char*>(const_cast<void*>(p)) + off * es; };
    if (n == 1) {
        c.lastAlgo = HCCL_AMD_ALGO_AUTO;
        if (sendCounts[0] == 0) return HCCL_SUCCESS;
        return CopyUserBuffer(at(recvBuf, rdispls[0]), at(sendBuf, sdispls[0]), sendCounts[0] * es, stream);
    }
    // AlltoAll's record carries its sendCount; the V forms' records carry the data type only (FillCheckRecord)
    HCCL_CHK(CheckArgs(c, checkOp, 0, HCCL_REDUCE_SUM, dt, sendCounts[0], stream));
    const bool ipcOnly = !c.transport->HasSendRecv();
    const int32_t algo = c.algoOverride;
    const bool asked = algo == HCCL_AMD_ALGO_IPC || algo == HCCL_AMD_ALGO_IPC_TWOSHOT || algo == HCCL_AMD_ALGO_AIV ||
                       algo == HCCL_AMD_ALGO_AIV_ONLY;
    const bool byRule = algo == HCCL_AMD_ALGO_AUTO && !c.ipc.unavailable &&
                        (!known || uint64_t(n) * maxCount * es <= c.cfg.smallIpcBytes);
    if (n <= uint32_t(kIpcMaxRanks) && (ipcOnly || asked || byRule)) {
        IpcA2aTables t{};
        for (uint32_t q = 0; q < n; ++q) {
            t.v[kA2aSend][q] = sendCounts[q];
            t.v[kA2aSdispl][q] = sdispls[q];
            t.v[kA2aRecv][q] = recvCounts[q];
            t.v[kA2aRdispl][q] = rdispls[q];
        }
        const HcclResult r = RunIpcAllToAll(c, sendBuf, recvBuf, t, maxCount, !known, dt, stream);
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = HCCL_AMD_ALGO_IPC;
            return r;
        }
    }
    if (ipcOnly) return HCCL_E_NOT_SUPPORT;
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_ALLTOALL;
    p.algo = HCCL_AMD_ALGO_MESH_ONESHOT;
    p.counts.assign(sendCounts, sendCounts + n);
    p.displs.assign(sdispls, sdispls + n);
    p.recvCounts.assign(recvCounts, recvCounts + n);
    p.recvDispls.assign(rdispls, rdispls + n);
    p.count = sendCounts[c.rank];
    uint64_t payload = 0;
    for (uint32_t q = 0; q < n; ++q) payload += sendCounts[q] * es;
    return RunSchedule(c, p, payload, const_cast<void*>(sendBuf), recvBuf, dt, HCCL_REDUCE_SUM, stream);
}

// An all-to-all's blocks must be addressable: a count within SYS_MAX_COUNT and an end that fits in 64 bits.
HcclResult CheckA2aBlocks(const uint64_t* counts, const uint64_t* displs, uint32_t n)
{
    for (uint32_t q = 0; q < n; ++q) {
        if (displs[q] > UINT64_MAX / 16 - counts[q]) return HCCL_E_PARA;
    }
    return HCCL_SUCCESS;
}

// The selection Scatter and AllGatherV share with the Broadcast (data movement only, so no family has bits of its
// own): the one-sided kernel on an IPC-only communicator, when a one-sided family is asked for, and under AUTO for
// calls of at most HCCL_AMD_SMALL_IPC_BYTES (`bytes`, equal on every rank); the mesh schedule otherwise.
bool WantsOneSided(const Comm& c, uint64_t bytes)
{
    const int32_t algo = c.algoOverride;
    const bool asked = algo == HCCL_AMD_ALGO_IPC || algo == HCCL_AMD_ALGO_IPC_TWOSHOT || algo == HCCL_AMD_ALGO_AIV ||
                       algo == HCCL_AMD_ALGO_AIV_ONLY;
    const bool small = algo == HCCL_AMD_ALGO_AUTO && !c.ipc.unavailable && bytes <= c.cfg.smallIpcBytes;
    return c.nRanks <= uint32_t(kIpcMaxRanks) && (!c.transport->HasSendRecv() || asked || small);
}

// HcclScatter behind its checks (ins_temp_scatter_mesh_1D.cc). The size the rule looks at is the root's input,
// n x recvCount x es. Measured on one GPU only.
HcclResult RunScatter(Comm& c, void* sendBuf, void* recvBuf, uint64_t recvCount, HcclDataType dt, uint32_t root,
                      hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    const uint64_t es = DataTypeSize(dt);
    if (c.nRanks == 1) {
        c.lastAlgo = HCCL_AMD_ALGO_AUTO;
        return CopyUserBuffer(recvBuf, sendBuf, recvCount * es, stream);  // block 0
    }
    HCCL_CHK(CheckArgs(c, HCCL_AMD_OP_SCATTER, root, HCCL_REDUCE_SUM, dt, recvCount, stream));
    if (WantsOneSided(c, uint64_t(c.nRanks) * recvCount * es)) {
        const HcclResult r = RunIpcScatter(c, sendBuf, recvBuf, recvCount, dt, root, stream);
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = HCCL_AMD_ALGO_IPC;
            return r;
        }
    }
    if (!c.transport->HasSendRecv()) return HCCL_E_NOT_SUPPORT;
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_SCATTER;
    p.algo = HCCL_AMD_ALGO_MESH_ONESHOT;
    p.count = recvCount;
    p.root = root;
    // a rank other than the root has no record that reads its input, so a null sendBuf there is never addressed
    const uint64_t payload = (c.rank == root ? uint64_t(c.nRanks) : 1) * recvCount * es;
    return RunSchedule(c, p, payload, sendBuf, recvBuf, dt, HCCL_REDUCE_SUM, stream);
}

// HcclAllGatherV behind its checks (ins_temp_all_gather_v_mesh_1D.cc). The size the rule looks at is the output,
// sum(recvCounts) x es. Measured on one GPU only.
HcclResult RunAllGatherV(Comm& c, void* sendBuf, void* recvBuf, const uint64_t* counts, const uint64_t* displs,
                         HcclDataType dt, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    const uint32_t n = c.nRanks, me = c.rank;
    const uint64_t es = DataTypeSize(dt);
    char* own = static_cast<char*>(recvBuf) + displs[me] * es;
    if (n == 1) {
        c.lastAlgo = HCCL_AMD_ALGO_AUTO;
        return CopyUserBuffer(own, sendBuf, counts[0] * es, stream);
    }
    HCCL_CHK(CheckArgs(c, HCCL_AMD_OP_ALLGATHER_V, 0, HCCL_REDUCE_SUM, dt, 0, stream));
    uint64_t total = 0;
    for (uint32_t q = 0; q < n; ++q) total += counts[q] * es;
    if (WantsOneSided(c, total)) {
        const HcclResult r = RunIpcAllGatherV(c, sendBuf, recvBuf, counts, displs, dt, stream);
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = HCCL_AMD_ALGO_IPC;
            return r;
        }
    }
    if (!c.transport->HasSendRecv()) return HCCL_E_NOT_SUPPORT;
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_ALLGATHER_V;
    p.algo = HCCL_AMD_ALGO_MESH_ONESHOT;
    p.counts.assign(counts, counts + n);
    p.displs.assign(displs, displs + n);
    p.count = counts[me];
    p.inPlace = counts[me] != 0 && sendBuf == own;
    return RunSchedule(c, p, counts[me] * es, sendBuf, recvBuf, dt, HCCL_REDUCE_SUM, stream);
}

// HcclBarrier behind its checks. Always a "small call" (WantsOneSided of 0 bytes): the one-sided kernel on an IPC-only
// communicator, when a one-sided family is asked for, and under AUTO whenever the one-sided path is available; the
// token schedule on the transport otherwise, and when the one-sided path reports NOT_SUPPORT, as RunScatter falls back.
HcclResult RunBarrier(Comm& c, hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());
    if (c.nRanks == 1) {  // barrier_op.cc:137-140: returns directly, nothing is enqueued
        c.lastAlgo = HCCL_AMD_ALGO_AUTO;
        return HCCL_SUCCESS;
    }
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    HCCL_CHK(CheckArgs(c, HCCL_AMD_OP_BARRIER, 0, HCCL_REDUCE_SUM, HCCL_DATA_TYPE_RESERVED, 0, stream));
    if (WantsOneSided(c, 0)) {
        const HcclResult r = RunIpcBarrier(c, stream);
        if (r != HCCL_E_NOT_SUPPORT) {
            c.lastAlgo = HCCL_AMD_ALGO_IPC;
            return r;
        }
    }
    if (!c.transport->HasSendRecv()) return HCCL_E_NOT_SUPPORT;
    HCCL_CHK(c.EnsureBarrierTokens());
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_BARRIER;
    p.algo = c.algoOverride;  // the two mesh families: Mesh1D; every other one: NHR (ResolveAlgo)
    char* tokens = static_cast<char*>(c.barrierTokens);
    // the outgoing tokens and the incoming ones: halves of one allocation, so no record aliases another
    return RunSchedule(c, p, 0, tokens, tokens + Comm::kBarrierTokenBytes / 2, HCCL_DATA_TYPE_INT8, HCCL_REDUCE_SUM,
                       stream);
}

// HcclSend / HcclRecv / HcclBatchSendRecv behind their checks: the self pairs are local copies, the remote items one
// group. One-sided (k_ipc_p2p) once HcclAmdCommEnableP2p has succeeded and the rule Scatter uses says so for the
// call's largest item; that threshold was measured for collectives, not for point-to-point. Otherwise
// one Transport::Group of the user buffers, which RCCL's group makes deadlock-free whatever the batch holds.
struct SelfCopy {
    void* dst;
    const void* src;
    uint64_t bytes;
};

HcclResult RunP2p(Comm& c, const std::vector<P2pOp>& ops, const std::vector<SelfCopy>& self, uint64_t es,
                  hipStream_t stream)
{
    const HostProfileScope hp(HCCL_AMD_HP_ENTRY);
    std::lock_guard<std::mutex> lk(c.mu);
    HCCL_CHK(c.Gate());
    HIP_CHK(hipSetDevice(c.device));
    const EntryScope entry(c, stream);
    HCCL_CHK(entry.status());
    c.lastAlgo = HCCL_AMD_ALGO_AUTO;
    for (const SelfCopy& k : self) HCCL_CHK(CopyUserBuffer(k.dst, k.src, k.bytes, stream));
    if (ops.empty()) return HCCL_SUCCESS;
    uint64_t largest = 0;
    for (const P2pOp& o : ops) largest = std::max(largest, o.bytes);
    if (c.ipc.p2p.ready && WantsOneSided(c, largest)) {
        const HcclResult r = RunIpcP2p(c, ops, es, stream);
        // a list too long for one launch is refused aloud: its peers would not follow it to the other path
        if (r != HCCL_E_NOT_SUPPORT || ops.size() > kP2pMaxItems) {
            c.lastAlgo = HCCL_AMD_ALGO_IPC;
            return r;
        }
    }
    if (!c.transport->HasSendRecv()) return HCCL_E_NOT_SUPPORT;
    if (c.transport->SelfLoop()) {
        // the stand-in hands every receive this rank's own send of the same size: anything else cannot run there
        std::vector<uint64_t> sends, recvs;
        for (const P2pOp& o : ops) (o.isSend ? sends : recvs).push_back(o.bytes);
        std::sort(sends.begin(), sends.end());
        std::sort(recvs.begin(), recvs.end());
        if (sends != recvs) return HCCL_E_NOT_SUPPORT;
    }
    if (entry.captured() && c.transport->SharedDevice()) return HCCL_E_NOT_SUPPORT;  // as Execute
    const WatchScope watch(entry.captured() ? nullptr : c.watchdog.get(), stream, false);
    c.lastAlgo = HCCL_AMD_ALGO_MESH_ONESHOT;
    return c.transport->Group(ops, stream);
}

// The checks HcclSend and HcclRecv share (send_op.cc:126-150, recv_op.cc), behind count == 0.
HcclResult SendRecvOne(bool isSend, void* buf, uint64_t count, HcclDataType dt, uint32_t peer, HcclComm comm,
                       aclrtStream stream)
{
    if (comm == nullptr || buf == nullptr || stream == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    HCCL_CHK(CheckCount(count));
    // CheckDataType(dataType, needReduce = false): every valid type but INT128
    if (DataTypeSize(dt) == 0 || dt == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    if (peer == c->rank) return HCCL_E_NOT_SUPPORT;
    if (c->rank >= c->nRanks || peer >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    const uint64_t es = DataTypeSize(dt);
    return RunP2p(*c, {P2pOp{isSend, peer, buf, count * es}}, {}, es, static_cast<hipStream_t>(stream));
}

// Rows of nRanks entries (a ring or RHD table) into the caller's array, `capacity` rows at most; returns the row count.
int32_t FlattenTable(const std::vector<std::vector<uint32_t>>& t, uint32_t nRanks, uint32_t* out, uint32_t capacity)
{
    for (uint32_t k = 0; out != nullptr && k < t.size() && k < capacity; ++k) {
        std::memcpy(out + size_t(k) * nRanks, t[k].data(), nRanks * sizeof(uint32_t));
    }
    return static_cast<int32_t>(t.size());
}

// Builds p's schedule with the default staging and CCL sizes and hands it to the caller (HcclAmdBuildSchedule[V]).
HcclResult BuildAndCopyOut(ScheduleParams& p, HcclAmdIrOp* ops, uint64_t capacity, uint64_t* numOps, int32_t* algoUsed,
                           uint64_t* scratchElems)
{
    p.scratchCapBytes = ScratchBytesDefault();
    p.cclBytes = CclBytesDefault();
    Schedule s;
    HcclResult r = static_cast<HcclResult>(BuildSchedule(p, &s));
    if (r != HCCL_SUCCESS) return r;
    *numOps = s.ops.size();
    if (algoUsed != nullptr) *algoUsed = s.algo;
    if (scratchElems != nullptr) *scratchElems = s.scratchElems;
    if (ops != nullptr) {
        if (capacity < s.ops.size()) return HCCL_E_PARA;
        std::memcpy(ops, s.ops.data(), s.ops.size() * sizeof(HcclAmdIrOp));
    }
    return HCCL_SUCCESS;
}

}  // namespace

}  // namespace hccl_amd

using namespace hccl_amd;

extern "C" {

// ------------------------------------------------------------------------------------------------ operators

HcclResult HcclAllReduce(void* sendBuf, void* recvBuf, uint64_t count, HcclDataType dataType, HcclReduceOp op,
                         HcclComm comm, aclrtStream stream)
{
    if (count == 0) return HCCL_SUCCESS;  // all_reduce_op.cc:37
    if (stream == nullptr || comm == nullptr || sendBuf == nullptr || recvBuf == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    HCCL_CHK(CheckCount(count));
    HCCL_CHK(CheckReduceDataType(dataType));
    HCCL_CHK(CheckReduceOp(dataType, op));
    return RunCollective(*c, HCCL_AMD_OP_ALLREDUCE, sendBuf, recvBuf, count, dataType, op, 0,
                         static_cast<hipStream_t>(stream));
}

HcclResult HcclReduceScatter(void* sendBuf, void* recvBuf, uint64_t recvCount, HcclDataType dataType,
                             HcclReduceOp op, HcclComm comm, aclrtStream stream)
{
    if (recvCount == 0) return HCCL_SUCCESS;  // reduce_scatter_op.cc:47
    if (stream == nullptr || comm == nullptr || sendBuf == nullptr || recvBuf == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;
    HCCL_CHK(CheckCount(recvCount));
    HCCL_CHK(CheckReduceDataType(dataType));
    HCCL_CHK(CheckReduceOp(dataType, op));
    return RunCollective(*c, HCCL_AMD_OP_REDUCE_SCATTER, sendBuf, recvBuf, recvCount, dataType, op, 0,
                         static_cast<hipStream_t>(stream));
}

HcclResult HcclReduceScatterV(void* sendBuf, const void* sendCounts, const void* sendDispls, void* recvBuf,
                              uint64_t recvCount, HcclDataType dataType, HcclReduceOp op, HcclComm comm,
                              aclrtStream stream)
{
    // CheckReduceScatterVInputParam (reduce_scatter_v_op.cc:155-183): stream, comm, sendCounts, sendDispls, then
    // recvBuf when recvCount > 0 (sendBuf is not checked there: a rank may send nothing)
    if (stream == nullptr || comm == nullptr || sendCounts == nullptr || sendDispls == nullptr) return HCCL_E_PTR;
    if (recvCount > 0 && recvBuf == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    const uint64_t* counts = static_cast<const uint64_t*>(sendCounts);
    const uint64_t* displs = static_cast<const uint64_t*>(sendDispls);
    bool any = false;
    for (uint32_t q = 0; q < c->nRanks; ++q) any = any || counts[q] != 0;
    if (!any) return HCCL_SUCCESS;  // every sendCounts entry 0: success (:45-53)
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    HCCL_CHK(CheckCount(recvCount));
    HCCL_CHK(CheckReduceDataType(dataType));
    HCCL_CHK(CheckReduceOp(dataType, op));
    for (uint32_t q = 0; q < c->nRanks; ++q) {
        HCCL_CHK(CheckCount(counts[q]));
        // a block whose end does not fit in 64 bits would wrap the schedule's offsets onto other memory
        if (displs[q] > UINT64_MAX / 16 - counts[q]) return HCCL_E_PARA;
    }
    // The template writes sendCounts[rank] elements to recvBuf (PostCopy, ins_temp_reduce_scatter_v_mesh_1D.cc:
    // 107-146); a smaller recvCount would overrun it, so it is refused here (the reference has no such check).
    if (counts[c->rank] > recvCount) return HCCL_E_PARA;
    if (sendBuf == nullptr) return HCCL_E_PTR;  // some rank's block is non-empty: the input is read
    return RunReduceScatterV(*c, sendBuf, counts, displs, recvBuf, dataType, op, static_cast<hipStream_t>(stream));
}

HcclResult HcclReduce(void* sendBuf, void* recvBuf, uint64_t count, HcclDataType dataType, HcclReduceOp op,
                      uint32_t root, HcclComm comm, aclrtStream stream)
{
    if (count == 0) return HCCL_SUCCESS;  // reduce_op.cc:42
    // CheckReduceInputPara order: comm, sendBuf, recvBuf, stream (reduce_op.cc:106-127)
    if (comm == nullptr || sendBuf == nullptr || recvBuf == nullptr || stream == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    HCCL_CHK(CheckCount(count));
    HCCL_CHK(CheckReduceDataType(dataType));
    HCCL_CHK(CheckReduceOp(dataType, op));
    if (root >= c->nRanks) return HCCL_E_PARA;     // HcomCheckUserRank(rankSize, root)
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank(rankSize, userRank)
    return RunCollective(*c, HCCL_AMD_OP_REDUCE, sendBuf, recvBuf, count, dataType, op, root,
                         static_cast<hipStream_t>(stream));
}

HcclResult HcclAllGather(void* sendBuf, void* recvBuf, uint64_t sendCount, HcclDataType dataType, HcclComm comm,
                         aclrtStream stream)
{
    // all_gather_op.cc:22-50, AllGatherInitAndCheck :97-122
    if (sendCount == 0) return HCCL_SUCCESS;
    if (stream == nullptr || comm == nullptr || sendBuf == nullptr || recvBuf == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    HCCL_CHK(CheckCount(sendCount));
    // CheckDataType(dataType, needReduce = false): every valid type but INT128
    if (DataTypeSize(dataType) == 0 || dataType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;
    return RunCollective(*c, HCCL_AMD_OP_ALLGATHER, sendBuf, recvBuf, sendCount, dataType, HCCL_REDUCE_SUM, 0,
                         static_cast<hipStream_t>(stream));
}

HcclResult HcclBroadcast(void* buf, uint64_t count, HcclDataType dataType, uint32_t root, HcclComm comm,
                         aclrtStream stream)
{
    // broadcast_op.cc:23-50, BroadcastInitAndCheck :99-123, CheckBroadcastInputPara :125-142
    if (count == 0) return HCCL_SUCCESS;
    if (comm == nullptr || buf == nullptr || stream == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank(rankSize, userRank)
    if (root >= c->nRanks) return HCCL_E_PARA;     // HcomCheckUserRank(rankSize, root)
    HCCL_CHK(CheckCount(count));
    // CheckDataType(dataType, needReduce = false): every valid type but INT128
    if (DataTypeSize(dataType) == 0 || dataType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    return RunCollective(*c, HCCL_AMD_OP_BROADCAST, buf, buf, count, dataType, HCCL_REDUCE_SUM, root,
                         static_cast<hipStream_t>(stream));
}

HcclResult HcclScatter(void* sendBuf, void* recvBuf, uint64_t recvCount, HcclDataType dataType, uint32_t root,
                       HcclComm comm, aclrtStream stream)
{
    // scatter_op.cc:70-84, CheckScatterInputPara :126-139
    if (recvCount == 0) return HCCL_SUCCESS;
    if (comm == nullptr || recvBuf == nullptr || stream == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank == root && sendBuf == nullptr) return HCCL_E_PTR;  // read on the root only
    if (root >= c->nRanks) return HCCL_E_PARA;                     // HcomCheckUserRank(rankSize, root)
    HCCL_CHK(CheckCount(recvCount));
    // CheckDataType(dataType, needReduce = false): every valid type but INT128
    if (DataTypeSize(dataType) == 0 || dataType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    return RunScatter(*c, sendBuf, recvBuf, recvCount, dataType, root, static_cast<hipStream_t>(stream));
}

HcclResult HcclAllGatherV(void* sendBuf, uint64_t sendCount, void* recvBuf, const void* recvCounts,
                          const void* recvDispls, HcclDataType dataType, HcclComm comm, aclrtStream stream)
{
    // all_gather_v_op.cc:40-54, CheckAllGatherVInputPara :136-162, CheckAllGatherVRecvAndGetRank :166-188
    if (comm == nullptr || recvCounts == nullptr || recvDispls == nullptr || stream == nullptr) return HCCL_E_PTR;
    if (sendCount > 0 && sendBuf == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    const uint32_t n = c->nRanks;
    const uint64_t* counts = static_cast<const uint64_t*>(recvCounts);
    const uint64_t* displs = static_cast<const uint64_t*>(recvDispls);
    if (std::all_of(counts, counts + n, [](uint64_t x) { return x == 0; })) return HCCL_SUCCESS;
    if (recvBuf == nullptr) return HCCL_E_PTR;
    if (c->rank >= n) return HCCL_E_PARA;  // HcomCheckUserRank
    HCCL_CHK(CheckCount(sendCount));
    if (DataTypeSize(dataType) == 0 || dataType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    // no reference counterpart (hccl.h): this rank's two statements of its own block agree, and every block is
    // addressable
    if (sendCount != counts[c->rank]) return HCCL_E_PARA;
    for (uint32_t q = 0; q < n; ++q) HCCL_CHK(CheckCount(counts[q]));
    HCCL_CHK(CheckA2aBlocks(counts, displs, n));
    // a rank with nothing to send still takes part: its peers wait for it
    return RunAllGatherV(*c, sendBuf, recvBuf, counts, displs, dataType, static_cast<hipStream_t>(stream));
}

HcclResult HcclBarrier(HcclComm comm, aclrtStream stream)
{
    // CheckBarrierInputPara (barrier_op.cc:91-102): the stream first, then the communicator
    if (stream == nullptr) return HCCL_E_PTR;
    if (comm == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    return RunBarrier(*c, static_cast<hipStream_t>(stream));
}

HcclResult HcclSend(void* sendBuf, uint64_t count, HcclDataType dataType, uint32_t destRank, HcclComm comm,
                    aclrtStream stream)
{
    if (count == 0) return HCCL_SUCCESS;  // send_op.cc:33
    return SendRecvOne(true, sendBuf, count, dataType, destRank, comm, stream);
}

HcclResult HcclRecv(void* recvBuf, uint64_t count, HcclDataType dataType, uint32_t srcRank, HcclComm comm,
                    aclrtStream stream)
{
    if (count == 0) return HCCL_SUCCESS;
    return SendRecvOne(false, recvBuf, count, dataType, srcRank, comm, stream);
}

HcclResult HcclBatchSendRecv(HcclSendRecvItem* sendRecvInfo, uint32_t itemNum, HcclComm comm, aclrtStream stream)
{
    // batch_send_recv_op.cc:39-56, CheckBatchSendRecvInputPara :73-93
    if (itemNum == 0) return HCCL_SUCCESS;
    if (stream == nullptr || comm == nullptr || sendRecvInfo == nullptr) return HCCL_E_PTR;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    for (uint32_t i = 0; i < itemNum; ++i) {
        HCCL_CHK(CheckCount(sendRecvInfo[i].count));
        const HcclDataType dt = sendRecvInfo[i].dataType;
        if (DataTypeSize(dt) == 0 || dt == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    }
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    for (uint32_t i = 0; i < itemNum; ++i) {
        if (sendRecvInfo[i].remoteRank >= c->nRanks) return HCCL_E_PARA;
    }
    // GetPairWiseList (ins_v2_batch_send_recv_executor.cc:136-208)
    std::vector<uint32_t> order(itemNum);
    uint32_t sends = 0, recvs = 0, pairs = 0;
    HCCL_CHK(BatchSendRecvOrder(sendRecvInfo, itemNum, c->rank, c->nRanks, order.data(), &sends, &recvs, &pairs));
    std::vector<P2pOp> ops;
    uint64_t es = 8;  // the kernel's element: the smallest of the items' (pieces and windows are whole bytes alike)
    for (uint32_t k = 0; k < sends + recvs; ++k) {
        const HcclSendRecvItem& it = sendRecvInfo[order[k]];
        const uint64_t e = DataTypeSize(it.dataType);
        es = std::min(es, e);
        ops.push_back({k < sends, it.remoteRank, it.buf, it.count * e});
    }
    std::vector<SelfCopy> self;
    for (uint32_t k = 0; k < pairs; ++k) {
        const HcclSendRecvItem& s = sendRecvInfo[order[sends + recvs + 2 * k]];
        const HcclSendRecvItem& r = sendRecvInfo[order[sends + recvs + 2 * k + 1]];
        if (DataTypeSize(s.dataType) != DataTypeSize(r.dataType)) return HCCL_E_PARA;
        self.push_back({r.buf, s.buf, s.count * DataTypeSize(s.dataType)});
    }
    return RunP2p(*c, ops, self, es, static_cast<hipStream_t>(stream));
}

HcclResult HcclAlltoAll(const void* sendBuf, uint64_t sendCount, HcclDataType sendType, const void* recvBuf,
                        uint64_t recvCount, HcclDataType recvType, HcclComm comm, aclrtStream stream)
{
    // all_to_all_v_op.cc:38-56, CheckAlltoAllInputPara :456-493
    if (sendCount == 0 && recvCount == 0) return HCCL_SUCCESS;
    if (comm == nullptr || sendBuf == nullptr || recvBuf == nullptr) return HCCL_E_PTR;
    if (sendCount != recvCount || sendType != recvType) return HCCL_E_PARA;
    if (stream == nullptr) return HCCL_E_PTR;
    if (sendBuf == recvBuf) return HCCL_E_PARA;
    const uint64_t es = DataTypeSize(sendType);
    if (es != 0 && sendCount > UINT64_MAX / es) return HCCL_E_PARA;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    HCCL_CHK(CheckCount(recvCount));
    // CheckDataType(recvType, needReduce = false): every valid type but INT128
    if (es == 0 || recvType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    // ConvertAlltoAllParam (:407-417): the V form with counts recvCount and displacements q * recvCount
    const uint32_t n = c->nRanks;
    std::vector<uint64_t> counts(n, recvCount), displs(n);
    for (uint32_t q = 0; q < n; ++q) displs[q] = uint64_t(q) * recvCount;
    return RunAlltoAll(*c, sendBuf, const_cast<void*>(recvBuf), counts.data(), displs.data(), counts.data(),
                       displs.data(), recvType, true, recvCount, HCCL_AMD_OP_ALLTOALL,
                       static_cast<hipStream_t>(stream));
}

HcclResult HcclAlltoAllV(const void* sendBuf, const void* sendCounts, const void* sdispls, HcclDataType sendType,
                         const void* recvBuf, const void* recvCounts, const void* rdispls, HcclDataType recvType,
                         HcclComm comm, aclrtStream stream)
{
    // CheckAlltoAllVInputPara (all_to_all_v_op.cc:495-531)
    if (comm == nullptr || sendCounts == nullptr || sdispls == nullptr || recvCounts == nullptr ||
        rdispls == nullptr || stream == nullptr) {
        return HCCL_E_PTR;
    }
    if (sendBuf != nullptr && sendBuf == recvBuf) return HCCL_E_PARA;
    // no reference counterpart (it ignores sendType): nothing is converted, so the types must agree (hccl.h)
    if (sendType != recvType) return HCCL_E_PARA;
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    const uint32_t n = c->nRanks;
    const uint64_t* sc = static_cast<const uint64_t*>(sendCounts);
    const uint64_t* rc = static_cast<const uint64_t*>(recvCounts);
    // CheckBufNullptr (:558-576): a null buffer is legal only when all of its counts are 0
    uint64_t maxSend = 0, maxRecv = 0;
    for (uint32_t q = 0; q < n; ++q) {
        maxSend = std::max(maxSend, sc[q]);
        maxRecv = std::max(maxRecv, rc[q]);
    }
    if (maxSend != 0 && sendBuf == nullptr) return HCCL_E_PTR;
    if (maxRecv != 0 && recvBuf == nullptr) return HCCL_E_PTR;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    HCCL_CHK(CheckCount(std::max(maxSend, maxRecv)));
    if (DataTypeSize(recvType) == 0 || recvType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    HCCL_CHK(CheckA2aBlocks(sc, static_cast<const uint64_t*>(sdispls), n));
    HCCL_CHK(CheckA2aBlocks(rc, static_cast<const uint64_t*>(rdispls), n));
    // no early return for an all-zero row and column: the peers may still exchange data among themselves, and this
    // rank takes part in their barriers
    return RunAlltoAll(*c, sendBuf, const_cast<void*>(recvBuf), sc, static_cast<const uint64_t*>(sdispls), rc,
                       static_cast<const uint64_t*>(rdispls), recvType, false, 0, HCCL_AMD_CHECK_OP_ALLTOALLV,
                       static_cast<hipStream_t>(stream));
}

HcclResult HcclAlltoAllVC(const void* sendBuf, const void* sendCountMatrix, HcclDataType sendType, const void* recvBuf,
                          HcclDataType recvType, HcclComm comm, aclrtStream stream)
{
    // CheckAlltoAllVCInputPara (all_to_all_v_op.cc:533-556)
    if (comm == nullptr || sendCountMatrix == nullptr || stream == nullptr) return HCCL_E_PTR;
    if (sendBuf != nullptr && sendBuf == recvBuf) return HCCL_E_PARA;
    if (sendType != recvType) return HCCL_E_PARA;  // as HcclAlltoAllV
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PARA;
    if (c->rank >= c->nRanks) return HCCL_E_PARA;  // HcomCheckUserRank
    // ConvertAlltoAllVCParam (:419-454): row `rank` = send counts, column `rank` = receive counts, packed prefix sums
    const uint32_t n = c->nRanks, me = c->rank;
    const uint64_t* m = static_cast<const uint64_t*>(sendCountMatrix);
    uint64_t maxCount = 0;
    for (uint64_t i = 0; i < uint64_t(n) * n; ++i) maxCount = std::max(maxCount, m[i]);
    HCCL_CHK(CheckCount(maxCount));
    std::vector<uint64_t> sc(n), sd(n), rc(n), rd(n);
    uint64_t so = 0, ro = 0;
    for (uint32_t q = 0; q < n; ++q) {
        sc[q] = m[uint64_t(me) * n + q];
        sd[q] = so;
        so += sc[q];
        rc[q] = m[uint64_t(q) * n + me];
        rd[q] = ro;
        ro += rc[q];
    }
    if (so != 0 && sendBuf == nullptr) return HCCL_E_PTR;  // CheckBufNullptr
    if (ro != 0 && recvBuf == nullptr) return HCCL_E_PTR;
    if (DataTypeSize(recvType) == 0 || recvType == HCCL_DATA_TYPE_INT128) return HCCL_E_NOT_SUPPORT;
    return RunAlltoAll(*c, sendBuf, const_cast<void*>(recvBuf), sc.data(), sd.data(), rc.data(), rd.data(), recvType,
                       true, maxCount, HCCL_AMD_CHECK_OP_ALLTOALLVC, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ communicators

static const char kRootMagic[8] = {'H', 'C', 'C', 'L', 'A', 'M', 'D', '1'};

HcclResult HcclGetRootInfo(HcclRootInfo* rootInfo)
{
    if (rootInfo == nullptr) return HCCL_E_PTR;
    std::memset(rootInfo->internal, 0, sizeof rootInfo->internal);
    std::memcpy(rootInfo->internal, kRootMagic, sizeof kRootMagic);
    return RcclGetUniqueId(rootInfo->internal + 8);
}

HcclResult HcclCommInitRootInfo(uint32_t nRanks, const HcclRootInfo* rootInfo, uint32_t rank, HcclComm* comm)
{
    if (rootInfo == nullptr || comm == nullptr) return HCCL_E_PTR;
    if (nRanks == 0 || rank >= nRanks || nRanks > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    if (std::memcmp(rootInfo->internal, kRootMagic, sizeof kRootMagic) != 0) return HCCL_E_PARA;
    int dev = 0;
    HIP_CHK(hipGetDevice(&dev));
    auto c = std::make_unique<Comm>();
    c->rank = rank;
    c->nRanks = nRanks;
    HCCL_CHK(c->Init(dev));
    HcclResult err = HCCL_SUCCESS;
    c->transport = MakeRcclTransport(const_cast<char*>(rootInfo->internal + 8), nRanks, rank, &err);
    if (c->transport == nullptr) return err == HCCL_SUCCESS ? HCCL_E_INTERNAL : err;
    HCCL_CHK(c->StartWatchdog());
    *comm = c.release();
    return HCCL_SUCCESS;
}

HcclResult HcclCommDestroy(HcclComm comm)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    c->magic = 0;  // no further use through this handle, whether torn down now or later
    // A graph captured on this communicator still holds its staging and RCCL plans, and ncclCommDestroy would wait
    // for that graph to be destroyed: the teardown then runs when the last such graph goes (watchdog.cc).
    if (DeferDestroy(c)) return HCCL_SUCCESS;
    delete c;
    return HCCL_SUCCESS;
}

HcclResult HcclGetCommAsyncError(HcclComm comm, HcclResult* asyncError)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || asyncError == nullptr) return HCCL_E_PTR;
    *asyncError = c->PollAsyncError();  // lock-free: a watchdog thread never waits behind a collective
    return HCCL_SUCCESS;
}

uint64_t HcclAmdIpcTimeoutMs(void) { return IpcTimeoutTicks() / 100000; }

HcclResult HcclGetRankSize(HcclComm comm, uint32_t* rankSize)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || rankSize == nullptr) return HCCL_E_PTR;
    *rankSize = c->nRanks;
    return HCCL_SUCCESS;
}

HcclResult HcclGetRankId(HcclComm comm, uint32_t* rank)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || rank == nullptr) return HCCL_E_PTR;
    *rank = c->rank;
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommInitLoopback(uint32_t nRanks, HcclComm* comms)
{
    if (comms == nullptr) return HCCL_E_PTR;
    if (nRanks == 0 || nRanks > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    int dev = 0;
    HIP_CHK(hipGetDevice(&dev));
    auto world = MakeLoopbackWorld(nRanks);
    std::vector<std::unique_ptr<Comm>> made;
    for (uint32_t r = 0; r < nRanks; ++r) {
        auto c = std::make_unique<Comm>();
        c->rank = r;
        c->nRanks = nRanks;
        HCCL_CHK(c->Init(dev));
        c->transport = MakeLoopbackTransport(world, r);
        made.push_back(std::move(c));
    }
    for (uint32_t r = 0; r < nRanks; ++r) comms[r] = made[r].release();
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommInitHostExchange(uint32_t nRanks, uint32_t rank, HcclAmdHostAllGatherFn fn, void* ctx,
                                       HcclComm* comm)
{
    if (fn == nullptr || comm == nullptr) return HCCL_E_PTR;
    if (nRanks == 0 || rank >= nRanks || nRanks > kIpcMaxRanks) return HCCL_E_PARA;
    int dev = 0;
    HIP_CHK(hipGetDevice(&dev));
    auto c = std::make_unique<Comm>();
    c->rank = rank;
    c->nRanks = nRanks;
    HCCL_CHK(c->Init(dev));
    c->transport = MakeHostExchangeTransport(fn, ctx);
    c->algoOverride = HCCL_AMD_ALGO_IPC_TWOSHOT;
    *comm = c.release();
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommInitSelfLoop(uint32_t nRanks, uint32_t rank, HcclComm* comm)
{
    if (comm == nullptr) return HCCL_E_PTR;
    if (nRanks == 0 || rank >= nRanks || nRanks > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    int dev = 0;
    HIP_CHK(hipGetDevice(&dev));
    auto c = std::make_unique<Comm>();
    c->rank = rank;
    c->nRanks = nRanks;
    HCCL_CHK(c->Init(dev));
    HcclResult err = HCCL_SUCCESS;
    c->transport = MakeRcclSelfLoopTransport(&err);
    if (c->transport == nullptr) return err == HCCL_SUCCESS ? HCCL_E_INTERNAL : err;
    c->ipc.unavailable = true;  // no peers to map: the one-sided kernel answers NOT_SUPPORT
    HCCL_CHK(c->StartWatchdog());
    *comm = c.release();
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommSetAlgo(HcclComm comm, int32_t algo)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    if (algo < HCCL_AMD_ALGO_AUTO || algo > HCCL_AMD_ALGO_IPC_RHD) return HCCL_E_PARA;
    c->algoOverride = algo;
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommSetIpcBlocks(HcclComm comm, uint32_t blocks)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    if (blocks > kIpcMaxBlocks) return HCCL_E_PARA;
    c->ipcBlocks = blocks;
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommSetBroadcastKind(HcclComm comm, int32_t kind)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    if (kind < 0 || kind > 2) return HCCL_E_PARA;
    c->bcastKind = kind;
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommSetPieceBytes(HcclComm comm, uint64_t pieceBytes)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    c->pieceBytes = pieceBytes;
    return HCCL_SUCCESS;
}

int32_t HcclAmdCommLastAlgo(HcclComm comm)
{
    Comm* c = AsComm(comm);
    return c == nullptr ? -1 : c->lastAlgo;
}

HcclResult HcclAmdCommSetConfig(HcclComm comm, int32_t key, int64_t value)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    return SetConfigEntry(c->cfg, key, value);
}

HcclResult HcclAmdCommReloadConfig(HcclComm comm)
{
    Comm* c = AsComm(comm);
    if (c == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    c->cfg = ReadCommConfig();
    return HCCL_SUCCESS;
}

HcclResult HcclAmdCommGetConfig(HcclComm comm, int32_t key, int64_t* value)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || value == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    return GetConfigEntry(c->cfg, key, value);
}

HcclResult HcclAmdCommDeviceBytes(HcclComm comm, uint64_t* bytes)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || bytes == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    *bytes = c->DeviceBytes();
    return HCCL_SUCCESS;
}

HcclResult HcclAmdIpcIdleStaging(int32_t release, uint64_t* bytes)
{
    if (bytes == nullptr) return HCCL_E_PTR;
    *bytes = IpcIdleBytes();
    // Freeing memory allocated with hipDeviceMallocUncached corrupts later GPU work on this stack (DESIGN.md §5b, item
    // 5; profiles/r06_release_stress.txt): the idle blocks stay with the process.
    return release != 0 ? HCCL_E_NOT_SUPPORT : HCCL_SUCCESS;
}

HcclResult HcclAmdCommScratch(HcclComm comm, void** ptr, uint64_t* bytes)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || ptr == nullptr || bytes == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    *ptr = c->scratch;
    *bytes = c->scratch != nullptr ? c->scratchBytes : 0;
    return HCCL_SUCCESS;
}

HcclResult HcclAmdRcclP2pChannels(uint32_t* perPeer, uint32_t* minP2pChannels)
{
    if (perPeer == nullptr || minP2pChannels == nullptr) return HCCL_E_PTR;
    RcclP2pChannels(perPeer, minP2pChannels);
    return HCCL_SUCCESS;
}

HcclResult HcclAmdL2Maintain(aclrtStream stream) { return ScrubL2(static_cast<hipStream_t>(stream)); }

HcclResult HcclAmdCommExecute(HcclComm comm,const HcclAmdIrOp* ops, uint64_t numOps, void* sendBuf, void* recvBuf,
                              HcclDataType dataType, HcclReduceOp op, int32_t singleStream, aclrtStream stream)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || stream == nullptr || (ops == nullptr && numOps != 0)) return HCCL_E_PTR;
    HCCL_CHK(CheckReduceDataType(dataType));
    HCCL_CHK(CheckReduceOp(dataType, op));
    const uint64_t es = DataTypeSize(dataType);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->scratch == nullptr) {
        // no staging until a program asks for it
        for (uint64_t i = 0; i < numOps; ++i) {
            bool uses = ops[i].kind != HCCL_AMD_IR_SEND && ops[i].dstBuf == HCCL_AMD_BUF_SCRATCH;
            for (int j = 0; j < ops[i].nsrc && j < HCCL_AMD_IR_MAX_SRC; ++j) {
                uses = uses || ops[i].srcBuf[j] == HCCL_AMD_BUF_SCRATCH;
            }
            if (uses) {
                HCCL_CHK(c->EnsureScratch());
                break;
            }
        }
    }
    // Every record must be well formed; staging references must lie inside the communicator's staging (the user
    // buffers' extents are the caller's contract, as for the collectives).
    auto bufOk = [&](int32_t b, uint64_t off, uint64_t cnt) {
        if (b == HCCL_AMD_BUF_INPUT) return sendBuf != nullptr;
        if (b == HCCL_AMD_BUF_OUTPUT) return recvBuf != nullptr;
        if (b != HCCL_AMD_BUF_SCRATCH || c->scratch == nullptr) return false;
        return off <= c->scratchBytes / es && cnt <= c->scratchBytes / es - off;
    };
    for (uint64_t i = 0; i < numOps; ++i) {
        const HcclAmdIrOp& o = ops[i];
        const bool p2p = o.kind == HCCL_AMD_IR_SEND || o.kind == HCCL_AMD_IR_RECV;
        if (o.kind < HCCL_AMD_IR_COPY || o.kind > HCCL_AMD_IR_RECV) return HCCL_E_PARA;
        if (p2p && (o.peer < 0 || static_cast<uint32_t>(o.peer) >= c->nRanks)) return HCCL_E_PARA;
        const int32_t wantSrc = o.kind == HCCL_AMD_IR_RECV ? 0 : (o.kind == HCCL_AMD_IR_REDUCE ? -1 : 1);
        if ((wantSrc >= 0 && o.nsrc != wantSrc) || (wantSrc < 0 && (o.nsrc < 1 || o.nsrc > HCCL_AMD_IR_MAX_SRC))) {
            return HCCL_E_PARA;
        }
        if (o.kind != HCCL_AMD_IR_SEND && !bufOk(o.dstBuf, o.dstOff, o.count)) return HCCL_E_PARA;
        for (int j = 0; j < o.nsrc; ++j) {
            if (!bufOk(o.srcBuf[j], o.srcOff[j], o.count)) return HCCL_E_PARA;
        }
    }
    HCCL_CHK(c->Gate());
    HIP_CHK(hipSetDevice(c->device));
    const EntryScope entry(*c, static_cast<hipStream_t>(stream));
    HCCL_CHK(entry.status());
    void* bufs[3] = {sendBuf, recvBuf, c->scratch};
    const CompiledSchedule* cs = nullptr;
    HCCL_CHK(CompileProgram(*c, ops, numOps, static_cast<uint32_t>(es), bufs, &cs));
    return RunCompiled(*c, *cs, bufs, dataType, op, static_cast<hipStream_t>(stream), singleStream != 0);
}

HcclResult HcclAmdCommCompileStats(HcclComm comm, uint64_t* hits, uint64_t* misses)
{
    Comm* c = AsComm(comm);
    if (c == nullptr || hits == nullptr || misses == nullptr) return HCCL_E_PTR;
    std::lock_guard<std::mutex> lk(c->mu);
    *hits = c->compileHits;
    *misses = c->compileMisses;
    return HCCL_SUCCESS;
}

int32_t HcclAmdRingTable(uint32_t nRanks, uint32_t* cycles, uint32_t capacity)
{
    return nRanks == 0 ? 0 : FlattenTable(RingTable(nRanks), nRanks, cycles, capacity);
}

int32_t HcclAmdRhdTable(uint32_t nRanks, uint32_t* realOfVirtual, uint32_t capacity)
{
    return nRanks == 0 ? 0 : FlattenTable(RhdTable(nRanks), nRanks, realOfVirtual, capacity);
}

HcclResult HcclAmdExecutorPlan(const HcclAmdIrOp* ops, uint64_t numOps, uint32_t elemSize, const uint64_t* bufBase,
                               HcclAmdUnitPlan* units, uint64_t capacity, uint64_t* numUnits)
{
    if ((ops == nullptr && numOps != 0) || bufBase == nullptr || numUnits == nullptr) return HCCL_E_PTR;
    if (elemSize == 0) return HCCL_E_PARA;
    const std::vector<HcclAmdIrOp> v(ops, ops + numOps);
    void* bufs[3];
    for (int i = 0; i < 3; ++i) bufs[i] = reinterpret_cast<void*>(static_cast<uintptr_t>(bufBase[i]));
    const std::vector<UnitPlan> plan = PlanUnits(v, bufs, elemSize);
    *numUnits = plan.size();
    if (units == nullptr) return HCCL_SUCCESS;
    if (capacity < plan.size()) return HCCL_E_PARA;
    for (size_t i = 0; i < plan.size(); ++i) {
        units[i].stream = plan[i].stream;
        units[i].isComm = plan[i].isComm ? 1 : 0;
        units[i].firstOp = plan[i].first;
        units[i].numOps = plan[i].count;
        units[i].waitUnit = plan[i].waitUnit;
    }
    return HCCL_SUCCESS;
}

int32_t HcclAmdSelectAivAlgo(int32_t opType, uint32_t nRanks, uint64_t count, HcclDataType dataType, HcclReduceOp op,
                             uint32_t coreLimit, int32_t flags, uint32_t* groupSize)
{
    return SelectAivPlan(opType, nRanks, count, dataType, DataTypeSize(dataType), op, (flags & 1) != 0,
                         (flags & 2) != 0, CclBytesDefault(),
                         coreLimit != 0 ? coreLimit : ReadCommConfig().aivCoreLimit, nullptr, groupSize);
}

HcclResult HcclAmdIpcPlan(const HcclAmdIpcPlanQuery* q, HcclAmdIpcPlanResult* result, HcclAmdIpcGeometry* launches,
                          uint64_t capacity)
{
    if (q == nullptr || result == nullptr) return HCCL_E_PTR;
    const CommConfig cfg = ReadCommConfig();
    std::vector<IpcGeometry> planned;
    HCCL_CHK(IpcPlanQuery(*q, DataTypeSize(static_cast<HcclDataType>(q->dataType)), CclBytesDefault(),
                          cfg.ipcStagingBytes, cfg.smallIpcBytes, result, launches != nullptr ? &planned : nullptr));
    if (launches == nullptr) return HCCL_SUCCESS;
    if (capacity < planned.size()) return HCCL_E_PARA;
    std::copy(planned.begin(), planned.end(), launches);
    return HCCL_SUCCESS;
}

HcclResult HcclAmdP2pPlan(uint64_t count, uint32_t elemSize, uint64_t slotBytes, uint32_t nRanks,
                          HcclAmdP2pPlanResult* plan)
{
    return P2pPlanFor(count, elemSize, slotBytes, nRanks, plan);
}

uint64_t HcclAmdP2pOffset(int32_t what, uint64_t slotBytes, uint32_t nRanks, uint32_t rank, uint32_t index)
{
    switch (what) {
        case HCCL_AMD_P2P_OFF_SLOT: return P2pSlotOffset(slotBytes, rank, index);
        case HCCL_AMD_P2P_OFF_FILLED: return P2pFilledOffset(slotBytes, nRanks, rank, index);
        case HCCL_AMD_P2P_OFF_DRAINED: return P2pDrainedOffset(slotBytes, nRanks, rank, index);
        default: return UINT64_MAX;
    }
}

HcclResult HcclAmdBatchSendRecvOrder(const HcclSendRecvItem* items, uint32_t itemNum, uint32_t rank, uint32_t rankSize,
                                     uint32_t* order, uint32_t* numSends, uint32_t* numRecvs, uint32_t* numSelfPairs)
{
    return BatchSendRecvOrder(items, itemNum, rank, rankSize, order, numSends, numRecvs, numSelfPairs);
}

HcclResult HcclAmdCheckRecord(int32_t opType, uint32_t root, HcclReduceOp op, HcclDataType dataType, uint64_t count,
                              uint64_t bufferBytes, int32_t expansionAiv, int32_t strict, uint32_t aivCoreLimit,
                              HcclAmdCheckRecordWords* record)
{
    if (record == nullptr) return HCCL_E_PTR;
    return FillCheckRecord(opType, root, op, dataType, count, bufferBytes, expansionAiv != 0, strict != 0, aivCoreLimit,
                           record);
}

const char* HcclAmdCheckFieldName(int32_t field)
{
    // the parameter names of InconsistentCheckParams (inconsistent_check.cc:92-128); the last is this library's own
    static const char* const kNames[HCCL_AMD_CHECK_FIELDS] = {
        "HcclBufferSize", "RootRankId", "OpType",       "OpExecuteConfig",  "HcclReduceOp",
        "HcclDataType",   "DataCount",  "AivCoreLimit", "HcclDeterministic"};
    return field >= 0 && field < HCCL_AMD_CHECK_FIELDS ? kNames[field] : nullptr;
}

HcclResult HcclAmdParseDfsConfig(const char* text, int32_t* inconsistentCheck)
{
    return ParseDfsConfig(text, inconsistentCheck);
}

HcclResult HcclAmdBuildScheduleV(uint32_t nRanks, uint32_t rank, const uint64_t* sendCounts,
                                 const uint64_t* sendDispls, HcclDataType dataType, uint64_t pieceBytes,
                                 HcclAmdIrOp* ops, uint64_t capacity, uint64_t* numOps, uint64_t* scratchElems)
{
    if (numOps == nullptr || sendCounts == nullptr || sendDispls == nullptr) return HCCL_E_PTR;
    const uint32_t es = DataTypeSize(dataType);
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    if (nRanks == 0 || rank >= nRanks) return HCCL_E_PARA;
    for (uint32_t q = 0; q < nRanks; ++q) {
        if (sendCounts[q] > UINT64_MAX / 16 || sendDispls[q] > UINT64_MAX / 16 - sendCounts[q]) return HCCL_E_PARA;
    }
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_REDUCE_SCATTER_V;
    p.nRanks = nRanks;
    p.rank = rank;
    p.counts.assign(sendCounts, sendCounts + nRanks);
    p.displs.assign(sendDispls, sendDispls + nRanks);
    p.count = sendCounts[rank];
    p.elemSize = es;
    p.pieceBytes = pieceBytes;
    return BuildAndCopyOut(p, ops, capacity, numOps, nullptr, scratchElems);
}

HcclResult HcclAmdBuildScheduleAlltoAll(uint32_t nRanks, uint32_t rank, const uint64_t* sendCounts,
                                        const uint64_t* sdispls, const uint64_t* recvCounts, const uint64_t* rdispls,
                                        HcclDataType dataType, uint64_t pieceBytes, HcclAmdIrOp* ops, uint64_t capacity,
                                        uint64_t* numOps, uint64_t* scratchElems)
{
    if (numOps == nullptr || sendCounts == nullptr || sdispls == nullptr || recvCounts == nullptr || rdispls == nullptr) {
        return HCCL_E_PTR;
    }
    const uint32_t es = DataTypeSize(dataType);
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    if (nRanks == 0 || rank >= nRanks || nRanks > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    HCCL_CHK(CheckA2aBlocks(sendCounts, sdispls, nRanks));
    HCCL_CHK(CheckA2aBlocks(recvCounts, rdispls, nRanks));
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_ALLTOALL;
    p.nRanks = nRanks;
    p.rank = rank;
    p.counts.assign(sendCounts, sendCounts + nRanks);
    p.displs.assign(sdispls, sdispls + nRanks);
    p.recvCounts.assign(recvCounts, recvCounts + nRanks);
    p.recvDispls.assign(rdispls, rdispls + nRanks);
    p.count = sendCounts[rank];
    p.elemSize = es;
    p.pieceBytes = pieceBytes;
    return BuildAndCopyOut(p, ops, capacity, numOps, nullptr, scratchElems);
}

HcclResult HcclAmdBuildScheduleAllGatherV(uint32_t nRanks, uint32_t rank, const uint64_t* recvCounts,
                                          const uint64_t* recvDispls, int32_t inPlace, HcclDataType dataType,
                                          uint64_t pieceBytes, HcclAmdIrOp* ops, uint64_t capacity, uint64_t* numOps,
                                          uint64_t* scratchElems)
{
    if (numOps == nullptr || recvCounts == nullptr || recvDispls == nullptr) return HCCL_E_PTR;
    const uint32_t es = DataTypeSize(dataType);
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    if (nRanks == 0 || rank >= nRanks || nRanks > HCCL_AMD_IR_MAX_SRC) return HCCL_E_PARA;
    HCCL_CHK(CheckA2aBlocks(recvCounts, recvDispls, nRanks));
    ScheduleParams p;
    p.opType = HCCL_AMD_OP_ALLGATHER_V;
    p.nRanks = nRanks;
    p.rank = rank;
    p.counts.assign(recvCounts, recvCounts + nRanks);
    p.displs.assign(recvDispls, recvDispls + nRanks);
    p.count = recvCounts[rank];
    p.inPlace = inPlace != 0;
    p.elemSize = es;
    p.pieceBytes = pieceBytes;
    return BuildAndCopyOut(p, ops, capacity, numOps, nullptr, scratchElems);
}

int32_t HcclAmdSelectAlgo(int32_t opType, uint32_t nRanks, uint64_t bytes, int32_t special)
{
    return SelectAlgo(opType, nRanks, bytes, special != 0);
}

HcclResult HcclAmdBuildSchedule(int32_t opType, int32_t algo, uint32_t nRanks, uint32_t rank, uint64_t count,
                                HcclDataType dataType, uint32_t root, uint64_t pieceBytes, HcclAmdIrOp* ops,
                                uint64_t capacity, uint64_t* numOps, int32_t* algoUsed, uint64_t* scratchElems)
{
    if (numOps == nullptr) return HCCL_E_PTR;
    uint32_t es = DataTypeSize(dataType);
    if (opType == HCCL_AMD_OP_BARRIER) {
        // no user data: count, root and dataType are ignored; the tokens are one INT8 element
        es = 1;
        count = 0;
        root = 0;
    }
    if (es == 0) return HCCL_E_NOT_SUPPORT;
    ScheduleParams p;
    p.opType = opType;
    p.algo = algo;
    p.nRanks = nRanks;
    p.rank = rank;
    p.count = count;
    p.elemSize = es;
    p.root = root;
    p.pieceBytes = pieceBytes;
    p.special = IsSpecialForSelector(dataType, HCCL_REDUCE_SUM);  // the op is not an argument here
    return BuildAndCopyOut(p, ops, capacity, numOps, algoUsed, scratchElems);
}

}  // extern "C"
