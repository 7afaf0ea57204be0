/*
 * hccl.h — MI355X-native drop-in for HCCL's operator surface.
 *
 * Each entry point below keeps the exact name, argument order, argument meaning and
 * return-code behaviour of the reference's declaration, so a caller linked against
 * HCCL links against libhccl_amd.so unchanged:
 *
 *   HcclAllReduce      replaces /root/reference/include/hccl.h:35-37  (impl all_reduce_op.cc:23-52)
 *   HcclReduceScatter  replaces /root/reference/include/hccl.h:67-69  (impl reduce_scatter_op.cc:23-72)
 *   HcclReduceScatterV replaces /root/reference/include/hccl.h:87-89  (impl reduce_scatter_v_op.cc:24-83)
 *   HcclReduce         replaces /root/reference/include/hccl.h:245-247 (impl reduce_op.cc:23-54)
 *   HcclBroadcast      replaces /root/reference/include/hccl.h:52      (impl broadcast_op.cc:23-50)
 *   HcclAlltoAll, HcclAlltoAllV, HcclAlltoAllVC
 *                      replace the reference's include/hccl.h:185-229  (impl all_to_all_v_op.cc:23-206)
 *   HcclSend, HcclRecv, HcclBatchSendRecv
 *                      replace the reference's include/hccl.h:154-169, 256-257 (impl send_op.cc:33, 126-150, recv_op.cc,
 *                      batch_send_recv_op.cc:39-56, ins_v2_batch_send_recv_executor.cc:106-208)
 *   HcclBarrier        replaces the reference's src/ops/barrier/barrier_op.h (impl barrier_op.cc:91-102, 137-140)
 *
 * The communicator calls are the hcomm functions the reference's callers use
 * (examples/02_collectives/01_allreduce/main.cc:75,100,122; test/st/.../all_reduce_testcase.cc:80);
 * they are external to the reference repo and are implemented here over RCCL:
 *
 *   HcclGetRootInfo, HcclCommInitRootInfo, HcclCommInitClusterInfo, HcclCommInitAll, HcclCommDestroy,
 *   HcclGetRankSize, HcclGetRankId
 *
 * Semantics: stream-ordered and asynchronous with respect to the host, like the reference
 * (op_common.cc:962-970): work is enqueued behind everything already on `stream`, internal
 * streams are joined back into `stream` before return, and the host never blocks.
 *
 * Inconsistent arguments. Where a paragraph below says that the peers of a rank "are not told" and wait for a bound,
 * that holds for a rank refused by its own argument checks: it never enters the collective. Ranks that enter a
 * collective with different arguments (count, data type, reduce op, root, operator, HCCL_BUFFSIZE, the (=)
 * configuration) are told when HCCL_DFS_CONFIG=inconsistent_check:on (or first) is set: a check ahead of the collective
 * fails every communicator that sees a difference with HCCL_E_PARA at once (HcclGetCommAsyncError; the next call
 * returns it, later ones HCCL_E_SUSPENDING), and HcclAmdCommInconsistency (hccl_amd.h) names the rank, the parameter and
 * both values. Checked: AllReduce, ReduceScatter, ReduceScatterV, Reduce, AllGather, AllGatherV, Broadcast, Scatter,
 * AlltoAll, AlltoAllV, AlltoAllVC and Barrier, except calls that return before any collective work (zero counts, one
 * rank). HcclSend, HcclRecv and HcclBatchSendRecv are not checked: they are not collective, so they cannot run the
 * check's collective set-up. Unset means off, where the reference defaults to first: the check adds a launch per call
 * and an allocation per communicator.
 */
#ifndef HCCL_AMD_HCCL_H_
#define HCCL_AMD_HCCL_H_

#include "hccl_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* AllReduce: recvBuf[i] = op over ranks of sendBuf[i], count elements. In-place allowed. */
extern HcclResult HcclAllReduce(void* sendBuf, void* recvBuf, uint64_t count, HcclDataType dataType,
                                HcclReduceOp op, HcclComm comm, aclrtStream stream);

/* ReduceScatter: sendBuf holds rankSize blocks of recvCount; rank r receives the reduce of block r. */
extern HcclResult HcclReduceScatter(void* sendBuf, void* recvBuf, uint64_t recvCount, HcclDataType dataType,
                                    HcclReduceOp op, HcclComm comm, aclrtStream stream);

/* ReduceScatterV: rank q's block of sendBuf is sendCounts[q] elements at sendDispls[q] (uint64 arrays of rankSize
 * entries); rank r receives the reduce of every rank's block r, sendCounts[r] elements (recvCount must hold them).
 * Replaces /root/reference/include/hccl.h:87-89 (reduce_scatter_v_op.cc:24-83).
 * Per-rank contract: the argument checks are local and run before any collective work, like the reference's. One
 * addition has no reference counterpart: sendCounts[rank] > recvCount returns HCCL_E_PARA on that rank alone (the
 * reference would overrun recvBuf). Its peers are not told: they wait in the collective until HCCL_EXEC_TIMEOUT
 * fails their communicators (HCCL_E_TIMEOUT, then HCCL_E_SUSPENDING), so every rank must pass consistent counts. */
extern HcclResult HcclReduceScatterV(void* sendBuf, const void* sendCounts, const void* sendDispls, void* recvBuf,
                                     uint64_t recvCount, HcclDataType dataType, HcclReduceOp op, HcclComm comm,
                                     aclrtStream stream);

/* Reduce: recvBuf on `root` receives the reduce of every rank's sendBuf (recvBuf must be non-null everywhere). */
extern HcclResult HcclReduce(void* sendBuf, void* recvBuf, uint64_t count, HcclDataType dataType, HcclReduceOp op,
                             uint32_t root, HcclComm comm, aclrtStream stream);

/* AllGather: recvBuf holds rankSize blocks of sendCount, block r = rank r's sendBuf (replaces
 * /root/reference/include/hccl.h:120-121; the gather half of AllReduce and of config C4's RS + AG). */
extern HcclResult HcclAllGather(void* sendBuf, void* recvBuf, uint64_t sendCount, HcclDataType dataType,
                                HcclComm comm, aclrtStream stream);

/* Broadcast: every rank's buf receives root's count elements, bit for bit; root's buf is not written (replaces
 * /root/reference/include/hccl.h:52; checks of broadcast_op.cc:23-50, 99-142). Every valid data type but INT128. */
extern HcclResult HcclBroadcast(void* buf, uint64_t count, HcclDataType dataType, uint32_t root, HcclComm comm,
                                aclrtStream stream);

/* Scatter: sendBuf on `root` holds rankSize blocks of recvCount; rank r's recvBuf receives block r, bit for bit (replaces
 * the reference's include/hccl.h:104-106; checks of scatter_op.cc:70-84, 126-139). recvCount == 0 returns HCCL_SUCCESS
 * before any other check. sendBuf is read on the root only: the other ranks may pass NULL. The root's own block is
 * copied. recvBuf == sendBuf on the root is legal (the reference's in-place PostCopy): block `root` then lands at the
 * head of the buffer, after block 0 has left it; any other overlap of the two buffers is the caller's error. Every
 * valid data type but INT128. */
extern HcclResult HcclScatter(void* sendBuf, void* recvBuf, uint64_t recvCount, HcclDataType dataType, uint32_t root,
                              HcclComm comm, aclrtStream stream);

/* AllGatherV: rank q contributes recvCounts[q] elements, which every rank receives at recvDispls[q] of its recvBuf
 * (uint64 arrays of rankSize entries, in elements, the same on every rank); sendCount is this rank's own contribution
 * (replaces the reference's include/hccl.h:138-140; checks of all_gather_v_op.cc:40-54, 136-188). All recvCounts zero
 * returns HCCL_SUCCESS (recvBuf may then be NULL); a rank with sendCount == 0 still takes part and may pass a NULL
 * sendBuf. sendBuf == recvBuf + recvDispls[rank] (in place) skips the own copy. Every valid data type but INT128.
 * Per-rank contract: the argument checks are local and run before any collective work, like the reference's. Two
 * additions have no reference counterpart: sendCount != recvCounts[rank] returns HCCL_E_PARA on that rank alone (the
 * reference would send what its peers do not expect), and a block whose count exceeds SYS_MAX_COUNT or whose end does
 * not fit 64 bits is refused (HCCL_E_PARA). The peers of a refused rank are not told: they wait in the collective until
 * the one-sided barrier's bound (HCCL_AMD_IPC_TIMEOUT_MS) or HCCL_EXEC_TIMEOUT fails their communicators, so every rank
 * must pass consistent counts, as with HcclReduceScatterV. */
extern HcclResult HcclAllGatherV(void* sendBuf, uint64_t sendCount, void* recvBuf, const void* recvCounts,
                                 const void* recvDispls, HcclDataType dataType, HcclComm comm, aclrtStream stream);

/* The all-to-all family (replaces the reference's include/hccl.h:185-229; checks of all_to_all_v_op.cc:23-206,
 * 419-576). Rank p sends sendCounts[q] elements at sdispls[q] of sendBuf to rank q, which receives them at rdispls[p] of
 * its recvBuf (counts and displacements are uint64 arrays of rankSize entries, in elements). Data is moved bit for bit;
 * every valid data type but INT128.
 * Caller's contract: sendBuf and recvBuf are distinct (HCCL_E_PARA otherwise), the regions of recvBuf overlap neither
 * each other nor sendBuf, and sendCounts[q] on rank p equals recvCounts[p] on rank q. The checks are local and run
 * before any collective work, like the reference's; ranks whose counts disagree wait for each other until the
 * one-sided barrier's bound (HCCL_AMD_IPC_TIMEOUT_MS) or HCCL_EXEC_TIMEOUT fails their communicators, as with
 * inconsistent HcclReduceScatterV counts.
 *   HcclAlltoAll    sendCount elements to every rank, block q of sendBuf to rank q, block p of recvBuf from rank p.
 *                   sendCount == recvCount == 0 returns HCCL_SUCCESS before any other check; sendCount != recvCount or
 *                   sendType != recvType is HCCL_E_PARA.
 *   HcclAlltoAllV   a null sendBuf / recvBuf is legal when all of its counts are 0. A rank whose counts are all 0 still
 *                   takes part: its peers may exchange data and wait for it. One addition has no reference
 *                   counterpart: the reference ignores sendType; here sendType != recvType returns HCCL_E_PARA (no
 *                   conversion is done, and a silent reinterpretation would hide a caller's mistake).
 *   HcclAlltoAllVC  sendCountMatrix is rankSize x rankSize uint64, row-major, the same on every rank: row `rank` holds
 *                   this rank's send counts, column `rank` its receive counts; both displacements are the packed prefix
 *                   sums. sendType != recvType is HCCL_E_PARA as above. */
extern HcclResult HcclAlltoAllVC(const void* sendBuf, const void* sendCountMatrix, HcclDataType sendType,
                                 const void* recvBuf, HcclDataType recvType, HcclComm comm, aclrtStream stream);
extern HcclResult HcclAlltoAllV(const void* sendBuf, const void* sendCounts, const void* sdispls,
                                HcclDataType sendType, const void* recvBuf, const void* recvCounts,
                                const void* rdispls, HcclDataType recvType, HcclComm comm, aclrtStream stream);
extern HcclResult HcclAlltoAll(const void* sendBuf, uint64_t sendCount, HcclDataType sendType, const void* recvBuf,
                               uint64_t recvCount, HcclDataType recvType, HcclComm comm, aclrtStream stream);

/* Point-to-point (replaces the reference's include/hccl.h:154-169, 256-257). HcclSend moves count elements of sendBuf
 * to destRank, whose HcclRecv from this rank receives them, bit for bit; every valid data type but INT128. Both calls
 * are stream-ordered like every other entry, and the messages of an ordered pair of ranks match in call order (FIFO per
 * ordered pair), whichever of the three entry points posted them.
 * Checks (send_op.cc:33, 126-150; recv_op.cc likewise): count == 0 returns HCCL_SUCCESS before any other check and the
 * peer is not called on; a null comm, buffer or stream is HCCL_E_PTR; then the count (HCCL_E_PARA), the data type
 * (HCCL_E_NOT_SUPPORT), a peer equal to this rank (HCCL_E_NOT_SUPPORT: a one-rank communicator has no valid Send or
 * Recv) and a peer outside the communicator (HCCL_E_PARA).
 * Caller's contract: both sides pass the same count and data type. The checks are local; a Send whose Recv never comes,
 * or comes with another count, waits until the one-sided wait's bound (HCCL_AMD_IPC_TIMEOUT_MS) or HCCL_EXEC_TIMEOUT
 * fails the communicator (HCCL_E_TIMEOUT, then HCCL_E_SUSPENDING), as with inconsistent HcclReduceScatterV counts.
 * A Send of at most two slots (HCCL_AMD_P2P_SLOT_BYTES each) on the one-sided path completes without its Recv having
 * started; no caller may rely on that: RCCL's Send waits for its Recv. Two ranks that first Send to and then Recv from
 * each other must use HcclBatchSendRecv.
 * The one-sided path (HcclAmdCommEnableP2p, include/hccl_amd.h) is chosen per call from the call's largest item;
 * under the automatic selection both ends of a message must therefore post it in calls whose largest items lie on the
 * same side of HCCL_AMD_SMALL_IPC_BYTES (always true of a lone Send and its Recv, and of symmetric batches). */
extern HcclResult HcclSend(void* sendBuf, uint64_t count, HcclDataType dataType, uint32_t destRank, HcclComm comm,
                           aclrtStream stream);
extern HcclResult HcclRecv(void* recvBuf, uint64_t count, HcclDataType dataType, uint32_t srcRank, HcclComm comm,
                           aclrtStream stream);

/* BatchSendRecv: the itemNum tasks of sendRecvInfo as one deadlock-free group (batch_send_recv_op.cc:39-56).
 * itemNum == 0 returns HCCL_SUCCESS; a null stream, comm or list is HCCL_E_PTR; then every item's count (HCCL_E_PARA)
 * and data type (HCCL_E_NOT_SUPPORT), then every item's remoteRank (HCCL_E_PARA outside the communicator). Items with
 * count == 0 are dropped; a remaining item with a null buf is HCCL_E_PTR, one whose sendRecvType is neither HCCL_SEND
 * nor HCCL_RECV HCCL_E_PARA. The list is ordered as the reference orders it (ins_v2_batch_send_recv_executor.cc:
 * 106-208): among the items of one direction and peer a stable sort by count descending, then dataType descending, so
 * two ranks that list duplicate pairs in different orders still match. Sends to this rank are paired, after the same
 * sort, with receives from it, and each pair is a local copy; an unmatched self item, or a pair whose counts or element
 * sizes differ, is HCCL_E_PARA. More than 32 remote items in one call are HCCL_E_NOT_SUPPORT on the one-sided path. */
extern HcclResult HcclBatchSendRecv(HcclSendRecvItem* sendRecvInfo, uint32_t itemNum, HcclComm comm,
                                    aclrtStream stream);

/* Barrier: work enqueued on any rank's `stream` after its HcclBarrier does not start until every rank's stream has
 * reached its own HcclBarrier. No user data moves. Stream-ordered and asynchronous to the host like every other entry:
 * the call returns once the barrier is enqueued, and a host that must wait synchronises the stream. The symbol
 * torch_npu's ProcessGroupHCCL::barrier calls.
 * Checks, in the reference's order (barrier_op.cc:91-102, 137-140): a null stream is HCCL_E_PTR, then a null comm is
 * HCCL_E_PTR, then the communicator's status gate applies as for every collective; a one-rank communicator returns
 * HCCL_SUCCESS and enqueues nothing.
 * It runs as one launch of one workgroup per rank on the one-sided path (the flag exchange of the collectives' own
 * barrier and nothing else: no staging tier, no allocation per call) wherever that path is available, and as the
 * reference's NHR token exchange (AicpuBarrierSoleNHR: ceil(log2 rankSize) steps) on the transport otherwise.
 * Per-rank contract: every rank of the communicator calls it. A rank that never calls leaves its peers waiting until
 * the one-sided wait's bound (HCCL_AMD_IPC_TIMEOUT_MS) or HCCL_EXEC_TIMEOUT fails their communicators (HCCL_E_TIMEOUT,
 * then HCCL_E_SUSPENDING), as with inconsistent HcclReduceScatterV counts. */
extern HcclResult HcclBarrier(HcclComm comm, aclrtStream stream);

/* Communicator management (hcomm surface used by the reference's callers). */
extern HcclResult HcclGetRootInfo(HcclRootInfo* rootInfo);
extern HcclResult HcclCommInitRootInfo(uint32_t nRanks, const HcclRootInfo* rootInfo, uint32_t rank,
                                       HcclComm* comm);
/* Rank `rank` of the communicator described by the rank table file `clusterInfo` (JSON, docs/.../cluster_info_config/rank_table_config_a2.md;
 * test/st/algorithm/testcase/all_reduce_testcase.cc:80). The rank runs on its entry's device_id. Rank 0 publishes the
 * transport's unique id over TCP at the rank-0 server's host_ip (else HCCL_IF_IP, else 127.0.0.1 for one server) and
 * the rank-0 device's host_port (else HCCL_IF_BASE_PORT, default 60000), waiting at most HCCL_CONNECT_TIMEOUT + 20 s. */
extern HcclResult HcclCommInitClusterInfo(const char* clusterInfo, uint32_t rank, HcclComm* comm);
/* One communicator per listed device in this process (single-node batch creation); comms[i] is rank i on
 * devices[i]. Drive each rank from its own host thread. */
extern HcclResult HcclCommInitAll(uint32_t ndev, int32_t* devices, HcclComm* comms);
/* Destroys the communicator. Its outstanding work is flushed first (ncclCommFinalize, bounded by HCCL_EXEC_TIMEOUT;
 * past it the communicator is aborted). If a HIP graph captured on a collective of this communicator is still alive,
 * the call returns HCCL_SUCCESS at once and the teardown runs when the last such graph is destroyed: the graph holds
 * the communicator's staging and RCCL plans (RCCL's own destroy would wait for the graph). The handle is invalid on
 * return either way. */
extern HcclResult HcclCommDestroy(HcclComm comm);
extern HcclResult HcclGetRankSize(HcclComm comm, uint32_t* rankSize);
extern HcclResult HcclGetRankId(HcclComm comm, uint32_t* rank);
/* Asynchronous error of the communicator (CANN hccl_comm.h; polled by framework watchdogs such as torch_npu's
 * ProcessGroupHCCL). Non-blocking. *asyncError = HCCL_E_TIMEOUT after a one-sided barrier wait exceeded its bound,
 * or after a collective on the RCCL path ran past HCCL_EXEC_TIMEOUT once started (default 1836 s, 0 = never; the
 * communicator's watchdog then aborts RCCL), the transport's error after an RCCL asynchronous failure, else
 * HCCL_SUCCESS. Once the first
 * collective entry has observed such an error (and returned it), every later collective on the communicator returns
 * HCCL_E_SUSPENDING: the reference's status gate, src/ops/op_common/op_common.cc:89-97. */
extern HcclResult HcclGetCommAsyncError(HcclComm comm, HcclResult* asyncError);

#ifdef __cplusplus
}
#endif
#endif /* HCCL_AMD_HCCL_H_ */
