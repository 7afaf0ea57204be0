/*
 * hccl_amd.h — extension C ABI of libhccl_amd.so (everything that is not in the reference's hccl.h).
 *
 * 1. The inner reduce primitive. In the reference every reducing schedule ends in
 *    LocalReduce (/root/reference/src/ops/op_common/template/wrapper/alg_data_trans_wrapper.cc:901-928),
 *    which enqueues hcomm's HcommLocalReduceOnThread(thread, dst, src, count, dtype, op) = "dst = src (+) dst"
 *    (call site :924-926; stub semantics test/st/algorithm/utils/src/hccl_proxy/hccl_stub.cc:648-677), or, for
 *    64-bit dtypes and PROD, runs AicpuReduce on the AICPU core (:1254-1353). HcclAmdLocalReduce replaces both
 *    with one HIP kernel family on a HIP stream. Element rule, identical to AicpuReduceTemplate (:1313-1353):
 *        SUM  dst = src + dst          PROD dst = src * dst   (integers wrap, two's complement)
 *        MAX  dst = (src < dst) ? dst : src    (std::max(src, dst): ties and NaN give src)
 *        MIN  dst = (dst < src) ? dst : src    (std::min(src, dst): ties and NaN give src)
 *    fp16 is computed through fp32 with round-to-nearest-even (AicpuReduceFp16, :1232-1252); bf16 the same way.
 *
 * 2. The schedule IR. Every collective is compiled to a per-rank list of HcclAmdIrOp records. The same records
 *    are executed by the HIP/RCCL executor and replayed by the CPU oracle (oracle/), so the association order of
 *    every reduced element is fixed by the IR and checked bit-for-bit.
 *
 * 3. A loopback world: nRanks communicators inside one process on the current device whose "links" are
 *    device-to-device copies. It runs the exact executor the RCCL path runs and is how the multi-rank schedules
 *    are tested on a single MI355X (the reference's analogue is its host simulator, test/st/algorithm).
 */
#ifndef HCCL_AMD_EXT_H_
#define HCCL_AMD_EXT_H_

#include "hccl_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- local reduce primitive */

/* dst[i] = src[i] (op) dst[i], i < count. Mirrors HcommLocalReduceOnThread(thread, dst, src, count, dt, op). */
extern HcclResult HcclAmdLocalReduce(void* dst, const void* src, uint64_t count, HcclDataType dataType,
                                     HcclReduceOp op, aclrtStream stream);

/* out[i] = src[i] (op) dst[i]: the out-of-place form (3 streams: 2 reads, 1 write). out may alias dst or src. */
extern HcclResult HcclAmdLocalReduce2(void* out, const void* src, const void* dst, uint64_t count,
                                      HcclDataType dataType, HcclReduceOp op, aclrtStream stream);

/* Ordered n-ary fold in one pass: acc = srcs[0]; for j = 1..nsrc-1: acc = srcs[j] (op) acc; out = acc.
 * 1 <= nsrc <= HCCL_AMD_IR_MAX_SRC. out may alias any srcs[j]. */
extern HcclResult HcclAmdLocalReduceN(void* out, const void* const* srcs, uint32_t nsrc, uint64_t count,
                                      HcclDataType dataType, HcclReduceOp op, aclrtStream stream);

/* Byte size of one element of dataType, 0 if unknown (DATATYPE_SIZE_TABLE, alg_param.h:43-61). */
extern uint32_t HcclAmdDataTypeSize(HcclDataType dataType);

extern const char* HcclAmdGetErrorString(HcclResult code);

/* ---------------------------------------------------------------- schedule IR */

#define HCCL_AMD_IR_MAX_SRC 16

typedef enum {
    HCCL_AMD_IR_COPY = 0,   /* dst <- src[0] */
    HCCL_AMD_IR_REDUCE = 1, /* dst <- fold(src[0..nsrc)) with the LocalReduceN order */
    HCCL_AMD_IR_SEND = 2,   /* send src[0] (count elements) to peer */
    HCCL_AMD_IR_RECV = 3    /* receive count elements from peer into dst */
} HcclAmdIrKind;

typedef enum {
    HCCL_AMD_BUF_INPUT = 0,   /* user sendBuf */
    HCCL_AMD_BUF_OUTPUT = 1,  /* user recvBuf */
    HCCL_AMD_BUF_SCRATCH = 2  /* per-communicator staging ("CCL buffer") */
} HcclAmdBuf;

typedef struct {
    int32_t kind;   /* HcclAmdIrKind */
    int32_t peer;   /* SEND / RECV peer rank, else -1 */
    int32_t nsrc;   /* number of valid src entries */
    int32_t group;  /* SEND/RECV records with equal group are posted together (one RCCL group) */
    uint64_t count; /* elements */
    int32_t dstBuf; /* HcclAmdBuf, -1 for SEND */
    int32_t reserved;
    uint64_t dstOff; /* element offset */
    int32_t srcBuf[HCCL_AMD_IR_MAX_SRC];
    uint64_t srcOff[HCCL_AMD_IR_MAX_SRC];
} HcclAmdIrOp;

typedef enum {
    HCCL_AMD_OP_ALLREDUCE = 0,
    HCCL_AMD_OP_REDUCE_SCATTER = 1,
    HCCL_AMD_OP_REDUCE = 2,
    HCCL_AMD_OP_ALLGATHER = 3, /* the second half of AllReduce as an operator (count = sendCount) */
    HCCL_AMD_OP_REDUCE_SCATTER_V = 4, /* per-rank counts and displacements (HcclAmdBuildScheduleV) */
    HCCL_AMD_OP_BROADCAST = 5, /* root's count elements into every rank's buffer, in place (INPUT = OUTPUT = buf);
                                  moves data only: the mesh two-shot schedule whatever family is asked for */
    HCCL_AMD_OP_ALLTOALL = 6,  /* AlltoAll / AlltoAllV / AlltoAllVC: per-peer send and receive counts and displacements
                                  (HcclAmdBuildScheduleAlltoAll); moves data only: the mesh schedule whatever family */
    HCCL_AMD_OP_SCATTER = 7,   /* block r of root's input (nRanks blocks of `count`) into rank r's output; moves data
                                  only: the mesh schedule whatever family (HcclAmdBuildSchedule with count and root) */
    HCCL_AMD_OP_ALLGATHER_V = 8, /* rank q's counts[q] elements to displs[q] of every rank's output
                                  (HcclAmdBuildScheduleAllGatherV); moves data only: the mesh schedule whatever family */
    HCCL_AMD_OP_BARRIER = 9    /* HcclBarrier: no user data. HcclAmdBuildSchedule ignores count, root and dataType; the
                                  records move tokens of one INT8 element: send k of a program reads byte k of INPUT,
                                  receive k writes byte k of OUTPUT (the communicator's token allocation, never the
                                  executor staging). AUTO, NHR and every family but the two meshes: the reference's
                                  AicpuBarrierSoleNHR, ceil(log2 nRanks) groups of one send and one receive;
                                  MESH_ONESHOT / MESH_TWOSHOT: its Mesh1D template, one group with every peer */
} HcclAmdOpType;

typedef enum {
    HCCL_AMD_ALGO_AUTO = 0,         /* reference selector policy (all_reduce_auto_selector.cc:517-550) */
    HCCL_AMD_ALGO_MESH_ONESHOT = 1, /* order O1: own input first, then ascending ranks */
    HCCL_AMD_ALGO_MESH_TWOSHOT = 2, /* AllReduce: order O2 (ascending from rank 0); RS/Reduce: O1 */
    HCCL_AMD_ALGO_RING = 3,         /* ring reduce-scatter (+ ring all-gather) */
    HCCL_AMD_ALGO_RHD = 4,          /* recursive halving / doubling (power-of-two rank counts) */
    HCCL_AMD_ALGO_NHR = 5,          /* AllReduce: the reference's NHR template, order O5 (any rank count) */
    HCCL_AMD_ALGO_ORDER_PRESERVED = 6, /* AllReduce / ReduceScatter: HCCL_DETERMINISTIC=STRICT tree, order O4 */
    HCCL_AMD_ALGO_IPC_TWOSHOT = 7,     /* AllReduce: one kernel over peer-mapped staging (AIV GM_IN model), O2 */
    HCCL_AMD_ALGO_MESH_CHUNK = 8,      /* AllReduce / ReduceScatter: the reference's MeshChunk templates, order O6
                                          (owner first, then the peers in a per-sub-slice rotated order) */
    HCCL_AMD_ALGO_IPC = 9,             /* the one-sided kernel in the order family the auto selector picks (one-shot
                                          O1 / two-shot O2 / MeshChunk O6 ...): the auto path's bits over IPC */
    HCCL_AMD_ALGO_AIV = 10,            /* the reference's AIV engine (HCCL_OP_EXPANSION_MODE=AIV): SelectAivAlgo's
                                          choice and orders on the one-sided kernel; what it does not match runs
                                          the auto (AICPU) selection, as the reference falls back */
    HCCL_AMD_ALGO_AIV_ONLY = 11,       /* the AIV engine with no fallback (OpExecuteConfig::AIV_ONLY): no 8 MiB x n
                                          bound, and what SelectAivAlgo does not match returns HCCL_E_NOT_SUPPORT */
    HCCL_AMD_ALGO_IPC_RHD = 12         /* AllReduce, power-of-two n: HCCL_AMD_ALGO_RHD's bits from one one-shot launch
                                          of the one-sided kernel (one barrier instead of 2 log2 n transport steps);
                                          anything else, or no peer mappings, runs HCCL_AMD_ALGO_RHD */
} HcclAmdAlgo;

/* Variant of the reference's AIV engine a call takes (HcclAmdSelectAivAlgo). */
typedef enum {
    HCCL_AMD_AIV_NOT_MATCHED = 0,       /* SelectAivAlgo does not match: the AICPU engine runs */
    HCCL_AMD_AIV_AR_ONESHOT = 1,        /* aiv_all_reduce_mesh_1d_oneshot.h:33-48, order O2 */
    HCCL_AMD_AIV_AR_TWOSHOT_LARGE = 2,  /* aiv_all_reduce_mesh_1d_twoshot.h:145-181: O1 over groupSize * n
                                           balanced slices, rank r owning [r * groupSize, (r + 1) * groupSize) */
    HCCL_AMD_AIV_AR_TWOSHOT_SMALL = 3,  /* aiv_all_reduce_mesh_1d_twoshot.h:224-271: O2 over ceil(count / n) */
    HCCL_AMD_AIV_RS_BIGDATA = 4,        /* aiv_reduce_scatter_mesh_1d_bigdata.h:85-101: O2 */
    HCCL_AMD_AIV_RS_LOCAL_TREE = 5      /* aiv_reduce_scatter_local_tree.h:138-172: O4 (pow-2 tree) */
} HcclAmdAivVariant;

/* The AIV-engine variant an operation would take (opType ALLREDUCE or REDUCE_SCATTER; count = recvCount for
 * ReduceScatter) on nRanks ranks with `coreLimit` vector cores (0 = HCCL_AMD_AIV_CORE_LIMIT, default 48) and the CCL
 * buffer HCCL_BUFFSIZE. flags: bit 0 = HCCL_DETERMINISTIC=strict, bit 1 = AIV_ONLY (HCCL_AMD_ALGO_AIV_ONLY).
 * *groupSize (may be NULL) receives the slices per rank of HCCL_AMD_AIV_AR_TWOSHOT_LARGE (1 otherwise). Returns an
 * HcclAmdAivVariant. */
extern int32_t HcclAmdSelectAivAlgo(int32_t opType, uint32_t nRanks, uint64_t count, HcclDataType dataType,
                                    HcclReduceOp op, uint32_t coreLimit, int32_t flags, uint32_t* groupSize);

/* Build rank `rank`'s schedule. If ops == NULL only *numOps is written. scratchElems receives the number of
 * scratch elements the schedule addresses. pieceBytes = 0 picks the default pipelining granule. */
extern HcclResult HcclAmdBuildSchedule(int32_t opType, int32_t algo, uint32_t nRanks, uint32_t rank, uint64_t count,
                                       HcclDataType dataType, uint32_t root, uint64_t pieceBytes, HcclAmdIrOp* ops,
                                       uint64_t capacity, uint64_t* numOps, int32_t* algoUsed,
                                       uint64_t* scratchElems);

/* ReduceScatterV schedule of rank `rank`: rank q's block of every input is [sendDispls[q], sendDispls[q] +
 * sendCounts[q]) elements (nRanks entries each); the mesh template's order O1
 * (ins_temp_reduce_scatter_v_mesh_1D.cc:107-146). Same output conventions as HcclAmdBuildSchedule. */
extern HcclResult HcclAmdBuildScheduleV(uint32_t nRanks, uint32_t rank, const uint64_t* sendCounts,
                                        const uint64_t* sendDispls, HcclDataType dataType, uint64_t pieceBytes,
                                        HcclAmdIrOp* ops, uint64_t capacity, uint64_t* numOps,
                                        uint64_t* scratchElems);

/* All-to-all schedule of rank `rank` (the reference's single-node mesh, ins_temp_all_to_all_v_mesh_1D.cc): a copy of the
 * own block, then for every peer q a send of sendCounts[q] elements at sdispls[q] of the input and a receive of
 * recvCounts[q] elements at rdispls[q] of the output (nRanks entries each; zero counts post nothing; no staging).
 * pieceBytes = 0 posts one transport group; otherwise group u holds piece u of every pair that has one. Same output
 * conventions as HcclAmdBuildSchedule. */
extern HcclResult HcclAmdBuildScheduleAlltoAll(uint32_t nRanks, uint32_t rank, const uint64_t* sendCounts,
                                               const uint64_t* sdispls, const uint64_t* recvCounts,
                                               const uint64_t* rdispls, HcclDataType dataType, uint64_t pieceBytes,
                                               HcclAmdIrOp* ops, uint64_t capacity, uint64_t* numOps,
                                               uint64_t* scratchElems);

/* AllGatherV schedule of rank `rank` (the reference's single-node mesh, ins_temp_all_gather_v_mesh_1D.cc): a copy of the
 * own recvCounts[rank] elements of the input to recvDispls[rank] of the output (skipped with inPlace != 0: the input
 * is that very place), then for every peer q a send of the whole input and a receive of recvCounts[q] elements at
 * recvDispls[q] of the output (nRanks entries each, equal on every rank; zero counts post nothing; no staging).
 * pieceBytes as in HcclAmdBuildScheduleAlltoAll. Same output conventions as HcclAmdBuildSchedule. */
extern HcclResult HcclAmdBuildScheduleAllGatherV(uint32_t nRanks, uint32_t rank, const uint64_t* recvCounts,
                                                 const uint64_t* recvDispls, int32_t inPlace, HcclDataType dataType,
                                                 uint64_t pieceBytes, HcclAmdIrOp* ops, uint64_t capacity,
                                                 uint64_t* numOps, uint64_t* scratchElems);

/* The algorithm HCCL_AMD_ALGO_AUTO selects for an operation of `bytes` bytes per rank (ReduceScatter: recvCount
 * bytes) on nRanks ranks; special = 64-bit data type or PROD (the reference selectors' isDataTypeOrReduceTypeSpecial).
 * Mirrors AllReduceAutoSelector / ReduceScatterAutoSelector / ReduceAutoSelector for a single-node MESH_1D. */
extern int32_t HcclAmdSelectAlgo(int32_t opType, uint32_t nRanks, uint64_t bytes, int32_t special);

/* The rings HCCL_AMD_ALGO_RING runs on nRanks ranks: arc-disjoint directed Hamiltonian cycles (n-1 of them for
 * n <= 8 except 4 and 6, where n-2 is the maximum). Writes up to `capacity` cycles of nRanks ranks each, row-major,
 * into cycles (may be NULL) and returns the number of rings (0 for nRanks == 0). */
extern int32_t HcclAmdRingTable(uint32_t nRanks, uint32_t* cycles, uint32_t capacity);

/* The concurrent instances HCCL_AMD_ALGO_RHD runs on a power-of-two nRanks (n-1 of them, one per XOR matching of
 * the ranks): for each instance the real rank of every virtual rank, row-major (nRanks entries per instance), up to
 * `capacity` instances. Returns the number of instances (0 when nRanks is not a power of two or exceeds 16). */
extern int32_t HcclAmdRhdTable(uint32_t nRanks, uint32_t* realOfVirtual, uint32_t capacity);

/* The executor's plan for one rank's IR, without running it (host only; what Execute issues on the GPU): units in
 * issue order, each a transport group (stream 0, the link stream) or a batch of folds / a copy (stream 1, the reduce
 * stream), with the unit of the other stream it waits for (hipStreamWaitEvent), derived from RAW / WAR / WAW conflicts
 * of the units' byte ranges at the buffer base addresses bufBase[HcclAmdBuf] (equal bases model in-place calls). */
typedef struct {
    int32_t stream;   /* 0 = link, 1 = reduce */
    int32_t isComm;   /* 1: SEND/RECV group */
    uint64_t firstOp; /* IR records [firstOp, firstOp + numOps) */
    uint64_t numOps;
    int64_t waitUnit; /* unit index on the other stream, or -1 */
} HcclAmdUnitPlan;
extern HcclResult HcclAmdExecutorPlan(const HcclAmdIrOp* ops, uint64_t numOps, uint32_t elemSize,
                                      const uint64_t* bufBase, HcclAmdUnitPlan* units, uint64_t capacity,
                                      uint64_t* numUnits);

/* The host-side plan of a one-sided call, without running it (host only, no communicator): the numbers the one-sided
 * kernel takes from its host side for every launch of the call. All lengths are in elements. */
#define HCCL_AMD_IPC_MAX_RANKS 16
typedef struct {
    uint64_t total;       /* elements of the launch's input range */
    uint64_t chunkStride; /* chunk c starts at c * chunkStride and holds min(chunkLen, total - c * chunkStride) */
    uint64_t chunkLen;    /* (balanced: the slice length; vgeom: the longest block) */
    uint64_t rem;         /* balanced: the first rem slices hold one element more */
    uint64_t group;       /* balanced: slices per chunk */
    uint64_t piece;       /* elements of every chunk that one round handles: the slot size */
    uint64_t blockElems;  /* piece coordinates per workgroup */
    uint64_t tileElems;   /* 0 = one window per workgroup, else the tile size */
    uint32_t rounds;
    uint32_t epochSpan;   /* barriers per workgroup in the launch (0 in the LL form) */
    uint32_t ll;          /* 1: the LL form (data and flag in one store, no barrier) */
    uint32_t balanced;    /* 1: group * nRanks balanced slices, chunk c = slices [c * group, (c + 1) * group) */
    uint32_t vgeom;       /* 1: chunk c = vLen[c] elements at vStart[c] */
    uint32_t reserved;
    uint64_t vStart[HCCL_AMD_IPC_MAX_RANKS];
    uint64_t vLen[HCCL_AMD_IPC_MAX_RANKS];
} HcclAmdIpcGeometry;

typedef struct {
    int32_t opType;   /* HcclAmdOpType (ReduceScatterV: HCCL_AMD_OP_REDUCE_SCATTER with the explicit V plan) */
    int32_t family;   /* the schedule family whose order the call follows (HcclAmdAlgo: MESH_ONESHOT, MESH_TWOSHOT,
                         MESH_CHUNK; IPC_RHD for RHD's plan; Broadcast: AUTO = by size, MESH_ONESHOT, MESH_TWOSHOT;
                         HCCL_AMD_OP_ALLTOALL: any family = AlltoAll / AlltoAllVC, count = the largest pair count;
                         HCCL_AMD_OP_SCATTER: any family, count = recvCount; HCCL_AMD_OP_ALLGATHER_V: any family, with
                         counts and displs = recvCounts and recvDispls; HCCL_AMD_OP_BARRIER: any family, count and
                         dataType unused: one launch of one workgroup, rounds 1, epochSpan 1, every length and both
                         area sizes 0, since the call needs no staging tier), or
                         -1 for the explicit plan in the next six fields (the AIV variants, ReduceScatterV; AlltoAllV:
                         kind 8, geom 4, subMode 1 = rounds agreed on the device: the launch reports rounds 0, and
                         blocks and tier do not depend on count) */
    uint32_t kind, order, geom, group, subMode; /* the one-sided kernel's kind, fold order and chunk layout */
    uint32_t nRanks;  /* 2 .. HCCL_AMD_IPC_MAX_RANKS */
    uint64_t loopElems;     /* explicit plan: elements per executor loop, 0 = one loop */
    uint64_t count;         /* as the operator takes it (ReduceScatter: recvCount, AllGather: sendCount) */
    const uint64_t* counts; /* V layout only: nRanks entries each */
    const uint64_t* displs;
    int32_t dataType;       /* HcclDataType; element sizes 1, 2, 4 and 8 */
    uint32_t blocks;        /* HcclAmdCommSetIpcBlocks' value, 0 = the default rule */
    uint32_t sharedDevice;  /* 1: a loopback world (all ranks on one device) */
    uint32_t residentPerRank; /* workgroups the device holds at once per rank on it, 0 = unknown (no cap) */
    uint64_t areaBytes;     /* one staging area, and one of the two alternate areas; both 0 = the tiers a */
    uint64_t altBytes;      /* communicator created now would take (small if one round fits there, else large) */
    uint64_t tileBytes;     /* HCCL_AMD_IPC_TILE_KIB in bytes */
    uint64_t llBytes;       /* HCCL_AMD_IPC_LL_BYTES */
} HcclAmdIpcPlanQuery;

typedef struct {
    uint32_t blocks;      /* workgroups per rank and launch */
    uint32_t ll;          /* 1: the call runs in the LL form (it then uses no staging area) */
    uint64_t areaBytes;   /* the area sizes the plan was made for */
    uint64_t altBytes;
    uint64_t numLaunches; /* one per executor loop */
} HcclAmdIpcPlanResult;

/* Plans the call q describes. launches (may be NULL: only *result is written) receives one geometry per launch, up
 * to `capacity`. HCCL_E_PARA for a rank count, element size, group or V layout outside what the operators pass on, or
 * a capacity below result->numLaunches; HCCL_E_NOT_SUPPORT for an operation and family without a one-sided plan. */
extern HcclResult HcclAmdIpcPlan(const HcclAmdIpcPlanQuery* q, HcclAmdIpcPlanResult* result,
                                 HcclAmdIpcGeometry* launches, uint64_t capacity);

/* The plan of one point-to-point message on the one-sided path, and the layout of a rank's p2p area (host only, no
 * communicator): what both ends derive from (count, element size, slot bytes) alone. */
typedef struct {
    uint64_t slotElems;    /* elements of one piece: slotBytes / elemSize */
    uint64_t blockElems;   /* piece coordinates per workgroup: window b = [b * blockElems, (b + 1) * blockElems) */
    uint64_t pieces;       /* ceil(count / slotElems): every workgroup's counters advance by this much */
    uint32_t blocks;       /* workgroups per lane, fixed per library */
    uint32_t slots;        /* data slots per source rank */
    uint64_t dataBytes;    /* nRanks x slots x slotBytes, at the head of the area */
    uint64_t areaBytes;    /* the uncached, peer-mapped allocation HcclAmdCommEnableP2p makes: data, then flags */
    uint64_t counterBytes; /* the private device counters beside it */
} HcclAmdP2pPlanResult;
extern HcclResult HcclAmdP2pPlan(uint64_t count, uint32_t elemSize, uint64_t slotBytes, uint32_t nRanks,
                                 HcclAmdP2pPlanResult* plan);
/* Byte offsets inside the area: the data slot (src, slot), and the flag words filled[src][block], drained[dst][block]. */
extern uint64_t HcclAmdP2pOffset(int32_t what, uint64_t slotBytes, uint32_t nRanks, uint32_t rank, uint32_t index);
#define HCCL_AMD_P2P_OFF_SLOT 0
#define HCCL_AMD_P2P_OFF_FILLED 1
#define HCCL_AMD_P2P_OFF_DRAINED 2

/* HcclBatchSendRecv's list handling without a communicator (include/hccl.h describes the rule). order (itemNum entries)
 * receives indices into items: *numSends remote sends, *numRecvs remote receives, then *numSelfPairs pairs (send,
 * receive). Returns what HcclBatchSendRecv would return for the list. */
extern HcclResult HcclAmdBatchSendRecvOrder(const HcclSendRecvItem* items, uint32_t itemNum, uint32_t rank,
                                            uint32_t rankSize, uint32_t* order, uint32_t* numSends, uint32_t* numRecvs,
                                            uint32_t* numSelfPairs);

/* ---------------------------------------------------------------- communicator extensions */

/* Sets up the one-sided path of HcclSend / HcclRecv / HcclBatchSendRecv. COLLECTIVE: every rank of comm calls it (a
 * point-to-point call involves two ranks, so it can never run a collective set-up itself). It sets up what every
 * one-sided call needs, then maps one more uncached allocation per rank (HcclAmdP2pPlan's areaBytes; slots of
 * HCCL_AMD_P2P_SLOT_BYTES) and allocates the private counters; HcclAmdCommDeviceBytes grows by exactly the two.
 * Idempotent. Not under stream capture. If it fails it fails on every rank alike (HCCL_E_NOT_SUPPORT) and only marks
 * the point-to-point path unavailable: the other one-sided operators stay usable, and the three operators keep taking
 * the transport path, as they do until this call has succeeded (HCCL_E_NOT_SUPPORT on a communicator without one). */
extern HcclResult HcclAmdCommEnableP2p(HcclComm comm);

/* nRanks communicators on the current HIP device, joined by device-to-device copies. comms[r] is rank r.
 * Each rank must be driven from its own host thread (collectives rendezvous like real ranks). */
extern HcclResult HcclAmdCommInitLoopback(uint32_t nRanks, HcclComm* comms);

/* Force the schedule family for subsequent collectives on comm (HCCL_AMD_ALGO_AUTO restores the selector). */
extern HcclResult HcclAmdCommSetAlgo(HcclComm comm, int32_t algo);

/* Workgroups per launch of the one-sided IPC kernel (1..512; 0 restores the default, which grows with the call's
 * bytes from 16 to 256). Must be equal on every rank of the communicator (block b synchronises with block b of each
 * peer). A loopback world uses at most 128 per rank unless set here. Either way the launch is capped at the blocks
 * the device holds at once, divided by the ranks that share it. */
extern HcclResult HcclAmdCommSetIpcBlocks(HcclComm comm, uint32_t blocks);

/* TEST AND PROBE HOOK ONLY, not part of the supported surface: fixes the kind of the one-sided Broadcast on comm so
 * that tests and tools/probes/bcast_loopback.py can run either kind at any size. 0 = one-shot up to the library's
 * byte bound and two-shot above it (the default, and the only value a caller should ever see), 1 = always two-shot,
 * 2 = always one-shot. Nothing checks that the ranks agree: ranks that disagree run different protocols and end in
 * the barrier timeout. There is deliberately no environment variable or configuration key behind it. */
extern HcclResult HcclAmdCommSetBroadcastKind(HcclComm comm, int32_t kind);

/* Pipelining granule (bytes per piece) for subsequent collectives on comm; 0 restores the default. */
extern HcclResult HcclAmdCommSetPieceBytes(HcclComm comm, uint64_t pieceBytes);

/* Algorithm the last collective on comm executed (HcclAmdAlgo), or -1. A collective that the small-call rule
 * (HCCL_AMD_CFG_SMALL_IPC_BYTES) put on the one-sided kernel reports HCCL_AMD_ALGO_IPC (the auto family's order) or,
 * for an AllReduce asked for RHD, HCCL_AMD_ALGO_IPC_RHD (RHD's order). */
extern int32_t HcclAmdCommLastAlgo(HcclComm comm);

/* Configuration. A communicator reads the environment once, when it is created (the reference parses its environment
 * once, InitEnvConfig, src/common/alg_env_config.cc:176); no collective reads it. HcclAmdCommSetConfig changes one
 * entry of comm afterwards: keys marked (=) must be equal on every rank of the communicator, as the environment
 * variables they stand for must be. HCCL_E_PARA for an unknown key or a value out of range. */
typedef enum {
    HCCL_AMD_CFG_DETERMINISTIC_STRICT = 0, /* (=) HCCL_DETERMINISTIC=strict: 1, else 0 */
    HCCL_AMD_CFG_EXPANSION_MODE_AIV = 1,   /* (=) HCCL_OP_EXPANSION_MODE=AIV: 1, else 0 */
    HCCL_AMD_CFG_AIV_CORE_LIMIT = 2,       /* (=) HCCL_AMD_AIV_CORE_LIMIT, 1..4096 (default 48) */
    HCCL_AMD_CFG_SINGLE_STREAM_BYTES = 3,  /* HCCL_AMD_SINGLE_STREAM_BYTES: programs up to this per-rank payload run
                                              on the caller's stream alone (default 1 MiB) */
    HCCL_AMD_CFG_SMALL_IPC_BYTES = 4,      /* (=) HCCL_AMD_SMALL_IPC_BYTES: an AllReduce of auto or RHD family, or a
                                              ReduceScatter or Reduce of auto family, with at most this many input
                                              bytes per rank runs on the one-sided kernel, same bits (default 1 MiB;
                                              0 = never) */
    HCCL_AMD_CFG_PLAN_CACHE = 5,           /* HCCL_AMD_PLAN_CACHE: compiled-collective cache on (1, default) / off (0) */
    HCCL_AMD_CFG_GRAPH_CACHE = 6,          /* HCCL_AMD_GRAPH_CACHE: executor graphs kept, 0..1024 (default 16) */
    HCCL_AMD_CFG_IPC_LIGHT_FENCE = 7,      /* (=) HCCL_AMD_IPC_LIGHT_FENCE: -1 per mode (default), 0 system, 1 light */
    HCCL_AMD_CFG_IPC_NT = 8,               /* (=) HCCL_AMD_IPC_NT: non-temporal loads and stores (default 1) */
    HCCL_AMD_CFG_IPC_THREADS = 9,          /* (=) HCCL_AMD_IPC_THREADS: 256 (default) or 512 */
    HCCL_AMD_CFG_IPC_TILE_KIB = 10,        /* (=) HCCL_AMD_IPC_TILE_KIB: 0 = one window per block (default) */
    HCCL_AMD_CFG_IPC_TIMEOUT_MS = 11,      /* HCCL_AMD_IPC_TIMEOUT_MS, else HCCL_EXEC_TIMEOUT's AIV rule (HcclAmdIpcTimeoutMs) */
    HCCL_AMD_CFG_IPC_STAGING_MIB = 12,     /* (=) HCCL_AMD_IPC_STAGING_MIB: the one-sided kernel's large staging tier,
                                              MiB per area (four areas per rank), 16..1000, or 0 (default) for
                                              HCCL_BUFFSIZE / 2, so that the tier holds 2 x HCCL_BUFFSIZE; read when
                                              the tier is set up (HcclAmdCommDeviceBytes) */
    /* 13 is retired (HCCL_AMD_IPC_STAGING_CACHED, an r03 diagnostic): HCCL_E_PARA */
    HCCL_AMD_CFG_IPC_TRACE = 14,           /* HCCL_AMD_IPC_TRACE: phase stamps (diagnostics); at the IPC set-up */
    HCCL_AMD_CFG_IPC_L2_SCRUB = 15,        /* HCCL_AMD_IPC_L2_SCRUB: L2 maintenance at the IPC set-up (default 1) */
    HCCL_AMD_CFG_FOLD_TIMING = 16,         /* HCCL_AMD_FOLD_TIMING: time the executor's folds (diagnostics; calls run
                                              eagerly, HcclAmdCommFoldTiming reads the last one) */
    HCCL_AMD_CFG_IPC_LL_BYTES = 17,        /* (=) HCCL_AMD_IPC_LL_BYTES, 0..65536 (default 65536): one-shot
                                              AllReduces of at most this many bytes per rank run in the LL form (data
                                              and flag in one 8-byte store, no barrier; same bits); 0 = off */
    HCCL_AMD_CFG_P2P_SLOT_BYTES = 18,      /* (=) HCCL_AMD_P2P_SLOT_BYTES: one data slot of the point-to-point area, a
                                              multiple of 128 in 128 .. 16 MiB (default 256 KiB, a design default that
                                              no measurement chose); read by HcclAmdCommEnableP2p */
    HCCL_AMD_CFG_P2P_IPC = 19,             /* HCCL_AMD_P2P_IPC=1: the caller wants HcclAmdCommEnableP2p at creation (the
                                              torch backend calls it then; the library itself never does) */
    HCCL_AMD_CFG_INCONSISTENT_CHECK = 20,  /* (=) HCCL_DFS_CONFIG=inconsistent_check:off|first|on: -1 (off, and the default
                                              here: unset means off, where the reference takes first), 0 (first: the first
                                              checked call of each operator type on the communicator), 1 (on: every
                                              checked call); HcclAmdCheckRecord describes the check */
    HCCL_AMD_CFG_COUNT = 21
} HcclAmdConfigKey;
extern HcclResult HcclAmdCommSetConfig(HcclComm comm, int32_t key, int64_t value);
extern HcclResult HcclAmdCommGetConfig(HcclComm comm, int32_t key, int64_t* value);
/* HCCL_DFS_CONFIG's grammar without a communicator (the reference's ParseDfsConfig): blanks removed, lower-cased, a
 * comma list of key:value items. inconsistent_check:on|first|off sets *inconsistentCheck to 1, 0 or -1 (it keeps its
 * value when the key is absent), task_exception:on|off is accepted and ignored, unknown keys are ignored.
 * HCCL_E_PARA, with *inconsistentCheck untouched, for an item that is not key:value or a value neither key takes: a
 * communicator ignores such a variable as a whole, as it ignores every other malformed one. Unset means off here; the
 * reference defaults to first. */
extern HcclResult HcclAmdParseDfsConfig(const char* text, int32_t* inconsistentCheck);
/* Re-reads comm's whole configuration from the environment, as at its creation (for test harnesses that keep one
 * communicator across cases with different environments; never called by a collective). */
extern HcclResult HcclAmdCommReloadConfig(HcclComm comm);

/* The folds of comm's last executor program while HCCL_AMD_CFG_FOLD_TIMING is on (diagnostics: the fold's operating
 * point inside a program, on staging a transport group has just written). Waits for that program's end. *folds = fold
 * launches (a batch counts once), *foldBytes = their algorithmic bytes (sum over records of (operands + 1) x count x
 * element size), *foldUs = the sum of their durations (HIP events around each launch on its stream), *spanUs = the
 * program's span on the caller's stream. HCCL_E_NOT_SUPPORT when no timed program ran (timing off, the one-sided
 * kernel, a capture). */
extern HcclResult HcclAmdCommFoldTiming(HcclComm comm, uint64_t* folds, uint64_t* foldBytes, double* foldUs,
                                        double* spanUs);


/* Runs one rank's IR program on comm's executor: what every collective runs after it has built its schedule (SEND/RECV
 * groups on the transport, folds and copies on the reduce stream, the cross-stream waits derived from the records'
 * byte ranges; singleStream != 0 puts everything on `stream` in program order). Collective over the peers the program
 * names, whose programs must post matching groups. For custom schedules and for testing the transport and executor.
 * Records are checked for form (kind, operand count, peer < rank count, buffer ids; staging inside the communicator's
 * staging); the extents of sendBuf / recvBuf are the caller's contract. */
extern HcclResult HcclAmdCommExecute(HcclComm comm, const HcclAmdIrOp* ops, uint64_t numOps, void* sendBuf,
                                     void* recvBuf, HcclDataType dataType, HcclReduceOp op, int32_t singleStream,
                                     aclrtStream stream);

/* Compiled-collective cache of comm: a call whose schedule parameters (operation, family, ranks, count, type, root,
 * piece size, buffer size) match an earlier one reuses its schedule and, for the same overlap of sendBuf / recvBuf /
 * staging, its executor plan (up to 32 entries, least recently used evicted; HCCL_AMD_PLAN_CACHE=0 disables it).
 * *hits and *misses count the RCCL-path calls that reused or built one. */
extern HcclResult HcclAmdCommCompileStats(HcclComm comm, uint64_t* hits, uint64_t* misses);

/* Executor graphs of comm (RCCL path, two-stream programs): *launches = calls served by one hipGraphLaunch of a
 * captured program, *captures = programs captured. A compiled collective runs eagerly the first time; later calls with
 * the same buffers, stream, dtype and op replay its graph. HCCL_AMD_GRAPH_CACHE = graphs kept per communicator
 * (default 16, least recently used evicted; 0 = every call eager). */
extern HcclResult HcclAmdCommGraphStats(HcclComm comm, uint64_t* launches, uint64_t* captures);

/* Status of the IPC path of comm (synchronous read). Bit 0: a cross-rank wait exceeded the communicator's bound
 * (HCCL_AMD_CFG_IPC_TIMEOUT_MS: HCCL_AMD_IPC_TIMEOUT_MS, else HCCL_EXEC_TIMEOUT's AIV rule, default 1091 s) — the
 * results of that and every later IPC collective on comm are invalid (sticky: the communicator is failed, as after an
 * asynchronous error). Bit 1: the cross-rank argument check found inconsistent arguments (bit 0 is then set too;
 * HcclAmdCommInconsistency has the report). Bits 8-15: bit length of the longest wait of the last IPC collective, in polls (diagnostic;
 * 0 = no block ever waited). */
extern HcclResult HcclAmdCommIpcStatus(HcclComm comm, uint32_t* status);

/* ---- the cross-rank argument check (HCCL_DFS_CONFIG=inconsistent_check:on|first; HCCL_AMD_CFG_INCONSISTENT_CHECK)
 *
 * With the switch on, a checked collective (AllReduce, ReduceScatter, ReduceScatterV, Reduce, AllGather, AllGatherV,
 * Broadcast, Scatter, AlltoAll, AlltoAllV, AlltoAllVC, Barrier) is preceded on its stream by a one-wave kernel that sends
 * this rank's call record to every peer and compares every peer's with its own (the reference's OpExchangeInfo,
 * src/common/inconsistent_check.cc). A difference fails the communicator with HCCL_E_PARA instead of leaving the ranks
 * in the collective until a time-out. The record is HCCL_AMD_CHECK_WORDS 32-bit words; 64-bit fields take two, low
 * word first. The fields are compared in the order of HcclAmdCheckField, which is the reference's, and the first one
 * that differs from the lowest differing peer is reported. */
enum {
    HCCL_AMD_CHECK_OP_ALLTOALLV = 10, /* the record's operator: HcclAmdOpType (6 = AlltoAll), and these two */
    HCCL_AMD_CHECK_OP_ALLTOALLVC = 11
};
typedef enum {
    HCCL_AMD_CHECK_BUFFER_SIZE = 0,    /* "HcclBufferSize": the communicator's HCCL_BUFFSIZE in bytes (words 0-1) */
    HCCL_AMD_CHECK_ROOT = 1,           /* "RootRankId": 0xFFFFFFFF for an operator without a root (word 2) */
    HCCL_AMD_CHECK_OP_TYPE = 2,        /* "OpType" (word 3) */
    HCCL_AMD_CHECK_EXECUTE_CONFIG = 3, /* "OpExecuteConfig": HCCL_AMD_CFG_EXPANSION_MODE_AIV (word 4) */
    HCCL_AMD_CHECK_REDUCE_OP = 4,      /* "HcclReduceOp": HCCL_REDUCE_RESERVED for an operator without one (word 5) */
    HCCL_AMD_CHECK_DATA_TYPE = 5,      /* "HcclDataType": HCCL_DATA_TYPE_RESERVED for the barrier (word 6) */
    HCCL_AMD_CHECK_COUNT = 6,          /* "DataCount": count (AlltoAll: sendCount); 0 for AlltoAllV, AlltoAllVC,
                                          AllGatherV and ReduceScatterV, whose counts differ by rank (words 7-8) */
    HCCL_AMD_CHECK_AIV_CORE_LIMIT = 7, /* "AivCoreLimit": HCCL_AMD_CFG_AIV_CORE_LIMIT; an error here, where the reference
                                          only warns, because the (=) keys change the one-sided geometry (word 9) */
    HCCL_AMD_CHECK_DETERMINISTIC = 8,  /* "HcclDeterministic": HCCL_AMD_CFG_DETERMINISTIC_STRICT; this library's own
                                          field, the reference's record has none (word 10) */
    HCCL_AMD_CHECK_FIELDS = 9
} HcclAmdCheckField;
#define HCCL_AMD_CHECK_WORDS 11
typedef struct {
    uint32_t w[HCCL_AMD_CHECK_WORDS];
} HcclAmdCheckRecordWords;
/* Fills the record of one call (pure host arithmetic, no communicator). opType is the record's operator, root the
 * caller's root (ignored for an operator without one), op and dataType likewise, count the operator's count by the rule
 * above. HCCL_E_PARA for an operator that is not checked, HCCL_E_PTR for a null record. */
extern HcclResult HcclAmdCheckRecord(int32_t opType, uint32_t root, HcclReduceOp op, HcclDataType dataType,
                                     uint64_t count, uint64_t bufferBytes, int32_t expansionAiv, int32_t strict,
                                     uint32_t aivCoreLimit, HcclAmdCheckRecordWords* record);
/* The name of a field as the reference spells it ("DataCount", ...), NULL for an index that is none. */
extern const char* HcclAmdCheckFieldName(int32_t field);

/* The difference a failed check recorded on comm (synchronous read of device words): the peer whose record differed
 * (the lowest such peer), the field and both values. HCCL_E_NOT_FOUND when none was recorded. One report is kept per
 * communicator: a failed check fails the communicator, so there is no second one. */
typedef struct {
    uint32_t peer;
    int32_t field;     /* HcclAmdCheckField */
    char name[24];     /* HcclAmdCheckFieldName(field) */
    uint64_t local;    /* this rank's value */
    uint64_t remote;   /* the peer's */
} HcclAmdInconsistency;
extern HcclResult HcclAmdCommInconsistency(HcclComm comm, HcclAmdInconsistency* info);

/* Check kernels comm has run so far (synchronous read of the check's device sequence word, which every check launch
 * advances; 0 before the first). Diagnostics: the `first` mode's tests count launches with it. */
extern HcclResult HcclAmdCommCheckLaunches(HcclComm comm, uint32_t* launches);

/* One-sided launches of comm that ran in the LL form so far (HCCL_AMD_CFG_IPC_LL_BYTES; synchronous read of the
 * device's LL sequence word; in a loopback world the launches count on rank 0's communicator, which issues them). */
extern HcclResult HcclAmdCommIpcLlLaunches(HcclComm comm, uint32_t* launches);

/* Phase timeline of the one-sided kernel (diagnostics). With HCCL_AMD_IPC_TRACE=1 set when comm makes its first IPC
 * call, every launch stamps, per rank and workgroup, 8 s_memrealtime values (100 MHz) of its last staging round:
 * entry, round start, phase 0 issued, barrier 1 passed, phase 1 issued, barrier 2 passed, phase 2 issued, exit.
 * Synchronises the device and copies the last launch's stamps into stamps[rank][block][8] (cap >= 16 x 512 x 8
 * entries; in a loopback world call it on rank 0, which issues the world's launch); *blocks = workgroups per rank of
 * that launch. HCCL_E_NOT_SUPPORT when tracing is off. */
extern HcclResult HcclAmdCommIpcTrace(HcclComm comm, uint64_t* stamps, uint64_t cap, uint32_t* blocks);

/* The barrier wait bound of the one-sided kernel in ms, as the next IPC call would take it from the environment:
 * HCCL_AMD_IPC_TIMEOUT_MS if set (1 .. 3600000), else HCCL_EXEC_TIMEOUT by the reference's AIV-mode rule (seconds,
 * at most two decimals; 0, above 1091 or unset = 1091 s). A wait past it fails the communicator (HcclGetCommAsyncError). */
extern uint64_t HcclAmdIpcTimeoutMs(void);

/* Parse and validate a rank table (as HcclCommInitClusterInfo does): *nRanks = number of ranks, *deviceId = the
 * device_id of `rank`. HCCL_E_PARA for a malformed table or a rank outside it. */
extern HcclResult HcclAmdRankTableInfo(const char* clusterInfo, uint32_t rank, uint32_t* nRanks, int32_t* deviceId);

/* The last HcclCommInitClusterInfo of this process: *stage = 0 (none, or it failed before the unique-id exchange
 * completed), 1 (the transport's unique id was exchanged over TCP; *idDigest = FNV-1a 64 of the 128-byte id, the same
 * on every rank of a good exchange), 2 (the RCCL communicator was then created). Diagnostics for bootstrap tests. */
extern HcclResult HcclAmdLastBootstrap(uint64_t* idDigest, int32_t* stage);

/* The rank-table TCP exchange alone (host only, no device): rank 0 serves the 128 bytes at id128 to every other
 * rank of the table, which receive them into id128. Same addresses and bounds as HcclCommInitClusterInfo. */
extern HcclResult HcclAmdBootstrapExchangeId(const char* clusterInfo, uint32_t rank, void* id128);

/* Host time by category, accumulated while HCCL_AMD_HOST_PROFILE=1 (read at library load): ns[i] and calls[i] for
 * i < n of the categories below; reset != 0 zeroes them afterwards. Diagnostics of the enqueue cost. */
enum {
    HCCL_AMD_HP_EXECUTE = 0, /* a whole Execute call */
    HCCL_AMD_HP_GROUP = 1,   /* transport groups (ncclGroupStart .. ncclGroupEnd) */
    HCCL_AMD_HP_FOLD = 2,    /* fold launches */
    HCCL_AMD_HP_COPY = 3,    /* copy launches */
    HCCL_AMD_HP_RECORD = 4,  /* unit event records */
    HCCL_AMD_HP_WAIT = 5,    /* cross-stream waits */
    HCCL_AMD_HP_PLAN = 6,    /* planning outside the compiled-collective cache */
    HCCL_AMD_HP_ENTRY = 7,   /* a whole collective call past its argument checks (HcclAllReduce, HcclReduceScatter,
                                HcclReduceScatterV, HcclReduce, HcclAllGather, HcclBroadcast, HcclAlltoAll,
                                HcclAlltoAllV, HcclAlltoAllVC, HcclBarrier): lock, selection, every enqueue */
    HCCL_AMD_HP_IPC = 8,     /* the one-sided kernel's host side: launch arguments and the launch (RunIpcPlan) */
    HCCL_AMD_HP_COUNT = 9
};
extern HcclResult HcclAmdHostProfile(uint64_t* ns, uint64_t* calls, uint32_t n, int32_t reset);

/* Communicators whose HcclCommDestroy is waiting for the graphs captured on them to be destroyed. */
extern uint32_t HcclAmdCommPendingDestroys(void);

/* RCCL's p2p channel settings of this process as requested through the environment: *perPeer =
 * NCCL_NCHANNELS_PER_PEER, *minP2pChannels = NCCL_MIN_P2P_NCHANNELS (0 when unset). Opt-in: only when
 * HCCL_AMD_P2P_CHANNELS_PER_PEER=k > 0 does the library, when it is loaded, set NCCL_NCHANNELS_PER_PEER = k rounded
 * up to a power of two and
 * NCCL_MIN_P2P_NCHANNELS = (the per-peer value in effect) x 7 rounded up to a power of two, at most 64, each unless the
 * caller set it (RCCL's p2p kernel streams about 43 GB/s per channel, an xGMI link 76.8 GB/s per direction). RCCL reads
 * them once per process, at its first communicator, so these are requests: RCCL's INIT log says what it set up.
 * Child processes inherit them. */
extern HcclResult HcclAmdRcclP2pChannels(uint32_t* perPeer, uint32_t* minP2pChannels);

/* The executor staging of comm (diagnostics): *ptr = its device address (NULL until allocated), *bytes = its size. */
extern HcclResult HcclAmdCommScratch(HcclComm comm, void** ptr, uint64_t* bytes);

/* The device memory the library holds for comm now, in bytes: the executor staging (2 x HCCL_BUFFSIZE, allocated by
 * the first collective that runs a schedule) plus the one-sided kernel's allocations (flags and LL area, status words
 * and unpack area at its first call; the small staging tier, n x HCCL_AMD_SMALL_IPC_BYTES per area, and the large
 * one, 2 x HCCL_BUFFSIZE, each at the first call that needs it) plus the 256 token bytes of the first HcclBarrier that
 * runs a schedule. RCCL's own buffers are not included. */
extern HcclResult HcclAmdCommDeviceBytes(HcclComm comm, uint64_t* bytes);

/* The one-sided path's uncached allocations outlive the communicator that made them: a destroyed communicator's
 * blocks stay with the process and serve the next communicator's set-up of the same size on the same device. *bytes =
 * the idle blocks' total size. They are never freed while the process runs: freeing memory allocated with
 * hipDeviceMallocUncached corrupts later GPU work on this stack (lost operands and memory aperture violations after
 * such frees), so release != 0 returns HCCL_E_NOT_SUPPORT after reporting. A block serves
 * only a request of its own size: communicators of other sizes (rank count, HCCL_BUFFSIZE) allocate their own. */
extern HcclResult HcclAmdIpcIdleStaging(int32_t release, uint64_t* bytes);

/* Enqueues on `stream` a system-scope write-back and invalidate of every XCD's L2 of the current device (one
 * workgroup per CU runs buffer_wbl2 sc0 sc1 / buffer_inv sc0 sc1) and waits for it. Diagnostics: a kernel launched
 * after it reads every line from memory. */
extern HcclResult HcclAmdL2Maintain(aclrtStream stream);

/* Enqueues on `stream` a read of `words` 4-byte words at device address p by 256 workgroups (dealt over the XCDs),
 * each reading the whole range with plain loads (nonTemporal = 0) or non-temporal loads (1) and comparing it with the
 * device array `expect`. out (device, 768 uint32) receives {mismatching words, zero words, XCC id} per workgroup.
 * Diagnostics: which XCDs see stale or unwritten lines of a buffer. */
extern HcclResult HcclAmdDiagReadByXcc(const void* p, const void* expect, uint64_t words, int32_t nonTemporal,
                                       void* out, aclrtStream stream);

/* Blocking host all-gather supplied by the caller's bootstrap (a TCP store, MPI, torch.distributed gloo ...):
 * gathers `bytes` bytes from every rank into all[nRanks * bytes] in rank order; returns 0 on success. */
typedef int32_t (*HcclAmdHostAllGatherFn)(void* ctx, const void* mine, uint64_t bytes, void* all);

/* Rank `rank` of an IPC-only communicator on the current HIP device, bootstrapped through `fn` instead of RCCL.
 * Its data path is the one-sided kernel over peer-mapped memory opened with hipIpcOpenMemHandle:
 * HCCL_AMD_ALGO_IPC_TWOSHOT (the default on such a communicator), HCCL_AMD_ALGO_IPC_RHD when RHD or IPC_RHD is set
 * (AllReduce, power-of-two ranks), otherwise HCCL_AMD_ALGO_IPC whatever family is set. Every operator has an IPC form,
 * HcclReduceScatterV included (per-rank blocks, order O1).
 * Ranks may share a device (separate processes), which is how the rank-mode IPC path is tested on one GPU.
 * `fn` and `ctx` must stay valid for the communicator's lifetime. */
extern HcclResult HcclAmdCommInitHostExchange(uint32_t nRanks, uint32_t rank, HcclAmdHostAllGatherFn fn, void* ctx,
                                              HcclComm* comm);

/* A stand-in for one rank of an nRanks-rank communicator on one GPU (benchmark and test harnesses; never a data
 * path): rank `rank`'s schedules run through a one-rank RCCL communicator with every peer mapped onto itself. Each
 * transport group's sends are paired with its receives of the same size (RCCL pairs messages to itself in posting
 * order), so every program keeps the schedule's shape (groups, pieces, staging, folds, waits, graph capture) and runs
 * through RCCL's kernels, while the data no longer means the collective. Sends and receives of a group whose sizes
 * differ (a ragged last chunk) are paired in order at the smaller size; a surplus on either side is dropped. The
 * one-sided kernel is unavailable (HCCL_E_NOT_SUPPORT; the small-call rule falls back to the schedule). */
extern HcclResult HcclAmdCommInitSelfLoop(uint32_t nRanks, uint32_t rank, HcclComm* comm);

#ifdef __cplusplus
}
#endif
#endif /* HCCL_AMD_EXT_H_ */
