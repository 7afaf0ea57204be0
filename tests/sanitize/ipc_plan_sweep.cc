// Host-code sanitizer run (ASan + UBSan) of the one-sided path's planner (hccl_amd/csrc/ipc_plan.cc): every operation
// x family that has a one-sided plan, the AIV variants, RHD's plan and the V plan, for 2..16 ranks, every element size
// and counts up to SYS_MAX_COUNT, with the default and the smallest staging tiers, and for every launch the invariants
// the kernels rely on without checking: the piece is a non-zero multiple of 16 B whose slots (and results) fit their
// area, the blocks' shares cover the piece, the rounds cover the widest chunk, the barrier epochs match the rounds, and
// the LL form is taken only for one round of at most kIpcLlMaxBytes. Overflow or a division by zero anywhere ends the
// run. Built and run by tests/test_sanitize.py; test infrastructure only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../hccl_amd/csrc/ipc_plan.h"

using namespace hccl_amd;

namespace {

constexpr uint64_t kSysMaxCount = 0x7FFFFFFFFull;  // SYS_MAX_COUNT: the largest count an operator accepts
constexpr uint64_t kCclBytes = 200ull << 20;       // HCCL_BUFFSIZE's default

long g_cases = 0, g_launches = 0, g_failures = 0;

#define EXPECT(cond)                                                                                        \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            if (++g_failures <= 20) {                                                                       \
                std::printf("FAIL %s: op %d family %d kind %u geom %u n %u es %llu count %llu tiers %d\n", #cond, \
                            q.opType, q.family, q.kind, q.geom, q.nRanks, (unsigned long long)es,           \
                            (unsigned long long)q.count, smallest ? 1 : 0);                                 \
            }                                                                                               \
            return;                                                                                         \
        }                                                                                                   \
    } while (0)

// Plans q with the default tiers or the smallest ones a configuration allows (1 MiB large areas, n x 64 KiB small
// ones) and checks every launch.
void Check(const HcclAmdIpcPlanQuery& q, uint64_t es, bool smallest)
{
    HcclAmdIpcPlanResult res{};
    std::vector<IpcGeometry> launches;
    const HcclResult r = IpcPlanQuery(q, es, kCclBytes, smallest ? 1 : 0, smallest ? 0 : 1ull << 20, &res, &launches);
    ++g_cases;
    EXPECT(r == HCCL_SUCCESS);
    EXPECT(res.blocks >= 1 && res.blocks <= kIpcMaxBlocks);
    EXPECT(res.numLaunches == launches.size() && !launches.empty());
    const uint64_t n = q.nRanks, V = 16 / es;
    // the kind and layout of the plan the query stands for
    uint32_t kind = q.kind, geom = q.geom;
    if (q.family >= 0) {
        IpcPlan p{};
        if (q.opType == HCCL_AMD_OP_BROADCAST) {
            p = IpcPlanBroadcast(q.count, es, q.family == HCCL_AMD_ALGO_AUTO ? 0 : q.family == HCCL_AMD_ALGO_MESH_TWOSHOT ? 1 : 2);
        } else if (q.family == HCCL_AMD_ALGO_IPC_RHD) {
            EXPECT(IpcPlanRhd(q.nRanks, &p) == HCCL_SUCCESS);
        } else {
            EXPECT(IpcPlanForFamily(q.opType, q.family, q.nRanks, es, kCclBytes, &p) == HCCL_SUCCESS);
        }
        kind = p.kind;
        geom = p.geom;
    }
    const bool single = HostSingleBarrierKind(kind);
    const uint64_t slots = kind == kIpcBroadcastOneShot ? 1 : n;
    uint64_t covered = 0;
    for (const IpcGeometry& g : launches) {
        ++g_launches;
        const uint64_t widest = g.balanced != 0 ? g.group * g.chunkLen + std::min(g.group, g.rem) : g.chunkLen;
        EXPECT(g.piece != 0 && g.piece % V == 0);
        EXPECT(g.blockElems % V == 0 && g.blockElems * res.blocks >= g.piece);
        EXPECT(g.tileElems % V == 0);
        EXPECT(g.rounds >= 1 && uint64_t(g.rounds) * g.piece >= widest && uint64_t(g.rounds - 1) * g.piece <= widest);
        EXPECT(g.rounds == 1 || uint64_t(g.rounds - 1) * g.piece < widest);
        if (g.ll != 0) {
            EXPECT(res.ll == 1 && q.llBytes != 0 && g.rounds == 1 && g.epochSpan == 0 && g.tileElems == 0);
            EXPECT(widest * es <= kIpcLlMaxBytes && widest * es <= q.llBytes && g.piece * es <= kIpcLlMaxBytes);
        } else {
            EXPECT(g.epochSpan == (single ? 1u : 2u) * g.rounds);
            EXPECT(g.piece * slots * es <= (single ? res.altBytes : res.areaBytes));
            EXPECT(single || g.piece * n * es <= res.areaBytes);  // the result area: chunk c at c * piece
        }
        // the chunks tile the launch
        if (g.vgeom != 0) {
            for (uint32_t c = 0; c < n; ++c) EXPECT(g.vLen[c] == q.counts[c] && g.vStart[c] == q.displs[c]);
            EXPECT(launches.size() == 1);
            covered = q.count;
        } else if (g.balanced != 0) {
            EXPECT(g.group >= 1 && g.group * n * g.chunkLen + g.rem == g.total && g.rem < g.group * n);
            covered += g.total;
        } else if (geom == kIpcGeomBlock) {  // the loop's elements of every block
            EXPECT(g.chunkStride == q.count && g.total == (n - 1) * q.count + g.chunkLen);
            covered += g.chunkLen;
        } else {
            EXPECT(g.chunkStride == 0 ? g.chunkLen == g.total : (g.chunkStride == g.chunkLen && n * g.chunkLen >= g.total));
            covered += g.total;
        }
    }
    EXPECT(covered == q.count);
    EXPECT(res.ll == 0 || (launches.size() == 1 && launches[0].ll == 1));
}

void CheckBoth(HcclAmdIpcPlanQuery q, uint64_t es)
{
    for (const uint32_t blocks : {0u, 1u, 512u}) {
        q.blocks = blocks;
        q.sharedDevice = blocks == 0 ? 1 : 0;
        q.residentPerRank = blocks == 512 ? 96 : 0;
        q.llBytes = blocks == 1 ? 0 : kIpcLlMaxBytes;
        q.tileBytes = blocks == 512 ? 64 << 10 : 0;
        Check(q, es, false);
        Check(q, es, true);
    }
}

void Rejects(const HcclAmdIpcPlanQuery& q, uint64_t es)
{
    HcclAmdIpcPlanResult res{};
    ++g_cases;
    if (IpcPlanQuery(q, es, kCclBytes, 0, 1ull << 20, &res, nullptr) != HCCL_E_PARA) {
        ++g_failures;
        std::printf("FAIL not rejected: n %u es %llu group %u geom %u\n", q.nRanks, (unsigned long long)es, q.group, q.geom);
    }
}

}  // namespace

int main()
{
    const uint64_t counts[] = {1, 2, 5, 33, 4099, 100003, (1ull << 31) + 3, kSysMaxCount};
    const int32_t dtypes[] = {HCCL_DATA_TYPE_INT8, HCCL_DATA_TYPE_FP16, HCCL_DATA_TYPE_FP32, HCCL_DATA_TYPE_INT64};
    const int32_t ops[] = {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_OP_REDUCE, HCCL_AMD_OP_ALLGATHER};
    const int32_t families[] = {HCCL_AMD_ALGO_MESH_ONESHOT, HCCL_AMD_ALGO_MESH_TWOSHOT, HCCL_AMD_ALGO_MESH_CHUNK};
    for (uint32_t n = 2; n <= 16; ++n) {
        for (int d = 0; d < 4; ++d) {
            const uint64_t es = 1ull << d;
            for (const uint64_t count : counts) {
                HcclAmdIpcPlanQuery q{};
                q.nRanks = n;
                q.count = count;
                q.dataType = dtypes[d];
                q.group = 1;
                for (const int32_t op : ops) {
                    for (const int32_t family : families) {
                        q.opType = op;
                        q.family = family;
                        CheckBoth(q, es);
                    }
                }
                q.opType = HCCL_AMD_OP_BROADCAST;
                for (const int32_t family : {HCCL_AMD_ALGO_AUTO, HCCL_AMD_ALGO_MESH_ONESHOT, HCCL_AMD_ALGO_MESH_TWOSHOT}) {
                    q.family = family;
                    CheckBoth(q, es);
                }
                IpcPlan p{};
                if (IpcPlanRhd(n, &p) == HCCL_SUCCESS) {
                    q.opType = HCCL_AMD_OP_ALLREDUCE;
                    q.family = HCCL_AMD_ALGO_IPC_RHD;
                    CheckBoth(q, es);
                }
                // the AIV engine's variants for the default core count, a small one and AIV_ONLY (no size bound)
                q.family = -1;
                for (const int32_t op : {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_OP_REDUCE_SCATTER}) {
                    for (const uint32_t cores : {48u, 8u, 1u}) {
                        for (const bool aivOnly : {false, true}) {
                            if (SelectAivPlan(op, n, count, static_cast<HcclDataType>(dtypes[d]), es, HCCL_REDUCE_SUM, false,
                                              aivOnly, kCclBytes, cores, &p, nullptr) == HCCL_AMD_AIV_NOT_MATCHED) {
                                continue;
                            }
                            q.opType = op;
                            q.kind = p.kind;
                            q.order = p.order;
                            q.geom = p.geom;
                            q.group = p.group;
                            q.subMode = p.subMode;
                            q.loopElems = p.loopElems;
                            CheckBoth(q, es);
                        }
                    }
                }
                // ReduceScatterV: ragged blocks with gaps, one of them empty
                std::vector<uint64_t> vc(n), vd(n);
                for (uint32_t c = 0; c < n; ++c) {
                    vc[c] = c == 1 ? 0 : count / (c + 1);
                    vd[c] = c == 0 ? 3 : vd[c - 1] + vc[c - 1] + c;
                }
                q.opType = HCCL_AMD_OP_REDUCE_SCATTER;
                q.kind = kIpcReduceScatter;
                q.order = kIpcO1;
                q.geom = kIpcGeomV;
                q.group = 1;
                q.subMode = 0;
                q.loopElems = 0;
                q.counts = vc.data();
                q.displs = vd.data();
                q.count = vc[0];
                CheckBoth(q, es);
            }
        }
    }
    // what no operator passes on
    HcclAmdIpcPlanQuery q{};
    q.opType = HCCL_AMD_OP_REDUCE_SCATTER;
    q.family = HCCL_AMD_ALGO_MESH_CHUNK;  // divides by n - 1
    q.count = 100;
    q.group = 1;
    for (const uint32_t n : {0u, 1u, 17u}) {
        q.nRanks = n;
        Rejects(q, 4);
    }
    q.nRanks = 4;
    for (const uint64_t es : {0ull, 3ull, 16ull}) Rejects(q, es);
    q.family = -1;
    q.kind = kIpcAllReduce;
    q.geom = kIpcGeomBalanced;
    q.group = 0;
    Rejects(q, 4);
    q.group = 1;
    q.geom = kIpcGeomV;  // without its tables
    Rejects(q, 4);
    q.geom = 6;
    Rejects(q, 4);
    std::printf("cases %ld launches %ld failures %ld\n", g_cases, g_launches, g_failures);
    return g_failures == 0 ? 0 : 1;
}
