// Host-code sanitizer run (ASan + UBSan) of what HcclScatter and HcclAllGatherV add to the host side: the planner's
// functions for kinds kIpcScatter and kIpcAllGatherV (hccl_amd/csrc/ipc_plan.cc) and the two schedule generators
// (hccl_amd/csrc/schedule.cc, ops HCCL_AMD_OP_SCATTER and HCCL_AMD_OP_ALLGATHER_V), over 2..16 ranks, every element
// size, counts from 1 to SYS_MAX_COUNT and count vectors with zeros and one huge entry.
// Planner: the piece is a non-zero multiple of 16 B, the slots (one for the Scatter, n for the AllGatherV) fit the
// alternate area, the blocks' shares cover the piece and the rounds cover the largest block exactly. Schedule: only COPY
// / SEND / RECV records inside the declared blocks, no staging, and every sender's pieces are the receiver's, group by
// group. Overflow or a division by zero anywhere ends the run. Built and run by tests/test_sanitize_scatter_gatherv.py;
// test infrastructure only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <tuple>
#include <vector>

#include "../../hccl_amd/csrc/ipc_plan.h"
#include "../../hccl_amd/csrc/schedule.h"

using namespace hccl_amd;

namespace {

constexpr uint64_t kSysMaxCount = 0x7FFFFFFFFull;  // SYS_MAX_COUNT
constexpr uint64_t kCclBytes = 200ull << 20;

long g_cases = 0, g_failures = 0;

#define EXPECT(cond)                                                                                     \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            if (++g_failures <= 20) std::printf("FAIL %s (line %d): n %u es %llu\n", #cond, __LINE__, n, \
                                                (unsigned long long)es);                                 \
            return;                                                                                      \
        }                                                                                                \
    } while (0)

uint64_t g_rng = 88172645463325252ull;
uint64_t Rand()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

void CheckPlan(uint32_t n, uint64_t es, bool scatter, const std::vector<uint64_t>& counts,
               const std::vector<uint64_t>& displs, bool smallest, bool shared)
{
    HcclAmdIpcPlanQuery q{};
    q.opType = scatter ? HCCL_AMD_OP_SCATTER : HCCL_AMD_OP_ALLGATHER_V;
    q.family = HCCL_AMD_ALGO_AUTO;
    q.group = 1;
    q.nRanks = n;
    q.count = counts[0];
    q.counts = scatter ? nullptr : counts.data();
    q.displs = scatter ? nullptr : displs.data();
    q.sharedDevice = shared ? 1 : 0;
    q.residentPerRank = shared ? 1536 / n : 0;
    HcclAmdIpcPlanResult res{};
    std::vector<IpcGeometry> launches;
    const HcclResult r = IpcPlanQuery(q, es, kCclBytes, smallest ? 1 : 0, smallest ? 0 : 1ull << 20, &res, &launches);
    ++g_cases;
    EXPECT(r == HCCL_SUCCESS);
    EXPECT(res.blocks >= 1 && res.blocks <= kIpcMaxBlocks && res.ll == 0);
    EXPECT(launches.size() == 1 && res.numLaunches == 1);
    const IpcGeometry& g = launches[0];
    const uint64_t V = 16 / es;
    const uint64_t widest = scatter ? counts[0] : *std::max_element(counts.begin(), counts.end());
    EXPECT(g.piece != 0 && g.piece % V == 0);
    EXPECT(g.piece * (scatter ? 1 : n) * es <= res.altBytes);
    EXPECT(g.blockElems % V == 0 && g.blockElems * res.blocks >= g.piece && g.tileElems % V == 0);
    EXPECT(g.ll == 0 && g.balanced == 0 && g.vgeom == (scatter ? 0u : 1u));
    EXPECT(g.epochSpan == g.rounds);
    EXPECT(uint64_t(g.rounds) * g.piece >= widest);
    EXPECT(g.rounds == 0 ? widest == 0 : uint64_t(g.rounds - 1) * g.piece < widest);
    if (scatter) {
        EXPECT(g.chunkStride == counts[0] && g.chunkLen == counts[0] && g.total == uint64_t(n) * counts[0]);
    } else {
        for (uint32_t c = 0; c < n; ++c) EXPECT(g.vStart[c] == displs[c] && g.vLen[c] == counts[c]);
    }
}

// (sender, receiver) -> the pieces (group, elements) in posting order
using Pieces = std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<int32_t, uint64_t>>>;

void CheckSchedule(uint32_t n, uint64_t es, bool scatter, uint32_t root, const std::vector<uint64_t>& counts,
                   const std::vector<uint64_t>& displs, bool inPlace, uint64_t pieceBytes)
{
    Pieces sent, received;
    for (uint32_t rank = 0; rank < n; ++rank) {
        ScheduleParams p;
        p.opType = scatter ? HCCL_AMD_OP_SCATTER : HCCL_AMD_OP_ALLGATHER_V;
        p.nRanks = n;
        p.rank = rank;
        p.elemSize = static_cast<uint32_t>(es);
        p.pieceBytes = pieceBytes;
        p.root = root;
        p.count = scatter ? counts[0] : counts[rank];
        if (!scatter) {
            p.counts = counts;
            p.displs = displs;
            p.inPlace = inPlace;
        }
        Schedule s;
        ++g_cases;
        EXPECT(BuildSchedule(p, &s) == HCCL_SUCCESS);
        EXPECT(s.scratchElems == 0 && s.algo == HCCL_AMD_ALGO_MESH_ONESHOT);
        uint64_t copies = 0;
        for (const HcclAmdIrOp& o : s.ops) {
            EXPECT(o.kind == HCCL_AMD_IR_COPY || o.kind == HCCL_AMD_IR_SEND || o.kind == HCCL_AMD_IR_RECV);
            EXPECT(o.count != 0);
            if (o.kind != HCCL_AMD_IR_RECV) {
                // reads stay inside the input: the root's n blocks, or this rank's own block
                EXPECT(o.nsrc == 1 && o.srcBuf[0] == HCCL_AMD_BUF_INPUT);
                const uint64_t inElems = scatter ? uint64_t(n) * counts[0] : counts[rank];
                EXPECT(o.srcOff[0] <= inElems && o.count <= inElems - o.srcOff[0]);
                EXPECT(!scatter || rank == root);
            }
            if (o.kind != HCCL_AMD_IR_SEND) {
                // writes stay inside one declared block of the output
                EXPECT(o.dstBuf == HCCL_AMD_BUF_OUTPUT);
                const uint32_t from = o.kind == HCCL_AMD_IR_COPY ? rank : static_cast<uint32_t>(o.peer);
                const uint64_t lo = scatter ? 0 : displs[from], len = scatter ? counts[0] : counts[from];
                EXPECT(o.dstOff >= lo && o.dstOff - lo <= len && o.count <= len - (o.dstOff - lo));
            }
            if (o.kind == HCCL_AMD_IR_COPY) ++copies;
            if (o.kind == HCCL_AMD_IR_SEND) sent[{rank, uint32_t(o.peer)}].push_back({o.group, o.count});
            if (o.kind == HCCL_AMD_IR_RECV) received[{uint32_t(o.peer), rank}].push_back({o.group, o.count});
        }
        if (scatter) {
            EXPECT(copies == (rank == root ? 1u : 0u));
            EXPECT(rank != root || s.ops.back().kind == HCCL_AMD_IR_COPY);  // the own block last (in-place Scatter)
        } else {
            EXPECT(copies == (inPlace || counts[rank] == 0 ? 0u : 1u));
        }
    }
    EXPECT(sent == received);
}

}  // namespace

int main()
{
    const uint64_t scalars[] = {1, 2, 17, 1000, 4099, (1ull << 20) + 3, (40ull << 20) + 1, kSysMaxCount};
    for (uint32_t n = 2; n <= 16; ++n) {
        for (uint64_t es : {1ull, 2ull, 4ull, 8ull}) {
            for (uint64_t count : scalars) {
                for (int flags = 0; flags < 4; ++flags) {
                    CheckPlan(n, es, true, {count}, {}, (flags & 1) != 0, (flags & 2) != 0);
                }
                if (count <= 4099) {
                    for (uint32_t root : {0u, n / 2, n - 1}) {
                        for (uint64_t piece : {0ull, 128ull, 4096ull}) CheckSchedule(n, es, true, root, {count}, {}, false, piece);
                    }
                }
            }
            for (int shape = 0; shape < 5; ++shape) {
                std::vector<uint64_t> counts(n), displs(n);
                uint64_t at = 0;
                for (uint32_t q = 0; q < n; ++q) {
                    switch (shape) {
                        case 0: counts[q] = 40; break;                                       // equal
                        case 1: counts[q] = Rand() % 3 == 0 ? 0 : Rand() % 5000; break;      // ragged with zeros
                        case 2: counts[q] = q == n - 1 ? 4099 : 0; break;                    // only one non-zero
                        case 3: counts[q] = q == n / 2 ? 0 : 1 + q; break;                   // one zero
                        default: counts[q] = q == 0 ? kSysMaxCount : Rand() % 2;             // one huge block
                    }
                }
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t q = shape % 2 == 0 ? i : n - 1 - i;  // ascending or descending, with gaps
                    at += Rand() % 4;
                    displs[q] = at;
                    at += counts[q];
                }
                for (int flags = 0; flags < 4; ++flags) CheckPlan(n, es, false, counts, displs, (flags & 1) != 0, (flags & 2) != 0);
                if (shape < 4) {
                    for (uint64_t piece : {0ull, 128ull, 4096ull}) {
                        CheckSchedule(n, es, false, 0, counts, displs, false, piece);
                        CheckSchedule(n, es, false, 0, counts, displs, true, piece);
                    }
                }
            }
        }
    }
    std::printf("cases %ld failures %ld\n", g_cases, g_failures);
    return g_failures == 0 ? 0 : 1;
}
