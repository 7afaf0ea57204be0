// Host-code sanitizer run (ASan + UBSan) of what the all-to-all family adds to the host side: the planner's functions
// for kind kIpcAllToAll (hccl_amd/csrc/ipc_plan.cc) and the schedule generator (hccl_amd/csrc/schedule.cc, op
// HCCL_AMD_OP_ALLTOALL), over 1..16 ranks, every element size and count matrices with zeros and one huge entry.
// Planner: the piece is a non-zero multiple of 16 B, n slots (header included) fit the alternate area, the blocks'
// shares cover the piece, the known form's rounds cover the largest pair exactly, and the agreed form's blocks, tier and
// piece are the same for every count. Schedule: only COPY / SEND / RECV records inside the declared blocks, no staging,
// pair sizes that match across ranks, and the same records whatever family is asked for. Overflow or a division by
// zero anywhere ends the run. Built and run by tests/test_sanitize_alltoall.py; test infrastructure only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

HcclAmdIpcPlanQuery Query(uint32_t n, uint64_t count, bool agreed, bool shared, uint32_t resident)
{
    HcclAmdIpcPlanQuery q{};
    q.opType = HCCL_AMD_OP_ALLTOALL;
    q.family = agreed ? -1 : HCCL_AMD_ALGO_AUTO;
    q.kind = kIpcAllToAll;
    q.geom = kIpcGeomWhole;
    q.group = 1;
    q.subMode = agreed ? kIpcA2aAgreed : kIpcA2aKnown;
    q.nRanks = n;
    q.count = count;
    q.sharedDevice = shared ? 1 : 0;
    q.residentPerRank = resident;
    return q;
}

void CheckPlan(uint32_t n, uint64_t es, uint64_t count, bool agreed, bool smallest, bool shared)
{
    const HcclAmdIpcPlanQuery q = Query(n, count, agreed, shared, shared ? 1536 / n : 0);
    HcclAmdIpcPlanResult res{};
    std::vector<IpcGeometry> launches;
    const HcclResult r = IpcPlanQuery(q, es, kCclBytes, smallest ? 1 : 0, smallest ? 0 : 1ull << 20, &res, &launches);
    ++g_cases;
    EXPECT(r == HCCL_SUCCESS);
    EXPECT(res.blocks >= 1 && res.blocks <= kIpcMaxBlocks && res.ll == 0);
    EXPECT(launches.size() == 1 && res.numLaunches == 1);
    const IpcGeometry& g = launches[0];
    const uint64_t V = 16 / es, hdr = agreed ? kIpcA2aHeaderBytes / es : 0;
    EXPECT(g.piece != 0 && g.piece % V == 0 && hdr % V == 0);
    EXPECT((g.piece + hdr) * n * es <= res.altBytes);
    EXPECT(g.blockElems % V == 0 && g.blockElems * res.blocks >= g.piece && g.tileElems % V == 0);
    EXPECT(g.ll == 0 && g.vgeom == 0 && g.balanced == 0);
    if (agreed) {
        EXPECT(g.rounds == 0 && g.epochSpan == 0);
        // count-free: the plan of any other count is the same
        HcclAmdIpcPlanResult res2{};
        std::vector<IpcGeometry> l2;
        const HcclAmdIpcPlanQuery q2 = Query(n, count ^ 0x5555555ull, agreed, shared, q.residentPerRank);
        EXPECT(IpcPlanQuery(q2, es, kCclBytes, smallest ? 1 : 0, smallest ? 0 : 1ull << 20, &res2, &l2) == HCCL_SUCCESS);
        EXPECT(res2.blocks == res.blocks && res2.altBytes == res.altBytes && res2.areaBytes == res.areaBytes);
        EXPECT(l2.size() == 1 && l2[0].piece == g.piece && l2[0].blockElems == g.blockElems);
        const IpcTierBytes small = IpcTierSizes(n, kCclBytes, smallest ? 1 : 0, smallest ? 0 : 1ull << 20, kIpcTierSmall);
        EXPECT(res.altBytes == small.altBytes);
    } else {
        EXPECT(g.rounds >= 1 && g.epochSpan == g.rounds);
        EXPECT(uint64_t(g.rounds) * g.piece >= count);
        EXPECT(g.rounds == 1 || uint64_t(g.rounds - 1) * g.piece < count);
    }
}

struct Matrix {
    uint32_t n;
    std::vector<uint64_t> m;  // m[p * n + q]: elements p sends to q
    uint64_t at(uint32_t p, uint32_t q) const { return m[size_t(p) * n + q]; }
};

Matrix MakeMatrix(uint32_t n, int shape)
{
    Matrix x{n, std::vector<uint64_t>(size_t(n) * n, 0)};
    for (uint32_t p = 0; p < n; ++p) {
        for (uint32_t q = 0; q < n; ++q) {
            uint64_t v = 0;
            switch (shape) {
                case 0: v = 5; break;                                            // even
                case 1: v = Rand() % 3 == 0 ? 0 : Rand() % 400; break;           // random with zeros
                case 2: v = p == n / 2 ? 0 : 1 + p + q; break;                   // a zero row
                case 3: v = q == n - 1 ? 0 : 2 + p * q; break;                   // a zero column
                case 4: v = 0; break;                                            // all zero
                default: v = p == 0 && q == n - 1 ? kSysMaxCount : Rand() % 2;   // one huge entry
            }
            x.m[size_t(p) * n + q] = v;
        }
    }
    return x;
}

void CheckSchedule(const Matrix& x, uint64_t es, uint64_t pieceBytes, uint64_t gap)
{
    const uint32_t n = x.n;
    std::vector<Schedule> scheds(n);
    std::vector<std::vector<uint64_t>> sd(n), rd(n), sc(n), rc(n);
    for (uint32_t r = 0; r < n; ++r) {
        ScheduleParams p;
        p.opType = HCCL_AMD_OP_ALLTOALL;
        p.nRanks = n;
        p.rank = r;
        p.elemSize = static_cast<uint32_t>(es);
        p.pieceBytes = pieceBytes;
        uint64_t so = 0, ro = 0;
        for (uint32_t q = 0; q < n; ++q) {
            so += gap;
            ro += gap + q;
            p.counts.push_back(x.at(r, q));
            p.displs.push_back(so);
            p.recvCounts.push_back(x.at(q, r));
            p.recvDispls.push_back(ro);
            so += x.at(r, q);
            ro += x.at(q, r);
        }
        sc[r] = p.counts, sd[r] = p.displs, rc[r] = p.recvCounts, rd[r] = p.recvDispls;
        ++g_cases;
        EXPECT(BuildSchedule(p, &scheds[r]) == HCCL_SUCCESS);
        EXPECT(scheds[r].scratchElems == 0 && scheds[r].algo == HCCL_AMD_ALGO_MESH_ONESHOT);
        for (int32_t algo = HCCL_AMD_ALGO_AUTO; algo <= HCCL_AMD_ALGO_IPC_RHD; ++algo) {
            ScheduleParams pa = p;
            pa.algo = algo;
            Schedule other;
            EXPECT(BuildSchedule(pa, &other) == HCCL_SUCCESS && other.ops.size() == scheds[r].ops.size());
            EXPECT(other.ops.empty() ||
                   std::memcmp(other.ops.data(), scheds[r].ops.data(), other.ops.size() * sizeof(HcclAmdIrOp)) == 0);
        }
    }
    // every record lies inside its pair's block, and the bytes of a pair agree on both ends
    std::vector<uint64_t> sent(size_t(n) * n, 0), received(size_t(n) * n, 0);
    for (uint32_t r = 0; r < n; ++r) {
        uint64_t copied = 0;
        for (const HcclAmdIrOp& o : scheds[r].ops) {
            EXPECT(o.kind == HCCL_AMD_IR_COPY || o.kind == HCCL_AMD_IR_SEND || o.kind == HCCL_AMD_IR_RECV);
            EXPECT(o.count != 0);
            if (o.kind == HCCL_AMD_IR_COPY) {
                EXPECT(o.srcBuf[0] == HCCL_AMD_BUF_INPUT && o.dstBuf == HCCL_AMD_BUF_OUTPUT);
                EXPECT(o.srcOff[0] == sd[r][r] && o.dstOff == rd[r][r] && o.count == sc[r][r]);
                copied += o.count;
            } else if (o.kind == HCCL_AMD_IR_SEND) {
                const uint32_t q = static_cast<uint32_t>(o.peer);
                EXPECT(q < n && q != r && o.srcBuf[0] == HCCL_AMD_BUF_INPUT);
                EXPECT(o.srcOff[0] == sd[r][q] + sent[size_t(r) * n + q]);  // pieces in order, no gap
                sent[size_t(r) * n + q] += o.count;
                EXPECT(sent[size_t(r) * n + q] <= sc[r][q]);
            } else {
                const uint32_t q = static_cast<uint32_t>(o.peer);
                EXPECT(q < n && q != r && o.dstBuf == HCCL_AMD_BUF_OUTPUT);
                EXPECT(o.dstOff == rd[r][q] + received[size_t(q) * n + r]);
                received[size_t(q) * n + r] += o.count;
                EXPECT(received[size_t(q) * n + r] <= rc[r][q]);
            }
        }
        EXPECT(copied == sc[r][r]);
    }
    for (uint32_t p = 0; p < n; ++p) {
        for (uint32_t q = 0; q < n; ++q) {
            if (p == q) continue;
            EXPECT(sent[size_t(p) * n + q] == x.at(p, q) && received[size_t(p) * n + q] == x.at(p, q));
        }
    }
}

}  // namespace

int main()
{
    const uint64_t counts[] = {0, 1, 7, 1000, 4099, 70001, (1ull << 20) + 1, 1ull << 30, kSysMaxCount};
    for (uint32_t n = 2; n <= 16; ++n) {
        for (uint64_t es : {1, 2, 4, 8}) {
            for (uint64_t count : counts) {
                for (int agreed = 0; agreed < 2; ++agreed) {
                    for (int smallest = 0; smallest < 2; ++smallest) {
                        CheckPlan(n, es, count, agreed != 0, smallest != 0, false);
                        CheckPlan(n, es, count, agreed != 0, smallest != 0, true);
                    }
                }
            }
        }
    }
    for (uint32_t n = 1; n <= 16; ++n) {
        for (uint64_t es : {1, 2, 4, 8}) {
            for (int shape = 0; shape < 6; ++shape) {
                const Matrix x = MakeMatrix(n, shape);
                // the huge entry is cut into pieces only at a granule that keeps the program small
                for (uint64_t pieceBytes : {uint64_t(0), shape == 5 ? uint64_t(1) << 30 : uint64_t(128)}) {
                    CheckSchedule(x, es, pieceBytes, shape % 3);
                }
            }
        }
    }
    std::printf("cases %ld failures %ld\n", g_cases, g_failures);
    return g_failures == 0 ? 0 : 1;
}
