// schedule_digest.cc — a digest of everything BuildSchedule emits, to compare two versions of schedule.cc record by
// record:   g++ -std=c++17 -O2 -I include tools/schedule_digest.cc <path to>/schedule.cc
// One line per case (its parameters and a 64-bit FNV-1a hash over all ranks) and a grand total. Per rank the hash
// folds the return code, algo, scratchElems and, per record, kind, peer, group, count, nsrc, dstBuf, dstOff and the
// first nsrc srcBuf / srcOff entries, each as one 64-bit word (fields, not struct bytes: padding is undefined).
// Grid: opType 0..3 x algo 0..9 x n {1..8, 16} x count {1, 7, 1000, 65537, 2^20+3} x elemSize {1, 2, 4, 8} x
// pieceBytes {0, 128, 4096, 2^20} x cclBytes {200, 1, 3 MiB} x scratchCapBytes {0, 2 x ccl}; refused combinations
// stay (their return code is hashed). Skipped: pieceBytes 128 at the largest count; root n-1 except for Reduce (root
// is read by Reduce only); special = true except for AUTO and IPC (the algorithms resolved through SelectAlgo).
// Added: the multi-ring / multi-instance calls of tests/sanitize/sched_replay_asan.cc and ReduceScatterV layouts.
// --time prints no digest: the wall time of the grid and of 1,000 builds each of three representative calls.
#include <malloc.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "../hccl_amd/csrc/schedule.h"

using hccl_amd::ScheduleParams;

static uint64_t g_total = 1469598103934665603ull, g_cases = 0;
static bool g_print = true;

static void Fold(uint64_t& h, uint64_t v) { h = (h ^ v) * 1099511628211ull; }

static void Case(ScheduleParams p)
{
    uint64_t h = 1469598103934665603ull;
    for (p.rank = 0; p.rank < p.nRanks; ++p.rank) {
        if (!p.counts.empty()) p.count = p.counts[p.rank];
        hccl_amd::Schedule s;
        Fold(h, uint64_t(int64_t(hccl_amd::BuildSchedule(p, &s))));
        Fold(h, uint64_t(int64_t(s.algo)));
        Fold(h, s.scratchElems);
        for (const HcclAmdIrOp& o : s.ops) {
            for (int64_t v : {int64_t(o.kind), int64_t(o.peer), int64_t(o.group), int64_t(o.nsrc), int64_t(o.dstBuf)}) {
                Fold(h, uint64_t(v));
            }
            Fold(h, o.count);
            Fold(h, o.dstOff);
            for (int i = 0; i < o.nsrc; ++i) {
                Fold(h, uint64_t(int64_t(o.srcBuf[i])));
                Fold(h, o.srcOff[i]);
            }
        }
    }
    Fold(g_total, h);
    ++g_cases;
    if (!g_print) return;
    std::printf("op %d algo %d n %u count %llu es %u piece %llu ccl %llu cap %llu root %u special %d v %zu: %016llx\n",
                p.opType, p.algo, p.nRanks, (unsigned long long)(p.counts.empty() ? p.count : 0), p.elemSize,
                (unsigned long long)p.pieceBytes, (unsigned long long)p.cclBytes, (unsigned long long)p.scratchCapBytes,
                p.root, int(p.special), p.counts.size(), (unsigned long long)h);
}

static void Grid()
{
    const uint64_t counts[] = {1, 7, 1000, 65537, (1ull << 20) + 3};
    const uint64_t pieces[] = {0, 128, 4096, 1ull << 20};
    const uint64_t ccls[] = {200ull << 20, 1ull << 20, 3ull << 20};
    ScheduleParams p;
    for (p.opType = 0; p.opType <= 3; ++p.opType)
    for (p.algo = 0; p.algo <= 9; ++p.algo)
    for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 16u})
    for (uint64_t count : counts)
    for (uint32_t es : {1u, 2u, 4u, 8u})
    for (uint64_t piece : pieces)
    for (uint64_t ccl : ccls)
    for (uint64_t cap : {uint64_t(0), 2 * ccl})
    for (uint32_t root = 0; root < n; root += std::max(1u, n - 1))
    for (bool special : {false, true}) {
        if (piece == 128 && count == counts[4]) continue;
        if (root != 0 && p.opType != HCCL_AMD_OP_REDUCE) continue;
        if (special && p.algo != HCCL_AMD_ALGO_AUTO && p.algo != HCCL_AMD_ALGO_IPC) continue;
        p.nRanks = n, p.count = count, p.elemSize = es, p.pieceBytes = piece, p.cclBytes = ccl;
        p.scratchCapBytes = cap, p.root = root, p.special = special;
        Case(p);
    }
    const struct { int op, algo; uint32_t n; uint64_t count; } bigs[] = {
        {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RHD, 8, (2ull << 20) / 8 + 3},
        {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RHD, 8, (49ull << 19) / 8 + 5},
        {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RHD, 4, (16ull << 20) / 8 + 1},
        {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RING, 8, (8ull << 20) / 8 + 7},
        {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RING, 8, (58ull << 20) / 8 + 1},
        {HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_RING, 8, (58ull << 20) / 64 + 3},
        {HCCL_AMD_OP_ALLGATHER, HCCL_AMD_ALGO_RING, 8, (58ull << 20) / 64 + 1},
        {HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RING, 5, (40ull << 20) / 8 + 3},
    };
    for (const auto& b : bigs) {
        ScheduleParams q;
        q.opType = b.op, q.algo = b.algo, q.nRanks = b.n, q.count = b.count, q.elemSize = 8, q.root = b.n / 2;
        q.pieceBytes = 1ull << 20;
        Case(q);
    }
    // ReduceScatterV: equal blocks with gaps, a zero-length block, unequal packed blocks (tests/test_group_liveness.py)
    for (uint32_t n : {1u, 3u, 8u})
    for (int style = 0; style < 3; ++style)
    for (uint64_t piece : {uint64_t(0), uint64_t(16) << 10}) {
        ScheduleParams q;
        q.opType = HCCL_AMD_OP_REDUCE_SCATTER_V, q.nRanks = n, q.pieceBytes = piece;
        q.scratchCapBytes = style == 2 ? 1ull << 20 : 0;
        uint64_t packed = 0;
        for (uint32_t r = 0; r < n; ++r) {
            const uint64_t c = style == 0 ? 7001 : style == 1 ? (r == 1 ? 0 : 4099) : (40961ull * (r + 3)) % 150001 + 1;
            q.counts.push_back(c);
            q.displs.push_back(style == 0 ? r * 9001ull + 3 : style == 1 ? r * 5000ull : packed);
            packed += c;
        }
        Case(q);
    }
}

template <class F>
static double Seconds(F f)
{
    const auto t0 = std::chrono::steady_clock::now();
    f();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv)
{
    // keep the large record vectors on the heap: mapping and unmapping each one costs as much as building it
    mallopt(M_MMAP_THRESHOLD, 1 << 30);
    mallopt(M_TRIM_THRESHOLD, 1 << 30);
    if (argc > 1 && std::strcmp(argv[1], "--time") == 0) {
        g_print = false;
        ScheduleParams p;
        p.nRanks = 8, p.rank = 3, p.count = 64ull << 20, p.elemSize = 4;
        const struct { const char* name; int op, algo; uint64_t ccl; } calls[] = {
            {"allreduce two-shot", HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_MESH_TWOSHOT, 200ull << 20},
            {"allreduce rhd", HCCL_AMD_OP_ALLREDUCE, HCCL_AMD_ALGO_RHD, 200ull << 20},
            {"reducescatter nhr ccl 1 MiB", HCCL_AMD_OP_REDUCE_SCATTER, HCCL_AMD_ALGO_NHR, 1ull << 20},
        };
        for (const auto& c : calls) {
            p.opType = c.op, p.algo = c.algo, p.cclBytes = c.ccl;
            size_t ops = 0;
            const double s = Seconds([&] {
                for (int i = 0; i < 1000; ++i) {
                    hccl_amd::Schedule sch;
                    hccl_amd::BuildSchedule(p, &sch);
                    ops += sch.ops.size();
                }
            });
            std::printf("%s: 1000 builds %.6f s (%zu records each)\n", c.name, s, ops / 1000);
        }
        std::fflush(stdout);
        std::printf("grid %.3f s\n", Seconds(Grid));
        return 0;
    }
    Grid();
    std::printf("cases %llu total %016llx\n", (unsigned long long)g_cases, (unsigned long long)g_total);
    return 0;
}
