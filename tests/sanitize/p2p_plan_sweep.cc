// Host-code sanitizer run (ASan + UBSan) of the point-to-point planner and HcclBatchSendRecv's list handling
// (hccl_amd/csrc/ipc_plan.cc P2pPlanFor, BatchSendRecvOrder): a stand-alone program that sweeps both and checks the
// invariants the kernel and the entry point rely on. Built and run by tests/test_sanitize_p2p.py with the host
// compiler; no GPU, no HIP.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../hccl_amd/csrc/ipc_plan.h"

using namespace hccl_amd;

static int failures = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

static void SweepPlans()
{
    const uint64_t slots[] = {128, 256, 4096, 65536, kP2pSlotBytesDefault, kP2pSlotBytesMax};
    for (uint64_t slot : slots) {
        for (uint64_t es : {1, 2, 4, 8}) {
            const uint64_t se = slot / es;
            for (uint64_t count : {uint64_t(0), uint64_t(1), se - 1, se, se + 1, 2 * se + 3, 5 * se, uint64_t(0x7FFFFFFFF)}) {
                for (uint32_t n : {1u, 2u, 3u, 8u, 16u}) {
                    P2pPlan p{};
                    EXPECT(P2pPlanFor(count, es, slot, n, &p) == HCCL_SUCCESS);
                    EXPECT(p.slotElems == se && p.blocks == kP2pBlocks && p.slots == kP2pSlots);
                    EXPECT(p.pieces * se >= count && (p.pieces == 0 || (p.pieces - 1) * se < count));
                    EXPECT(p.blockElems * kP2pBlocks >= se && p.blockElems * es % 16 == 0);
                    if (p.pieces > 64) continue;  // the windows of a short message, one by one
                    uint64_t next = 0;
                    for (uint64_t k = 0; k < p.pieces; ++k) {
                        const uint64_t off = k * se, len = se < count - off ? se : count - off;
                        for (uint32_t b = 0; b < p.blocks; ++b) {
                            const uint64_t lo = len < b * p.blockElems ? len : b * p.blockElems;
                            const uint64_t hi = len < lo + p.blockElems ? len : lo + p.blockElems;
                            if (hi > lo) {
                                EXPECT(off + lo == next);
                                next = off + hi;
                            }
                        }
                    }
                    EXPECT(next == count);
                    // the layout: slots, then filled, then drained, all inside the area
                    EXPECT(P2pSlotOffset(slot, n - 1, kP2pSlots - 1) + slot == p.dataBytes);
                    EXPECT(P2pFilledOffset(slot, n, 0, 0) == p.dataBytes);
                    EXPECT(P2pDrainedOffset(slot, n, 0, 0) == P2pFilledOffset(slot, n, n - 1, kP2pBlocks - 1) + 4);
                    EXPECT(P2pDrainedOffset(slot, n, n - 1, kP2pBlocks - 1) + 4 <= p.areaBytes);
                }
            }
        }
    }
    P2pPlan p{};
    EXPECT(P2pPlanFor(1, 3, 4096, 2, &p) == HCCL_E_PARA);
    EXPECT(P2pPlanFor(1, 4, 64, 2, &p) == HCCL_E_PARA);
    EXPECT(P2pPlanFor(1, 4, 4096, 17, &p) == HCCL_E_PARA);
    EXPECT(P2pPlanFor(1, 4, 4096, 2, nullptr) == HCCL_E_PTR);
}

static void SweepOrders()
{
    std::mt19937 rng(12345);
    char byte = 0;
    for (int iter = 0; iter < 20000; ++iter) {
        const uint32_t n = 1 + rng() % 16, me = rng() % n, num = rng() % 12;
        std::vector<HcclSendRecvItem> items(num);
        for (HcclSendRecvItem& it : items) {
            it.sendRecvType = static_cast<HcclSendRecvType>(rng() % 8 == 0 ? 2 : rng() % 2);
            it.count = rng() % 4;
            it.buf = rng() % 16 == 0 ? nullptr : &byte;
            it.dataType = static_cast<HcclDataType>(rng() % 6);
            it.remoteRank = rng() % n;
        }
        std::vector<uint32_t> order(num + 1, 0xFFFFFFFFu);
        uint32_t s = 0, r = 0, pr = 0;
        const HcclResult res = BatchSendRecvOrder(items.data(), num, me, n, order.data(), &s, &r, &pr);
        EXPECT(res == HCCL_SUCCESS || res == HCCL_E_PARA || res == HCCL_E_PTR);
        EXPECT(order[num] == 0xFFFFFFFFu);  // never written past itemNum entries
        if (res != HCCL_SUCCESS) continue;
        EXPECT(s + r + 2 * pr <= num);
        std::vector<int> seen(num, 0);
        for (uint32_t k = 0; k < s + r + 2 * pr; ++k) {
            EXPECT(order[k] < num);
            if (order[k] >= num) continue;
            const HcclSendRecvItem& it = items[order[k]];
            EXPECT(++seen[order[k]] == 1 && it.count > 0 && it.buf != nullptr);
            const bool self = k >= s + r, send = self ? (k - s - r) % 2 == 0 : k < s;
            EXPECT((it.remoteRank == me) == self && (it.sendRecvType == HCCL_SEND) == send);
        }
        for (uint32_t i = 0; i < num; ++i) EXPECT(seen[i] == (items[i].count > 0 ? 1 : 0));
        for (uint32_t k = 0; k < pr; ++k) {
            EXPECT(items[order[s + r + 2 * k]].count == items[order[s + r + 2 * k + 1]].count);
        }
        // duplicates of a pair: count, then data type, descending
        for (uint32_t k = 1; k < s + r; ++k) {
            if (k == s) continue;
            const HcclSendRecvItem &a = items[order[k - 1]], &b = items[order[k]];
            if (a.remoteRank != b.remoteRank) continue;
            EXPECT(a.count > b.count || (a.count == b.count && a.dataType >= b.dataType));
        }
    }
    uint32_t x = 0;
    EXPECT(BatchSendRecvOrder(nullptr, 0, 0, 1, &x, &x, &x, &x) == HCCL_E_PTR);
}

int main()
{
    SweepPlans();
    SweepOrders();
    std::printf("failures %d\n", failures);
    return failures == 0 ? 0 : 1;
}
