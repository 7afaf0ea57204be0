"""HcclAmdP2pPlan, the arithmetic both ends of a one-sided point-to-point message share (hccl_amd/csrc/ipc_plan.cc
P2pPlanFor): the windows of all workgroups and pieces cover [0, count) exactly once, the plan depends on nothing but
(count, element size, slot bytes), so both roles compute the same one, and the slots and flag words of distinct pairs
never overlap inside a rank's area, whose size is what HcclAmdCommEnableP2p allocates. CPU only."""
import pytest

import hccl_amd as H

SLOTS = [128, 4096, H.P2P_SLOT_BYTES_DEFAULT]
SLOT_OFF, FILLED, DRAINED = 0, 1, 2


def windows(plan, count):
    """(piece, block, lo, hi) in message coordinates, as k_ipc_p2p derives them."""
    out = []
    for k in range(plan.pieces):
        off = k * plan.slotElems
        ln = min(plan.slotElems, count - off)
        for b in range(plan.blocks):
            lo = min(ln, b * plan.blockElems)
            out.append((k, b, off + lo, off + min(ln, lo + plan.blockElems)))
    return out


@pytest.mark.parametrize("es", [1, 2, 4, 8])
@pytest.mark.parametrize("slot", SLOTS)
def test_windows_cover_the_message_exactly_once(es, slot):
    se = slot // es
    for count in (0, 1, se - 1, se, se + 1, 2 * se + 3):
        plan = H.p2p_plan(count, es, slot, 2)
        assert plan.slotElems == se and plan.blocks == 4 and plan.slots == 2
        assert plan.pieces == -(-count // se)
        assert plan.blockElems % (16 // es) == 0 and plan.blockElems * plan.blocks >= se
        nxt = 0
        for _, _, lo, hi in windows(plan, count):
            assert lo <= hi
            if hi > lo:
                assert lo == nxt  # contiguous in (piece, block) order: no gap, no overlap
                nxt = hi
        assert nxt == count
        # in bytes the pieces and windows do not depend on the element size (a mixed batch runs at its smallest one)
        byte_plan = H.p2p_plan(count * es, 1, slot, 2)
        assert [(k, b, lo * es, hi * es) for k, b, lo, hi in windows(plan, count)] == windows(byte_plan, count * es)


def test_both_roles_compute_the_same_plan():
    """The plan takes no role, rank or peer: there is one function of (count, element size, slot bytes, ranks)."""
    a, b = H.p2p_plan(70001, 4, 4096, 8), H.p2p_plan(70001, 4, 4096, 8)
    fields = [f for f, _ in H.HcclAmdP2pPlanResult._fields_]
    assert [getattr(a, f) for f in fields] == [getattr(b, f) for f in fields]
    assert len(H.SIGNATURES["HcclAmdP2pPlan"][1]) == 5


@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("slot", SLOTS)
def test_slots_and_flag_words_of_distinct_pairs_never_overlap(n, slot):
    plan = H.p2p_plan(0, 1, slot, n)
    spans = []
    for p in range(n):
        for k in range(plan.slots):
            o = H.p2p_offset(SLOT_OFF, slot, n, p, k)
            spans.append((o, o + slot))
            assert o % 16 == 0 and o + slot <= plan.dataBytes
        for b in range(plan.blocks):
            for what in (FILLED, DRAINED):
                o = H.p2p_offset(what, slot, n, p, b)
                spans.append((o, o + 4))
                assert o % 4 == 0 and o >= plan.dataBytes
    spans.sort()
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi <= lo
    assert spans[-1][1] <= plan.areaBytes
    assert plan.dataBytes == n * plan.slots * slot
    assert plan.areaBytes % 4096 == 0 and plan.areaBytes - spans[-1][1] < 4096
    assert plan.counterBytes == 2 * n * plan.blocks * 4


def test_bad_queries_are_refused():
    E = H.HcclResult
    res = H.HcclAmdP2pPlanResult()
    for count, es, slot, n in [(1, 3, 4096, 2), (1, 16, 4096, 2), (1, 4, 64, 2), (1, 4, 4100, 2), (1, 4, 32 << 20, 2),
                               (1, 4, 4096, 0), (1, 4, 4096, 17)]:
        assert H.lib.HcclAmdP2pPlan(count, es, slot, n, res) == E.HCCL_E_PARA, (count, es, slot, n)
