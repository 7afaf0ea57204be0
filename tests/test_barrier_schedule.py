"""HcclBarrier's transport schedules (HcclAmdBuildSchedule with HCCL_AMD_OP_BARRIER; schedule.cc BarrierNhr,
BarrierMesh), host only.

AUTO, NHR and every family but the two meshes give the reference's AicpuBarrierSoleNHR (RunNHRBarrier,
ins_temp_barrier_nhr_aicpu.cc:69-140), restated here as tests/sched_ref.py restates the other templates:
    nSteps = ceil(log2 n); step s: delta = 1 << (nSteps - 1 - s), send to (rank + delta) % n,
    receive from (rank - delta + n) % n.
MESH_ONESHOT / MESH_TWOSHOT give its Mesh1D template (RunBarrierMesh, ins_temp_barrier_mesh_1D.cc:79-111): one group
with a token to and from every peer. Tokens are one INT8 element; count, root and dataType are ignored.

What makes either a barrier is the knowledge-closure property: with known[r] = {r} at the start, and every receive
in group g from p adding what p knew before group g, every rank ends up knowing every rank: no rank's program can
have ended before every rank's has begun."""
import pytest

import hccl_amd as H
from oracle import oracle as O
from test_group_liveness import RECV, SEND, check_live, groups_of

BARRIER = int(H.OpType.BARRIER)
AUTO, MESH1, MESH2, RING, RHD, NHR = (int(H.Algo[k]) for k in
                                      ("AUTO", "MESH_ONESHOT", "MESH_TWOSHOT", "RING", "RHD", "NHR"))
INPUT, OUTPUT = 0, 1
RANKS = list(range(2, 17))


def records(n, algo, count=0, dtype=O.INT8, root=0):
    """Per rank: the program's records, and the algorithm and staging it reports."""
    progs, used = [], set()
    for r in range(n):
        arr, nops, u, scratch = H.build_schedule(BARRIER, algo, n, r, count, dtype, root)
        assert scratch == 0  # the tokens are the program's INPUT and OUTPUT, never the executor staging
        used.add(u)
        progs.append([arr[i] for i in range(nops)])
    assert len(used) == 1
    return progs, used.pop()


def grouped(prog):
    """The records of one rank by transport group, in order; every record of a barrier program is a SEND or RECV."""
    out = []
    for o in prog:
        assert o.kind in (SEND, RECV) and o.count == 1
        if not out or out[-1][0] != o.group:
            out.append((o.group, []))
        out[-1][1].append(o)
    assert [g for g, _ in out] == list(range(len(out)))
    return [ops for _, ops in out]


def nhr_steps(n):
    steps = 0
    while (1 << steps) < n:
        steps += 1
    return steps


def ref_nhr_peers(n, rank):
    """RunNHRBarrier's (sendTo, recvFrom) per step."""
    steps = nhr_steps(n)
    return [((rank + (1 << (steps - 1 - s))) % n, (rank - (1 << (steps - 1 - s)) + n) % n) for s in range(steps)]


def check_pairing(progs):
    """Every SEND has a RECV from the sending rank on the peer, in the group of the same index, with the same count:
    the pairing logic of tests/test_group_liveness.py, whose strict-rendezvous model also says the groups are live."""
    n = len(progs)
    as_groups = []
    for r in range(n):
        arr = progs[r]
        as_groups.append(groups_of(arr, len(arr)))
    for r in range(n):
        for gi, g in enumerate(as_groups[r]):
            for kind, peer, cnt in g:
                other = as_groups[peer][gi]
                want = (RECV if kind == SEND else SEND, r, cnt)
                assert other.count(want) == 1, (r, gi, kind, peer)
    check_live(as_groups)


def check_no_alias(progs):
    """No two records of a group touch the same byte (INT8 tokens: an element is a byte)."""
    for prog in progs:
        for ops in grouped(prog):
            seen = set()
            for o in ops:
                where = (o.srcBuf[0], o.srcOff[0]) if o.kind == SEND else (o.dstBuf, o.dstOff)
                assert where[0] in (INPUT, OUTPUT) and where[1] < 128  # inside a half of the 256 token bytes
                assert (where[0] == INPUT) == (o.kind == SEND)
                assert where not in seen, where
                seen.add(where)


def check_closure(progs):
    """known[r] = {r}; the groups in order; a receive in group g from p adds what p knew before group g."""
    n = len(progs)
    per_rank = [grouped(p) for p in progs]
    known = [{r} for r in range(n)]
    for g in range(max(len(p) for p in per_rank)):
        before = [set(k) for k in known]
        for r in range(n):
            if g < len(per_rank[r]):
                for o in per_rank[r][g]:
                    if o.kind == RECV:
                        known[r] |= before[o.peer]
    for r in range(n):
        assert known[r] == set(range(n)), (r, sorted(set(range(n)) - known[r]))


def check_all(progs):
    check_pairing(progs)
    check_no_alias(progs)
    check_closure(progs)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("algo", [AUTO, NHR])
def test_nhr_barrier(n, algo):
    progs, used = records(n, algo)
    assert used == NHR
    for r in range(n):
        groups = grouped(progs[r])
        assert len(groups) == nhr_steps(n)
        got = []
        for ops in groups:
            assert [o.kind for o in ops] == [SEND, RECV]  # one send and one receive per step
            got.append((ops[0].peer, ops[1].peer))
        assert got == ref_nhr_peers(n, r)
    check_all(progs)


@pytest.mark.parametrize("n", RANKS)
def test_mesh_barrier(n):
    progs, used = records(n, MESH1)
    assert used == MESH1
    for r in range(n):
        groups = grouped(progs[r])
        assert len(groups) == 1
        assert sorted(o.peer for o in groups[0] if o.kind == SEND) == [q for q in range(n) if q != r]
        assert sorted(o.peer for o in groups[0] if o.kind == RECV) == [q for q in range(n) if q != r]
    check_all(progs)


@pytest.mark.parametrize("n", [2, 5, 8, 16])
def test_family_mapping_and_ignored_arguments(n):
    base, _ = records(n, NHR)
    key = lambda progs: [[(o.kind, o.peer, o.group, o.count, o.dstBuf, o.dstOff, o.srcBuf[0], o.srcOff[0])
                          for o in p] for p in progs]
    assert records(n, MESH2)[1] == MESH1  # both mesh families: the Mesh1D template
    for algo in (RING, RHD, int(H.Algo.ORDER_PRESERVED), int(H.Algo.MESH_CHUNK), int(H.Algo.IPC)):
        progs, used = records(n, algo)
        assert used == NHR and key(progs) == key(base)
    # count, root and dataType are ignored: the tokens stay one INT8 element
    progs, used = records(n, NHR, count=12345, dtype=O.FP64, root=n - 1)
    assert used == NHR and key(progs) == key(base)


def test_one_rank_posts_nothing():
    arr, nops, used, scratch = H.build_schedule(BARRIER, AUTO, 1, 0, 0, O.INT8)
    assert nops == 0 and scratch == 0


@pytest.mark.parametrize("n", [5, 8])
def test_the_checker_rejects_a_program_without_its_last_step(n):
    """Mutation: every rank drops the last NHR step. The pairing still holds (the ranks agree), so only the closure
    property can tell: after ceil(log2 n) - 1 steps a rank has heard from at most 2^(steps-1) < n ranks."""
    progs, _ = records(n, NHR)
    last = nhr_steps(n) - 1
    cut = [[o for o in p if o.group != last] for p in progs]
    check_pairing(cut)
    check_no_alias(cut)
    with pytest.raises(AssertionError):
        check_closure(cut)
    check_closure(progs)
