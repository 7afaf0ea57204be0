"""Model check of the one-sided Scatter's and AllGatherV's protocol (hccl_amd/csrc/ipc_k_sg.hip) among the other kinds.

The random-interleaving model of tests/test_ipc_protocol.py: a rank is a stream of launches, a launch is `blocks`
workgroups, one step of one workgroup runs at a time, chosen at random; a launch starts when the rank's previous one
has ended, with no barrier between calls. The launches here mix every kind that shares the staging:
  * SINGLE and DOUBLE as tests/test_ipc_protocol.py models them (k_ipc_collective);
  * the Broadcast's two kinds (ipc_k_bcast.hip): the one-shot, whose root stores into slot 0 of every peer's alternate
    area, and the two-shot through the slot and result areas with two barriers;
  * the all-to-all with the rounds set by the host (ipc_k_a2a.hip): slot `me` of every peer's alternate area;
  * SCATTER: the root stores block c's piece into slot 0 of rank c's alternate area; barrier; rank c reads it. Ranks
    other than the root store nothing and run every barrier;
  * GATHERV: every rank with data left stores its piece into slot `me` of every peer's alternate area; barrier; each
    reads the slots of the ranks whose block reaches into the round. The rounds come from the largest block, so a rank
    with a short or empty block runs barriers in which it moves nothing.
The alternate area of a round is chosen by the parity of its barrier epoch; the epoch bases are equal on every rank.
Checked on every element: a read sees exactly what the matching round's sender stored, and no store lands on an element
while a read of it is in progress. Two seeded mutations must be caught: a single alternate area (no parity), and a
Scatter rank other than the root that skips a round's barrier.
"""
import random

import pytest

from test_ipc_protocol import DOUBLE, SINGLE, Violation

BCAST1, BCAST2, A2A, SCATTER, GATHERV = "bcast_one_shot", "bcast_two_shot", "a2a", "scatter", "gatherv"
KINDS = (SINGLE, DOUBLE, BCAST1, BCAST2, A2A, SCATTER, SCATTER, GATHERV, GATHERV)
TWO_BARRIERS = (DOUBLE, BCAST2)
CAP = 16  # elements per slot in every area


def make_launch(rng, n, kind=None):
    """(kind, rounds, blocks, piece, root, need): need[q] = rounds that rank q's block reaches into (GATHERV)."""
    kind = kind or rng.choice(KINDS)
    rounds = rng.choice((1, 2, 3))
    need = [rng.choice((0, 1, rounds, rounds)) for _ in range(n)]
    need[rng.randrange(n)] = rounds  # the largest block sets the rounds
    return (kind, rounds, rng.choice((1, 2, 3, 4)), rng.choice((4, 5, 8, 12)), rng.randrange(n), need)


def program(n, me, launch, b, epoch0, round0, parity=True, skip_barrier=False):
    """The step list of block b of rank `me` (mirrors the kernels' per-round steps)."""
    kind, rounds, blocks, piece, root, need = launch
    be = -(-piece // blocks)
    lo, hi = min(piece, b * be), min(piece, (b + 1) * be)
    others = [c for c in range(n) if c != me]
    steps, e = [], epoch0

    def reads(area, slots, want):
        return [("begin", me, area, q, lo, hi, want(q)) for q in slots] + [("end", me, area, q, lo, hi) for q in slots]

    for k in range(rounds):
        g = round0 + k
        alt = f"alt{(e + 1) & 1}" if parity else "alt0"
        if kind == SINGLE:
            steps += [("store", c, alt, me, lo, hi, (g, me)) for c in others]
            e += 1
            steps.append(("wait", e))
            steps += reads(alt, others, lambda q: (g, q))
        elif kind == DOUBLE:
            steps += [("store", c, "in", me, lo, hi, (g, me)) for c in others]
            e += 1
            steps.append(("wait", e))
            steps += [("begin", me, "in", q, lo, hi, (g, q)) for q in others]
            steps += [("store", p, "res", me, lo, hi, (g, "res", me)) for p in others]
            steps += [("end", me, "in", q, lo, hi) for q in others]
            e += 1
            steps.append(("wait", e))
            steps += reads("res", others, lambda c: (g, "res", c))
        elif kind == BCAST1:
            if me == root:
                steps += [("store", c, alt, 0, lo, hi, (g, root)) for c in others]
            e += 1
            steps.append(("wait", e))
            if me != root:
                steps += reads(alt, [0], lambda q: (g, root))
        elif kind == BCAST2:
            if me == root:  # chunk c into slot 0 and the root's own chunk into slot 1 of rank c
                for c in others:
                    steps += [("store", c, "in", 0, lo, hi, (g, "chunk", c)), ("store", c, "in", 1, lo, hi, (g, "own"))]
            e += 1
            steps.append(("wait", e))
            if me != root:
                steps += [("begin", me, "in", 0, lo, hi, (g, "chunk", me)), ("begin", me, "in", 1, lo, hi, (g, "own"))]
                steps += [("store", p, "res", me, lo, hi, (g, "res", me)) for p in others if p != root]
                steps += [("end", me, "in", 0, lo, hi), ("end", me, "in", 1, lo, hi)]
            e += 1
            steps.append(("wait", e))
            if me != root:
                steps += reads("res", [c for c in others if c != root], lambda c: (g, "res", c))
        elif kind == A2A:
            steps += [("store", c, alt, me, lo, hi, (g, me, c)) for c in others]
            e += 1
            steps.append(("wait", e))
            steps += reads(alt, others, lambda q: (g, q, me))
        elif kind == SCATTER:
            if me == root:
                steps += [("store", c, alt, 0, lo, hi, (g, "block", c)) for c in others]
            e += 1
            if not (skip_barrier and me != root and k == rounds - 1):
                steps.append(("wait", e))
            if me != root:
                steps += reads(alt, [0], lambda q: (g, "block", me))
        else:  # GATHERV
            if k < need[me]:
                steps += [("store", c, alt, me, lo, hi, (g, me)) for c in others]
            e += 1
            steps.append(("wait", e))
            steps += reads(alt, [q for q in others if k < need[q]], lambda q: (g, q))
    return steps


def run(n, launches, seed, parity=True, skip_barrier=False, max_steps=300000):
    rng = random.Random(seed)
    areas = ("in", "res", "alt0", "alt1")
    tag = {(o, a, q, x): None for o in range(n) for a in areas for q in range(n) for x in range(CAP)}
    readers = {k: 0 for k in tag}
    flags, signalled = {}, set()
    # epoch base and global round id of each launch: equal on every rank (the device epoch word advances by the
    # launch's barriers, which the host sets)
    bases, e, g = [], 0, 0
    for launch in launches:
        bases.append((e, g))
        e += launch[1] * (2 if launch[0] in TWO_BARRIERS else 1)
        g += launch[1]
    cur = [0] * n
    progs, pc = {}, {}

    def start(me):
        lid = cur[me]
        if lid < len(launches):
            for b in range(launches[lid][2]):
                progs[(me, b)] = program(n, me, launches[lid], b, *bases[lid], parity, skip_barrier)
                pc[(me, b)] = 0

    def advance(me):
        mine = [k for k in progs if k[0] == me]
        if cur[me] >= len(launches) or not all(pc[k] >= len(progs[k]) for k in mine):
            return False
        for k in mine:
            del progs[k], pc[k]
        cur[me] += 1
        start(me)
        return True

    for me in range(n):
        start(me)
    for _ in range(max_steps):
        if all(cur[me] >= len(launches) for me in range(n)):
            return
        if any(advance(me) for me in range(n) if rng.random() < 0.3):
            continue
        live = [k for k in progs if pc[k] < len(progs[k])]
        rng.shuffle(live)
        progressed = False
        for me, b in live:
            step = progs[(me, b)][pc[(me, b)]]
            if step[0] == "wait":
                ep = step[1]
                if (me, b, ep) not in signalled:  # the barrier's release store to every rank's flag
                    signalled.add((me, b, ep))
                    for c in range(n):
                        flags[(c, b, me)] = ep
                    progressed = True
                    break
                if any(flags.get((me, b, c), 0) < ep for c in range(n)):
                    continue  # still waiting: try another block
            elif step[0] == "store":
                _, owner, area, slot, lo, hi, val = step
                for x in range(lo, hi):
                    k = (owner, area, slot, x)
                    if readers[k]:
                        raise Violation(f"store to {k} during a read")
                    tag[k] = val
            elif step[0] == "begin":
                _, owner, area, slot, lo, hi, want = step
                for x in range(lo, hi):
                    k = (owner, area, slot, x)
                    if tag[k] != want:
                        raise Violation(f"read of {k} saw {tag[k]}, want {want}")
                    readers[k] += 1
            else:
                _, owner, area, slot, lo, hi = step
                for x in range(lo, hi):
                    readers[(owner, area, slot, x)] -= 1
            pc[(me, b)] += 1
            progressed = True
            break
        if not progressed and not any([advance(me) for me in range(n)]):
            raise Violation("deadlock")
    raise Violation("step limit")


def launches_for(rng, n, count):
    return [make_launch(rng, n) for _ in range(count)]


@pytest.mark.parametrize("n", [2, 3, 4])
def test_mixed_launches_are_race_free(n):
    seen = set()
    for seed in range(80):
        rng = random.Random(5000 * n + seed)
        launches = launches_for(rng, n, 7)
        seen |= {launch[0] for launch in launches}
        run(n, launches, seed)
    assert seen == set(KINDS)  # every kind was among the launches


@pytest.mark.parametrize("kind", [SCATTER, GATHERV])
def test_back_to_back_with_every_other_kind(kind):
    """The new kind before and after each other kind, call after call: the pairs that share the alternate areas and
    the pairs that do not."""
    n = 3
    for other in (SINGLE, DOUBLE, BCAST1, BCAST2, A2A, SCATTER, GATHERV):
        for seed in range(25):
            rng = random.Random(seed)
            launches = [make_launch(rng, n, k) for k in (kind, other, kind, kind, other, kind)]
            run(n, launches, seed)


def test_a_single_alternate_area_is_caught():
    """Mutation: one alternate area, no parity. With one barrier per round the root's next-round store lands on a slot
    that a receiver still copies out; likewise a peer's next AllGatherV piece."""
    for kind in (SCATTER, GATHERV):
        found = 0
        for seed in range(200):
            rng = random.Random(seed)
            n = 3
            launches = [(kind, 3, 2, 8, 1, [3, 3, 3])] + [make_launch(rng, n, kind) for _ in range(3)]
            try:
                run(n, launches, seed, parity=False)
            except Violation:
                found += 1
        assert found > 0, kind


def test_a_scatter_rank_that_skips_a_barrier_is_caught():
    """Mutation: a rank other than the root leaves out the last round's barrier (it has nothing to push). It then reads
    its slot without waiting for the root's store of that round."""
    found = 0
    for seed in range(200):
        rng = random.Random(seed)
        n = 3
        launches = [(SCATTER, 2, 2, 8, 0, [2, 2, 2])] + [make_launch(rng, n) for _ in range(3)]
        try:
            run(n, launches, seed, skip_barrier=True, max_steps=60000)
        except Violation:
            found += 1
    assert found > 0
