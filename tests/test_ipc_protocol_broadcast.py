"""Model check of the one-sided Broadcast's protocol (hccl_amd/csrc/ipc_k_bcast.hip) among the other kinds.

The random-interleaving model of tests/test_ipc_protocol.py (ranks are streams of launches, a launch is `blocks`
workgroups, one step of one workgroup runs at a time, chosen at random) with the Broadcast's two kinds added:
  * BCAST2 (kIpcBroadcast), root R: phase 0: R stores chunk c into slot 0 and its own chunk into slot 1 of rank c's slot
    area (stgIn); barrier; phase 1: rank r != R reads both slots and stores chunk r into the result area (stgRes) of
    every peer other than R; barrier; phase 2: r reads the other non-root ranks' chunks from its own result area.
  * BCAST1 (kIpcBroadcastOneShot): R stores the piece into every peer's alternate area (parity of the round's barrier
    epoch), where it spans all the slots the other single-barrier kinds use; barrier; the peers read it.
They are mixed in launch sequences with the existing single-barrier (alternate areas) and two-barrier (stgIn, stgRes)
kinds, with the blocks, rounds, pieces and roots varying from launch to launch.

Checked on every element: a read sees exactly the current round's data from the right writer, and no store lands on an
element while a read of it is in progress. The two-barrier kinds share stgIn and stgRes from call to call with no
barrier in between, which holds only while stgIn is read, and stgRes written, between a call's two barriers. The
variant in which the root pushes its own chunk into the peers' result areas in phase 0 breaks that, and must be caught.
"""
import random

import pytest

from test_ipc_protocol import DOUBLE, SINGLE, Violation

BCAST2, BCAST1 = "bcast2", "bcast1"
KINDS = (SINGLE, DOUBLE, BCAST2, BCAST2, BCAST1)


def _launches(rng, n, count, kinds=KINDS):
    return [(rng.choice(kinds), rng.choice((1, 2, 3)), rng.choice((1, 2, 3, 4)), rng.choice((4, 5, 8, 12)),
             rng.randrange(n)) for _ in range(count)]


def _program(n, me, launch, b, epoch0, round0, root_pushes_results):
    """The step list of block b of rank `me` (mirrors k_ipc_collective and k_ipc_bcast)."""
    kind, rounds, blocks, piece, root = launch
    be = -(-piece // blocks)
    lo, hi = min(piece, b * be), min(piece, (b + 1) * be)
    others = [c for c in range(n) if c not in (me, root)]
    steps, e = [], epoch0
    for k in range(rounds):
        g = round0 + k
        if kind in (SINGLE, DOUBLE):
            area = f"alt{(e + 1) & 1}" if kind == SINGLE else "in"
            steps += [("store", c, area, me, lo, hi, (g, me)) for c in range(n) if c != me]
            e += 1
            steps.append(("wait", e))
            steps += [("begin", me, area, q, lo, hi, (g, q)) for q in range(n) if q != me]
            if kind == DOUBLE:
                steps += [("store", p, "res", me, lo, hi, (g, "res", me)) for p in range(n) if p != me]
            steps += [("end", me, area, q, lo, hi) for q in range(n) if q != me]
            if kind == DOUBLE:
                e += 1
                steps.append(("wait", e))
                steps += [("begin", me, "res", c, lo, hi, (g, "res", c)) for c in range(n) if c != me]
                steps += [("end", me, "res", c, lo, hi) for c in range(n) if c != me]
        elif kind == BCAST1:
            area = f"alt{(e + 1) & 1}"
            # the kernel's piece spans the whole alternate area (one slot per area), so it lies over every slot q the
            # other single-barrier kinds use there: modelled as all n slots
            if me == root:
                steps += [("store", c, area, q, lo, hi, (g, "piece")) for c in range(n) if c != me for q in range(n)]
            e += 1
            steps.append(("wait", e))
            if me != root:
                steps += [("begin", me, area, q, lo, hi, (g, "piece")) for q in range(n)]
                steps += [("end", me, area, q, lo, hi) for q in range(n)]
        else:
            if me == root:
                for c in range(n):
                    if c == me:
                        continue
                    steps.append(("store", c, "in", 0, lo, hi, (g, "chunk", c)))
                    if root_pushes_results:
                        steps.append(("store", c, "res", root, lo, hi, (g, "chunk", root)))
                    else:
                        steps.append(("store", c, "in", 1, lo, hi, (g, "chunk", root)))
            e += 1
            steps.append(("wait", e))
            if me != root:
                steps.append(("begin", me, "in", 0, lo, hi, (g, "chunk", me)))
                if not root_pushes_results:
                    steps.append(("begin", me, "in", 1, lo, hi, (g, "chunk", root)))
                steps += [("store", p, "res", me, lo, hi, (g, "chunk", me)) for p in others]
                steps.append(("end", me, "in", 0, lo, hi))
                if not root_pushes_results:
                    steps.append(("end", me, "in", 1, lo, hi))
            e += 1
            steps.append(("wait", e))
            if me != root:
                srcs = others + ([root] if root_pushes_results else [])
                steps += [("begin", me, "res", c, lo, hi, (g, "chunk", c)) for c in srcs]
                steps += [("end", me, "res", c, lo, hi) for c in srcs]
    return steps


def _run(n, launches, seed, root_pushes_results=False, max_steps=400000):
    rng = random.Random(seed)
    cap = 16
    areas = ("in", "res", "alt0", "alt1")
    tag = {(o, a, q, x): None for o in range(n) for a in areas for q in range(n) for x in range(cap)}
    readers = {k: 0 for k in tag}
    flags = {}

    def store(owner, area, slot, lo, hi, val):
        for x in range(lo, hi):
            k = (owner, area, slot, x)
            if readers[k]:
                raise Violation(f"store to {k} during a read")
            tag[k] = val

    def begin_read(owner, area, slot, lo, hi, want):
        for x in range(lo, hi):
            k = (owner, area, slot, x)
            if tag[k] != want:
                raise Violation(f"read of {k} saw {tag[k]}, want {want}")
            readers[k] += 1

    def end_read(owner, area, slot, lo, hi):
        for x in range(lo, hi):
            readers[(owner, area, slot, x)] -= 1

    bases, e, g = [], 0, 0
    for kind, rounds, _blocks, _piece, _root in launches:
        bases.append((e, g))
        e += rounds * (1 if kind in (SINGLE, BCAST1) else 2)
        g += rounds
    cur = [0] * n
    progs, pc = {}, {}

    def start(me):
        lid = cur[me]
        if lid < len(launches):
            for b in range(launches[lid][2]):
                progs[(me, b)] = _program(n, me, launches[lid], b, *bases[lid], root_pushes_results)
                pc[(me, b)] = 0

    def advance(me):
        mine = [k for k in progs if k[0] == me]
        if cur[me] >= len(launches) or not all(pc[k] >= len(progs[k]) for k in mine):
            return False
        for k in mine:
            del progs[k]
            del pc[k]
        cur[me] += 1
        start(me)
        return True

    signalled = set()
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
                if (me, b, ep) not in signalled:
                    signalled.add((me, b, ep))
                    for c in range(n):
                        flags[(c, b, me)] = ep
                    progressed = True
                    break
                if any(flags.get((me, b, c), 0) < ep for c in range(n)):
                    continue
            elif step[0] == "store":
                store(*step[1:])
            elif step[0] == "begin":
                begin_read(*step[1:])
            else:
                end_read(*step[1:])
            pc[(me, b)] += 1
            progressed = True
            break
        if not progressed and not any([advance(me) for me in range(n)]):
            raise Violation("deadlock")
    raise Violation("step limit")


@pytest.mark.parametrize("n", [2, 3, 4])
def test_broadcast_kinds_are_race_free_among_the_others(n):
    for seed in range(60):
        rng = random.Random(5000 * n + seed)
        _run(n, _launches(rng, n, 7), seed)


def test_back_to_back_broadcasts_with_changing_roots():
    """Only Broadcasts, the root moving from call to call: the next root's phase 0 meets the last call's phase 2."""
    for seed in range(60):
        rng = random.Random(seed)
        _run(3, _launches(rng, 3, 8, kinds=(BCAST2, BCAST2, BCAST1)), seed)


def test_root_pushing_results_in_phase_0_is_caught():
    """Negative control: the root storing its own chunk into the peers' result areas before the first barrier lands
    under a peer's phase-2 read of the previous two-barrier call (a Broadcast or an AllReduce)."""
    found = 0
    for seed in range(200):
        rng = random.Random(seed)
        launches = [(DOUBLE, 2, 2, 8, 0), (BCAST2, 2, 2, 8, seed % 3)] + _launches(rng, 3, 3, kinds=(BCAST2, DOUBLE))
        try:
            _run(3, launches, seed, root_pushes_results=True)
        except Violation:
            found += 1
    assert found > 0
