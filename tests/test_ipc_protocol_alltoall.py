"""Model check of the one-sided all-to-all's protocol (hccl_amd/csrc/ipc_k_a2a.hip).

The random-interleaving model of tests/test_ipc_protocol.py and tests/test_ipc_protocol_broadcast.py: a rank is a stream
of launches, a launch is `blocks` workgroups, one step of one workgroup runs at a time, chosen at random; a launch starts
when the rank's previous one has ended, with no barrier between calls. What this kind adds, and what is modelled:
  * every pair (p, q) has its own round need (its count over the slot capacity), so the ranks' own needs differ;
  * the slots lie in two alternate areas, chosen by the parity of the round's barrier epoch;
  * in the agreed form (AlltoAllV) block b of rank p stores p's own need into word b of the header of slot p on every
    peer in round 0, and after that round's barrier takes the maximum over the headers of its own area; a rank that has
    finished its own data still runs every remaining barrier; the launch's end advances the rank's epoch counter by the
    agreed count, so the next launch's epochs agree on every rank;
  * launches of the known form (AlltoAll, AlltoAllVC: the host sets the rounds) are mixed in.
Checked on every element: a receiver reads exactly what the sender's matching round stored (launch, round and sender),
every header read is this launch's, and no store lands on an element while a read of it is in progress.
Two seeded mutations must be caught: a rank that leaves after its own rounds (no agreement), and a single slot area
instead of two alternating ones.
"""
import random

import pytest

from test_ipc_protocol import Violation

CAP = 12  # piece coordinates per slot in the model


def make_launch(rng, n, agreed):
    """(agreed, blocks, piece, need[p][q]): need[p][q] = rounds of pair p -> q (0: nothing to send)."""
    need = [[rng.choice((0, 1, 1, 2, 3)) if p != q else 0 for q in range(n)] for p in range(n)]
    if rng.random() < 0.3:
        need[rng.randrange(n)] = [0] * n  # a rank that sends nothing
    return (agreed, rng.choice((1, 2, 3)), rng.choice((4, 5, 8, CAP)), need)


def own_need(need, p):
    return max(1, max(need[p]))  # at least one round always runs


def block_program(n, me, lid, launch, b, epoch0, agree=True, two_areas=True):
    """Generator of the steps of block b of rank `me`; its return value is the rounds it ran (the epoch advance)."""
    agreed, blocks, piece, need = launch
    be = -(-piece // blocks)
    lo, hi = min(piece, b * be), min(piece, (b + 1) * be)
    mine = own_need(need, me)
    rounds = mine if agreed else max(own_need(need, p) for p in range(n))  # known form: the host's ceil(max / cap)
    e, k = epoch0, 0
    while k < rounds:
        area = f"alt{(e + 1) & 1}" if two_areas else "alt0"
        if agreed and k == 0:
            for c in range(n):
                if c != me:
                    yield ("hstore", c, area, me, b, (lid, mine))
        for i in range(n - 1):
            c = (me + 1 + (i + b) % (n - 1)) % n
            if k < need[me][c]:
                yield ("store", c, area, me, lo, hi, (lid, k, me))
        e += 1
        yield ("wait", e)
        if agreed and k == 0 and agree:
            for q in range(n):
                if q != me:
                    got = yield ("hread", me, area, q, b, lid)
                    rounds = max(rounds, got)
        srcs = [q for q in range(n) if q != me and k < need[q][me]]
        for q in srcs:
            yield ("begin", me, area, q, lo, hi, (lid, k, q))
        for q in srcs:
            yield ("end", me, area, q, lo, hi)
        k += 1
    return rounds


def run(n, launches, seed, agree=True, two_areas=True, max_steps=300000):
    rng = random.Random(seed)
    areas = ("alt0", "alt1")
    tag = {(o, a, q, x): None for o in range(n) for a in areas for q in range(n) for x in range(CAP)}
    readers = {k: 0 for k in tag}
    header, flags, signalled = {}, {}, set()
    epoch = [0] * n   # the device epoch word of each rank
    cur = [0] * n     # index of the rank's running launch
    gens, pending, sent, spans = {}, {}, {}, {}

    def start(me):
        if cur[me] < len(launches):
            for b in range(launches[cur[me]][1]):
                g = block_program(n, me, cur[me], launches[cur[me]], b, epoch[me], agree, two_areas)
                gens[(me, b)] = g
                pending[(me, b)] = next(g)
            spans[me] = []

    def step_on(key, value=None):
        try:
            pending[key] = gens[key].send(value)
        except StopIteration as stop:
            pending[key] = None
            spans[key[0]].append(stop.value)

    def advance(me):
        mine = [k for k in gens if k[0] == me]
        if cur[me] >= len(launches) or any(pending[k] is not None for k in mine):
            return False
        if len(set(spans[me])) != 1:
            raise Violation(f"rank {me}: blocks disagree on the rounds {spans[me]}")
        epoch[me] += spans[me][0]  # EndLaunchSpan: the last block to arrive advances the counter
        for k in mine:
            del gens[k], pending[k]
        cur[me] += 1
        start(me)
        return True

    for me in range(n):
        start(me)
    for _ in range(max_steps):
        if all(cur[me] >= len(launches) for me in range(n)):
            if len(set(epoch)) != 1:
                raise Violation(f"epoch counters differ at the end: {epoch}")
            return
        if any(advance(me) for me in range(n) if rng.random() < 0.3):
            continue
        live = [k for k in gens if pending[k] is not None]
        rng.shuffle(live)
        progressed = False
        for key in live:
            me, b = key
            step = pending[key]
            op, value = step[0], None
            if op == "wait":
                ep = step[1]
                if (me, b, ep) not in signalled:
                    signalled.add((me, b, ep))
                    for c in range(n):
                        flags[(c, b, me)] = ep
                    progressed = True
                    break
                if any(flags.get((me, b, c), 0) < ep for c in range(n)):
                    continue
            elif op == "hstore":
                _, owner, area, slot, blk, val = step
                header[(owner, area, slot, blk)] = val
            elif op == "hread":
                _, owner, area, slot, blk, lid = step
                got = header.get((owner, area, slot, blk))
                if got is None or got[0] != lid:
                    raise Violation(f"header {(owner, area, slot, blk)} holds {got}, want launch {lid}")
                value = got[1]
            elif op == "store":
                _, owner, area, slot, lo, hi, val = step
                for x in range(lo, hi):
                    k = (owner, area, slot, x)
                    if readers[k]:
                        raise Violation(f"store to {k} during a read")
                    tag[k] = val
            elif op == "begin":
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
            step_on(key, value)
            progressed = True
            break
        if not progressed and not any([advance(me) for me in range(n)]):
            raise Violation("deadlock")
    raise Violation("step limit")


def launches_for(rng, n, count):
    return [make_launch(rng, n, agreed=rng.random() < 0.7) for _ in range(count)]


@pytest.mark.parametrize("n", [2, 3, 4])
def test_every_receiver_reads_what_the_matching_round_stored(n):
    for seed in range(60):
        rng = random.Random(9000 * n + seed)
        run(n, launches_for(rng, n, 6), seed)


def test_unequal_needs_back_to_back():
    """One rank needs three rounds, the others one or none, call after call with no barrier between the calls."""
    n = 3
    need = [[0, 3, 1], [1, 0, 0], [0, 0, 0]]
    for seed in range(60):
        rng = random.Random(seed)
        launches = [(True, rng.choice((1, 2, 3)), rng.choice((4, 8, CAP)), need) for _ in range(5)]
        run(n, launches, seed)


def test_leaving_after_the_own_rounds_is_caught():
    """Mutation: no agreement. A rank runs only its own rounds' barriers, so the ranks' barrier counts differ: a peer
    waits for a barrier that never comes, or the epoch counters part and a later launch reads another round's data."""
    found = 0
    for seed in range(100):
        rng = random.Random(seed)
        n = 3
        launches = [(True, 2, 8, [[0, 3, 1], [1, 0, 1], [1, 1, 0]])] + launches_for(rng, n, 3)
        try:
            run(n, launches, seed, agree=False, max_steps=60000)
        except Violation:
            found += 1
    assert found == 100


def test_a_single_slot_area_is_caught():
    """Mutation: one slot area instead of two alternating ones. With one barrier per round, a peer's next-round store
    lands on a slot that this rank still copies out."""
    found = 0
    for seed in range(200):
        rng = random.Random(seed)
        n = 3
        launches = [(True, 2, 8, [[0, 3, 3], [3, 0, 3], [3, 3, 0]])] + launches_for(rng, n, 3)
        try:
            run(n, launches, seed, two_areas=False)
        except Violation:
            found += 1
    assert found > 0
