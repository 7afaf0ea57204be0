"""Model check of the one-sided barrier (hccl_amd/csrc/ipc_k_barrier.hip, kind kIpcBarrier) among the other kinds.

The random-interleaving model of tests/test_ipc_protocol.py, with one more launch kind:
  * BARRIER: one workgroup per rank, whatever the neighbouring launches use; it stores epoch E + 1 into workgroup 0's
    flag word of every rank and waits for every rank's; no store to and no read of any staging area. The launch's end
    advances the epoch counter by one.
The launches around it are the SINGLE (one barrier per round, slots in the alternate area of the epoch's parity) and
DOUBLE (two barriers, slot and result areas) kinds of 1-4 workgroups, so the barrier's epoch is one that workgroups
b >= 1 never see, and it flips the parity of the alternate areas between two SINGLE launches.

Checked: the model's element checks (a read sees exactly the current round's data, no store lands on an element that
is being read), and the barrier's own property: no rank's launch after a BARRIER starts before every rank has begun
that BARRIER (its stream has reached it). Two mutations must be caught: a BARRIER whose launch end advances the
epoch counter by 0, and a BARRIER rank that stores its flags but skips its wait.
"""
import random

import pytest

from test_ipc_protocol import DOUBLE, M32, SINGLE, Violation, _launches

BARRIER = "barrier"
CAP = 16  # elements per slot in every area


def mixed_launches(rng, count):
    """SINGLE / DOUBLE launches as tests/test_ipc_protocol.py draws them, with BARRIER launches (one workgroup, one
    round, no data) between them: sometimes two in a row."""
    out = []
    for launch in _launches(rng, count):
        out.append(launch)
        for _ in range(rng.choice((0, 1, 1, 2))):
            out.append((BARRIER, 1, 1, 0))
    return out


def program(n, me, launch, b, epoch0, round0, skip_wait_rank=None):
    """The step list of workgroup b of rank `me` (k_ipc_collective's per-round steps; k_ipc_barrier's one wait)."""
    kind, rounds, blocks, piece = launch
    if kind == BARRIER:
        # Barrier() = the flag stores, then the poll; the mutated rank stores and leaves
        return [("signal", epoch0 + 1)] if me == skip_wait_rank else [("wait", epoch0 + 1)]
    be = -(-piece // blocks)
    lo, hi = min(piece, b * be), min(piece, (b + 1) * be)
    others = [c for c in range(n) if c != me]
    steps, e = [], epoch0
    for k in range(rounds):
        g = round0 + k
        area = f"alt{(e + 1) & 1}" if kind == SINGLE else "in"
        steps += [("store", c, area, me, lo, hi, (g, me)) for c in others]
        e += 1
        steps.append(("wait", e))
        steps += [("begin", me, area, q, lo, hi, (g, q)) for q in others]
        if kind == DOUBLE:
            steps += [("store", p, "res", me, lo, hi, (g, "res", me)) for p in others]
        steps += [("end", me, area, q, lo, hi) for q in others]
        if kind == DOUBLE:
            e += 1
            steps.append(("wait", e))
            steps += [("begin", me, "res", c, lo, hi, (g, "res", c)) for c in others]
            steps += [("end", me, "res", c, lo, hi) for c in others]
    return steps


def run(n, launches, seed, barrier_span=1, skip_wait_rank=None, epoch_base=0, max_steps=300000):
    """barrier_span: what a BARRIER launch's end adds to the epoch counter (the kernel: 1). skip_wait_rank: the rank
    whose BARRIER launches store their flags and do not wait."""
    rng = random.Random(seed)
    areas = ("in", "res", "alt0", "alt1")
    tag = {(o, a, q, x): None for o in range(n) for a in areas for q in range(n) for x in range(CAP)}
    readers = {k: 0 for k in tag}
    flags, signalled = {}, set()

    def behind(flag, ep):  # (int32_t)(flag - ep) < 0, PollFlag's compare
        return (flag - ep) % M32 >= (1 << 31)

    # epoch base and global round id of each launch: equal on every rank (the device epoch word advances by what each
    # launch's end adds)
    bases, e, g = [], 0, 0
    for kind, rounds, blocks, piece in launches:
        bases.append((e, g))
        e += barrier_span if kind == BARRIER else rounds * (1 if kind == SINGLE else 2)
        g += rounds
    cur = [0] * n
    progs, pc = {}, {}

    def start(me):
        lid = cur[me]
        if lid >= len(launches):
            return
        if lid > 0 and launches[lid - 1][0] == BARRIER:
            # the barrier's own property: every rank's stream has reached the barrier this launch follows
            late = [r for r in range(n) if cur[r] < lid - 1]
            if late:
                raise Violation(f"rank {me} starts launch {lid} before ranks {late} have begun barrier {lid - 1}")
        for b in range(launches[lid][2]):
            progs[(me, b)] = program(n, me, launches[lid], b, *bases[lid], skip_wait_rank)
            pc[(me, b)] = 0

    def advance(me):
        """Start rank me's next launch if every workgroup of its current one has finished (stream order)."""
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
            if step[0] in ("wait", "signal"):
                ep = (epoch_base + step[1]) % M32
                if (me, b, cur[me], ep) not in signalled:  # the barrier's release store to every rank's flag
                    signalled.add((me, b, cur[me], ep))
                    for c in range(n):
                        flags[(c, b, me)] = ep
                    progressed = True
                    if step[0] == "signal":
                        pc[(me, b)] += 1
                    break
                if any(behind(flags.get((me, b, c), epoch_base % M32), ep) for c in range(n)):
                    continue  # still waiting: try another workgroup
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


@pytest.mark.parametrize("n", [2, 3, 4])
def test_barriers_between_launches_are_race_free(n):
    barriers = 0
    for seed in range(60):
        rng = random.Random(3000 * n + seed)
        launches = mixed_launches(rng, 6)
        barriers += sum(launch[0] == BARRIER for launch in launches)
        run(n, launches, seed)
    assert barriers > 60


@pytest.mark.parametrize("n", [2, 3])
def test_barriers_across_the_epoch_wrap(n):
    """PollFlag's signed compare keeps a skipped epoch harmless across the wrap at 2^32 too."""
    for seed in range(30):
        rng = random.Random(9000 * n + seed)
        run(n, mixed_launches(rng, 5), seed, epoch_base=M32 - 4)


def test_barrier_between_two_single_barrier_launches_of_many_workgroups():
    """The case the kernel's comment argues: workgroups b >= 1 never see the barrier's epoch, and the barrier flips
    the parity, so the SINGLE launches around it use the same alternate area."""
    for n in (2, 3, 4):
        for seed in range(40):
            run(n, [(SINGLE, 2, 4, 12), (BARRIER, 1, 1, 0), (SINGLE, 3, 4, 12), (BARRIER, 1, 1, 0), (BARRIER, 1, 1, 0),
                    (DOUBLE, 2, 3, 8), (BARRIER, 1, 1, 0), (SINGLE, 1, 2, 5)], seed)


def test_a_barrier_that_does_not_advance_the_epoch_is_caught():
    """Mutation: EndLaunch with epochSpan 0. The next launch reuses the barrier's epoch: workgroup 0's flag words
    already hold it, so its first wait opens at once and its fold reads slots the peers have not filled."""
    found = 0
    for seed in range(200):
        rng = random.Random(seed)
        launches = [(SINGLE, 1, 2, 8), (BARRIER, 1, 1, 0), (SINGLE, 2, 2, 8)] + mixed_launches(rng, 2)
        try:
            run(3, launches, seed, barrier_span=0, max_steps=60000)
        except Violation:
            found += 1
    assert found > 0


def test_a_barrier_rank_that_skips_its_wait_is_caught():
    """Mutation: one rank stores its flags and leaves. Its next launch starts while a peer has not reached the
    barrier: the barrier's own check, which the element checks alone would miss when no data follows."""
    found = 0
    for seed in range(200):
        rng = random.Random(seed)
        launches = [(DOUBLE, 2, 2, 8), (BARRIER, 1, 1, 0), (BARRIER, 1, 1, 0)] + mixed_launches(rng, 2)
        try:
            run(3, launches, seed, skip_wait_rank=1, max_steps=60000)
        except Violation as v:
            found += "have begun barrier" in str(v)
    assert found > 0
