"""Model check of the cross-rank argument check (hccl_amd/csrc/ipc_k_check.hip) among the other launch kinds.

The random-interleaving model of tests/test_ipc_protocol_barrier.py, with one more launch kind:
  * CHECK: one workgroup per rank. Lane t of rank `me` stores the words of its record into slot [parity][me] of rank
    t's check area, each word together with the check's sequence number s (one 8-byte store in the kernel: data and
    number become visible together), then polls slot [parity][t] of its own area until every word carries s, and
    compares. s is the rank's private counter + 1, parity is s & 1, and the launch's end stores s into the counter.
    The lanes of a wave are modelled as independent threads: their stores become visible in any order.
A CHECK reads and writes only the check areas and the counter: the epoch counter, the flag words and the staging
areas of the other kinds are other dictionaries here, as they are other allocations in the library, and the epoch
bases of the launches around a CHECK are computed as if it were not there.

Checked, beside the element checks of the SINGLE / DOUBLE / BARRIER launches that run in between:
  * a reader only ever compares a complete record of the current check (every word it accepts was stored by the peer's
    launch of the same check);
  * equal records never fail;
  * a differing record fails on every rank that has a peer differing from it, and on no other;
  * the launches of the other kinds see what they see without the CHECKs (their checks pass unchanged).
Two mutations must be caught: one parity instead of two, and a sequence counter that does not advance.
"""
import random

import pytest

from test_ipc_protocol import DOUBLE, M32, SINGLE, Violation
from test_ipc_protocol_barrier import BARRIER, CAP, mixed_launches, program

CHECK = "check"
WORDS = 11  # HCCL_AMD_CHECK_WORDS


def with_checks(rng, count):
    """SINGLE / DOUBLE / BARRIER launches as the barrier's model draws them, with CHECK launches in between: often
    several in a row, which is where a rank runs ahead of a peer that is still reading."""
    out = []
    for launch in mixed_launches(rng, count):
        for _ in range(rng.choice((0, 1, 2, 3))):
            out.append((CHECK, 1, 1, 0))
        out.append(launch)
    out.append((CHECK, 1, 1, 0))
    return out


def run(n, launches, seed, records=None, parities=2, seq_step=1, seq_base=0, max_steps=400000):
    """records: {launch index: [record of rank 0, ...]} (a record is a tuple of WORDS values) for the CHECK launches
    whose ranks do not all pass the same record (0, ..., 0). parities and seq_step are the mutations' knobs (the kernel:
    2 and 1). Returns {launch index: [failed on rank 0, ...]} for the CHECK launches."""
    rng = random.Random(seed)
    records = records or {}
    areas = ("in", "res", "alt0", "alt1")
    tag = {(o, a, q, x): None for o in range(n) for a in areas for q in range(n) for x in range(CAP)}
    readers = {k: 0 for k in tag}
    flags, signalled = {}, set()
    check_area = {}  # (owner, parity, src, word) -> (sequence number, value, launch index of the store)
    seq = [seq_base % M32] * n  # the private counter word of every rank
    failed = {}

    def behind(flag, ep):
        return (flag - ep) % M32 >= (1 << 31)

    def record(lid, r):
        return records.get(lid, [(0,) * WORDS] * n)[r]

    # a CHECK adds nothing to the epoch counter and is no round: the other kinds' bases do not see it
    bases, e, g = [], 0, 0
    for kind, rounds, blocks, piece in launches:
        bases.append((e, g))
        if kind == CHECK:
            continue
        e += 1 if kind == BARRIER else rounds * (1 if kind == SINGLE else 2)
        g += rounds
    cur = [0] * n
    progs, pc = {}, {}
    mine_seq = {}  # rank -> the number its running CHECK launch uses

    def start(me):
        lid = cur[me]
        if lid >= len(launches):
            return
        if launches[lid][0] == CHECK:
            s = (seq[me] + 1) % M32
            mine_seq[me] = s
            failed.setdefault(lid, [False] * n)
            for t in range(n):
                if t == me:
                    continue
                steps = [("csend", t, w) for w in range(WORDS)]
                rng.shuffle(steps)  # the stores of a lane land in any order
                progs[(me, t)] = steps + [("cpoll", t)]
                pc[(me, t)] = 0
            return
        for b in range(launches[lid][2]):
            progs[(me, b)] = program(n, me, launches[lid], b, *bases[lid])
            pc[(me, b)] = 0

    def advance(me):
        mine = [k for k in progs if k[0] == me]
        if cur[me] >= len(launches) or not all(pc[k] >= len(progs[k]) for k in mine):
            return False
        for k in mine:
            del progs[k], pc[k]
        if launches[cur[me]][0] == CHECK:
            seq[me] = (seq[me] + seq_step) % M32  # the launch's end stores s (the mutation: leaves the counter)
        cur[me] += 1
        start(me)
        return True

    for me in range(n):
        start(me)
    for _ in range(max_steps):
        if all(cur[me] >= len(launches) for me in range(n)):
            return failed
        if any(advance(me) for me in range(n) if rng.random() < 0.3):
            continue
        live = [k for k in progs if pc[k] < len(progs[k])]
        rng.shuffle(live)
        progressed = False
        for me, b in live:
            step = progs[(me, b)][pc[(me, b)]]
            lid = cur[me]
            if step[0] == "csend":
                _, t, w = step
                s = mine_seq[me]
                check_area[(t, s % parities, me, w)] = (s, record(lid, me)[w], lid)
            elif step[0] == "cpoll":
                _, t = step
                s = mine_seq[me]
                got = [check_area.get((me, s % parities, t, w), (None, None, None)) for w in range(WORDS)]
                if any(x[0] != s for x in got):
                    continue  # still waiting for a word of this check
                stale = [w for w, x in enumerate(got) if x[2] != lid]
                if stale:
                    raise Violation(f"rank {me} check {lid}: words {stale} of rank {t} are those of launch "
                                    f"{got[stale[0]][2]}")
                if tuple(x[1] for x in got) != record(lid, me):
                    failed[lid][me] = True
            elif step[0] in ("wait", "signal"):
                ep = step[1] % M32
                if (me, b, lid, ep) not in signalled:
                    signalled.add((me, b, lid, ep))
                    for c in range(n):
                        flags[(c, b, me)] = ep
                    progressed = True
                    break
                if any(behind(flags.get((me, b, c), 0), ep) for c in range(n)):
                    continue
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
def test_equal_records_never_fail_among_the_other_kinds(n):
    checks = 0
    for seed in range(40):
        rng = random.Random(5000 * n + seed)
        launches = with_checks(rng, 5)
        failed = run(n, launches, seed)
        checks += len(failed)
        assert len(failed) == sum(launch[0] == CHECK for launch in launches)
        assert not any(any(f) for f in failed.values())
    assert checks > 80


@pytest.mark.parametrize("n", [2, 3])
def test_the_sequence_number_wraps(n):
    for seed in range(20):
        rng = random.Random(7000 * n + seed)
        failed = run(n, with_checks(rng, 4), seed, seq_base=M32 - 3)
        assert not any(any(f) for f in failed.values())


@pytest.mark.parametrize("n", [2, 3, 4])
def test_a_differing_record_fails_on_every_rank_that_sees_a_difference(n):
    for seed in range(40):
        rng = random.Random(11000 * n + seed)
        launches = with_checks(rng, 3)
        last = len(launches) - 1
        odd, word = rng.randrange(n), rng.randrange(WORDS)
        recs = [tuple(7 if (r == odd and w == word) else 0 for w in range(WORDS)) for r in range(n)]
        failed = run(n, launches, seed, records={last: recs})
        # with one rank apart, every rank has a peer that differs from it
        assert failed[last] == [True] * n
        assert not any(any(f) for lid, f in failed.items() if lid != last)


def test_only_the_ranks_with_a_differing_peer_fail():
    """Two ranks with equal records and nobody else: a world of 2 never fails; in a world of 4 with two pairs, all do."""
    for seed in range(20):
        launches = [(CHECK, 1, 1, 0), (SINGLE, 2, 2, 8), (CHECK, 1, 1, 0)]
        a, b = (1,) * WORDS, (2,) * WORDS
        assert run(2, launches, seed, records={2: [a, a]})[2] == [False, False]
        assert run(4, launches, seed, records={2: [a, a, b, b]})[2] == [True] * 4


def test_one_parity_is_caught():
    """Mutation: every check uses the same slots. A rank one check ahead overwrites words a peer is still polling for:
    the peer never completes its record (or completes it from two checks)."""
    found = 0
    for seed in range(200):
        launches = [(CHECK, 1, 1, 0)] * 4 + [(SINGLE, 1, 2, 8), (CHECK, 1, 1, 0), (CHECK, 1, 1, 0)]
        try:
            run(3, launches, seed, parities=1, max_steps=60000)
        except Violation:
            found += 1
    assert found > 0


def test_a_sequence_counter_that_does_not_advance_is_caught():
    """Mutation: the launch's end leaves the counter. The next check uses the same number and parity, so the words of
    the check before pass for fresh ones."""
    found = 0
    for seed in range(200):
        launches = [(CHECK, 1, 1, 0), (DOUBLE, 1, 2, 8), (CHECK, 1, 1, 0), (BARRIER, 1, 1, 0), (CHECK, 1, 1, 0)]
        try:
            run(3, launches, seed, seq_step=0, max_steps=60000)
        except Violation as v:
            found += "are those of launch" in str(v)
    assert found > 0
