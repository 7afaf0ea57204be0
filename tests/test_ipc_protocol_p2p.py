"""Model check of the point-to-point credit protocol (hccl_amd/csrc/ipc_k_p2p.hip), in the manner of
tests/test_ipc_protocol_scatter_gatherv.py, but exhaustive: every interleaving of the workgroups is explored (a
breadth-first search over the reachable states), one step of one workgroup at a time.

One ordered pair and one workgroup index b: a sender block and a receiver block, two data slots, the words `filled`
(stored by the sender into the receiver) and `drained` (stored by the receiver into the sender), piece numbers that run
on across messages from a base that both private counters hold. Per piece s the sender waits drained >= s - 2, stores
its window into slot s % 2 (a store takes two steps, begin and end, so that a read in between is seen), then stores
filled = s; the receiver waits filled >= s, reads slot s % 2 (begin, end), then stores drained = s. All compares are
32-bit serial-number compares. Checked in every reachable state: no slot is written while a read of it is in progress or
before its last content was read, every read sees exactly the piece it waited for, and no state has every unfinished
block waiting. A peer that never arrives leads to the give-up state, after which the block stores nothing. Two seeded
mutations must be caught: a sender that takes one credit too many, and a receiver that does not wait.
"""
from collections import deque

import pytest

SLOTS = 2
M32 = 1 << 32


def reached(flag, want):
    """int32_t(flag - want) >= 0"""
    return ((flag - want) % M32) < (1 << 31)


class Violation(Exception):
    pass


def sender_program(base, pieces, credit=SLOTS):
    steps, s = [], base
    for _ in range(pieces):
        s = (s + 1) % M32
        steps += [("wait_drained", (s - credit) % M32), ("store_begin", s), ("store_end", s), ("set_filled", s)]
    return steps


def receiver_program(base, pieces, wait=True):
    steps, s = [], base
    for _ in range(pieces):
        s = (s + 1) % M32
        steps += ([("wait_filled", s)] if wait else []) + [("read_begin", s), ("read_end", s), ("set_drained", s)]
    return steps


def explore(pairs, absent=()):
    """pairs: list of (sender steps, receiver steps), each pair with its own slots and flag words (the lanes of distinct
    pairs share nothing). absent: indices of actors (2 * pair + role) that never run; a block that waits for one gives
    up. Returns (states, finished, gave_up): whether a state with every present actor done was reached, and the set of
    actors that gave up somewhere."""
    n = len(pairs)
    progs = [p for pair in pairs for p in pair]
    # per pair: filled, drained, slot contents (piece number or None), slot state ("idle" / "writing" / "reading"),
    # slot unread (content stored and not yet read)
    mem0 = tuple((pairs_base(pairs[i]), pairs_base(pairs[i]), (None,) * SLOTS, ("idle",) * SLOTS, (False,) * SLOTS)
                 for i in range(n))
    start = (tuple(0 for _ in progs), mem0, frozenset())
    seen, todo = {start}, deque([start])
    finished, gave_up_any = False, set()
    while todo:
        pcs, mem, gave = todo.popleft()
        live = [a for a in range(len(progs)) if a not in absent and a not in gave and pcs[a] < len(progs[a])]
        if not live:
            finished = finished or not gave
            continue
        moved = False
        for a in live:
            op, s = progs[a][pcs[a]]
            i = a // 2
            filled, drained, content, state, unread = mem[i]
            content, state, unread = list(content), list(state), list(unread)
            k = s % SLOTS
            nxt_gave = gave
            if op == "wait_drained":
                if not reached(drained, s):
                    if a + 1 in absent:  # its receiver never comes: the bounded wait ends, nothing more is stored
                        nxt_gave = gave | {a}
                        gave_up_any.add(a)
                    else:
                        continue
            elif op == "wait_filled":
                if not reached(filled, s):
                    if a - 1 in absent:
                        nxt_gave = gave | {a}
                        gave_up_any.add(a)
                    else:
                        continue
            elif op == "store_begin":
                if state[k] != "idle":
                    raise Violation(f"piece {s}: slot {k} written while {state[k]}")
                if unread[k]:
                    raise Violation(f"piece {s}: slot {k} overwritten before piece {content[k]} was read")
                state[k] = "writing"
            elif op == "store_end":
                state[k], content[k], unread[k] = "idle", s, True
            elif op == "set_filled":
                filled = s
            elif op == "read_begin":
                if state[k] != "idle":
                    raise Violation(f"piece {s}: slot {k} read while {state[k]}")
                if content[k] != s:
                    raise Violation(f"piece {s}: read before its fill (slot {k} holds {content[k]})")
                state[k] = "reading"
            elif op == "read_end":
                state[k], unread[k] = "idle", False
            elif op == "set_drained":
                drained = s
            moved = True
            new_mem = mem[:i] + ((filled, drained, tuple(content), tuple(state), tuple(unread)),) + mem[i + 1:]
            new_pcs = pcs[:a] + (pcs[a] + (0 if nxt_gave is not gave else 1),) + pcs[a + 1:]
            st = (new_pcs, new_mem, nxt_gave)
            if st not in seen:
                seen.add(st)
                todo.append(st)
        if not moved:
            raise Violation(f"every unfinished block waits: pcs {pcs}")
    return len(seen), finished, gave_up_any


def pairs_base(pair):
    """The flag words' value before the pair's first piece: the piece number before the sender's first."""
    return (pair[0][1][1] - 1) % M32 if pair[0] else 0


def pair(base, pieces, **kw):
    credit, wait = kw.get("credit", SLOTS), kw.get("wait", True)
    return (sender_program(base, pieces, credit), receiver_program(base, pieces, wait))


@pytest.mark.parametrize("base", [0, 7, M32 - 2, M32 - 1])
@pytest.mark.parametrize("pieces", [1, 2, 3, 4, 5])
def test_one_message_every_interleaving(base, pieces):
    states, finished, gave = explore([pair(base, pieces)])
    assert finished and not gave and states > pieces * 8


@pytest.mark.parametrize("base", [0, M32 - 3])
@pytest.mark.parametrize("first,second", [(1, 1), (1, 4), (3, 2), (5, 1), (2, 5)])
def test_two_messages_back_to_back(base, first, second):
    """The second message's pieces follow on the first's: one program per block, as two launches on a stream (or two
    items of a lane) run."""
    _, finished, gave = explore([pair(base, first + second)])
    assert finished and not gave


@pytest.mark.parametrize("a,b", [(1, 1), (2, 3), (3, 3), (4, 1)])
def test_both_directions_at_once(a, b):
    """A batch on both ranks: each rank's launch holds a sending lane and a receiving lane, four blocks in all, with
    the counters of one pair just below 2^32."""
    _, finished, gave = explore([pair(5, a), pair(M32 - 2, b)])
    assert finished and not gave


@pytest.mark.parametrize("pieces", [1, 2])
def test_a_short_message_completes_on_the_sender_alone(pieces):
    """At most two pieces: the sender needs no credit, so it finishes though the receiver never starts."""
    _, finished, gave = explore([pair(M32 - 1, pieces)], absent={1})
    assert finished and not gave


@pytest.mark.parametrize("pieces", [3, 5])
def test_a_lost_receiver_ends_in_the_give_up_state_with_no_further_store(pieces):
    sender, receiver = pair(0, pieces)
    _, finished, gave = explore([(sender, receiver)], absent={1})
    assert gave == {0} and not finished
    # the give-up is taken at a wait, and the block's program is abandoned there: what would have followed is exactly
    # the stores of piece 3 onwards, none of which any explored state has executed
    assert sender[8][0] == "wait_drained" and all(op != "wait_filled" for op, _ in sender)


def test_a_lost_sender_ends_in_the_give_up_state():
    _, finished, gave = explore([pair(0, 2)], absent={0})
    assert gave == {1} and not finished


def test_one_credit_too_many_is_caught():
    with pytest.raises(Violation, match="overwritten before|written while"):
        explore([pair(0, 4, credit=SLOTS + 1)])


def test_a_receiver_that_does_not_wait_is_caught():
    with pytest.raises(Violation, match="read before its fill|read while"):
        explore([pair(0, 2, wait=False)])
