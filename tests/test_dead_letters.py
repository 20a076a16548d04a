"""The dead-letter queue on CPU tensors (``ops/dead_letters.py``): the numpy model
(``DeadLetterRef``) against an independent oracle -- a plain Python loop that files one
letter at a time and keeps the unread tickets in a deque -- over sequences of Sends that
wrap the ring and drain it in between (shared with the GPU tests), the mask, the column
variants, then the runtime's ``dead_letter=`` switch, ``dead_letters()`` and ``redrive()``,
their place among the other wrappers, the public API and the ``gpu.dead_letter*`` config
keys.  All comparisons are exact integer equality."""
from collections import deque

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import dead_letters as DL
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_RETRY_TEST, STATUS_BREAKER_OPEN,
                                   STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NO_METHOD, STATUS_OK, STATUS_THROTTLED)

from test_coalesce import runtime
from test_send_retries import join_world1

U64 = (1 << 64) - 1
STATUSES = (0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 40)


# ---------------------------------------------------------------- the oracle
class Oracle:
    """One letter at a time: every letter is written (a later one over an earlier one),
    the unread tickets are a deque that drops its oldest when it outgrows the ring."""

    def __init__(self, entries, mask):
        self.E, self.mask = entries, mask
        self.ring = [[0] * 8 for _ in range(entries)]
        self.head = self.dropped = self.sends = 0
        self.unread = deque()

    def append(self, batch, status, attempts=None, tag=0):
        self.sends += 1
        for i, s in enumerate(status.tolist()):
            if not (0 <= s < 32 and (self.mask >> s) & 1):
                continue
            m = batch.method if isinstance(batch.method, int) else int(batch.method[i])
            att = 1 if attempts is None else min((int(attempts[i]) & 0xFFFFFFFF) + 1, 65535)
            col = (lambda t: 0 if t is None else int(t[i]) & U64)
            self.ring[self.head % self.E] = [
                self.head + 1, self.sends, i | (s & 0xFFFFFFFF) << 32,
                (int(batch.actor[i]) & 0xFFFFFFFF) | (m & 0xFFFF) << 32 | att << 48,
                col(batch.a0), col(batch.a1), col(batch.a2), tag & U64]
            self.unread.append(self.head)
            self.head += 1
            if len(self.unread) > self.E:
                self.unread.popleft()
                self.dropped += 1

    def take(self, max_letters=None, drain=True):
        n = len(self.unread) if max_letters is None else min(len(self.unread), max_letters)
        t = list(self.unread)[:n]
        if drain:
            for _ in range(n):
                self.unread.popleft()
        return [self.ring[x % self.E] for x in t]

    @property
    def tail(self):
        return self.unread[0] if self.unread else self.head


def random_send(M, seed, k=None, a1=True, a2=True, method="col", attempts=False, statuses=STATUSES):
    """A batch of M rows and its final statuses: random ones from ``statuses``, or -- with
    ``k`` -- exactly ``k`` letters (``STATUS_FAILED``) at random rows among OK ones."""
    g = torch.Generator().manual_seed(seed)
    big = (lambda: torch.randint(-2**62, 2**62, (M,), generator=g))
    if k is None:
        st = torch.tensor(statuses, dtype=torch.int32)[torch.randint(0, len(statuses), (M,), generator=g)]
    else:
        st = torch.zeros(M, dtype=torch.int32)
        st[torch.randperm(M, generator=g)[:k]] = STATUS_FAILED
    m = torch.randint(-2**15, 2**15, (M,), generator=g).to(torch.int16) if method == "col" else method
    b = MsgBatch(torch.randint(-2**31, 2**31, (M,), generator=g).to(torch.int32), big(), big() if a1 else None,
                 big() if a2 else None, m)
    att = torch.randint(0, 70000, (M,), generator=g).to(torch.int32) if attempts else None
    return b, st, att


def same_words(ref, other):
    """``ref`` (the model) against the oracle or a GPU queue, word for word."""
    if isinstance(other, Oracle):
        assert ref.ring.tolist() == other.ring
        assert [int(x) for x in ref.ctrl[:4]] == [other.head, other.tail, other.dropped, other.sends]
        return
    assert np.array_equal(other.ring.cpu().numpy().view(np.uint64), ref.ring)
    assert np.array_equal(other.ctrl.cpu().numpy().view(np.uint64), ref.ctrl)


def ks_of(E):
    return [0, 1, E - 1, E, E + 1, 3 * E, 5, 0, E // 2, E // 2 + 1]


def run_sequence(ref, also, E, to_device=None, seed=0):
    """Sends with K in {0, 1, E - 1, E, E + 1, 3 E, ...} letters each, a drain (peeked
    first, then partial, then whole) after every second one; everything compared after
    every step.  Returns what was reached."""
    dev = to_device or (lambda x: x)
    seen = {"wrapped": 0, "dropped": 0, "over": 0, "drained": 0}
    for n, K in enumerate(ks_of(E)):
        M = max(K, 1) + 37 * (n + 1)
        b, st, att = random_send(M, seed + n, k=K, a1=n % 2 == 0, a2=n % 3 != 0,
                                 method="col" if n % 2 else 7 + n, attempts=n % 3 == 1)
        before = int(ref.ctrl[DL.C_DROPPED])
        ref.append(b, st, att, tag=n * 0x9E3779B97F4A7C15)
        if isinstance(also, Oracle):
            also.append(b, st, att, tag=n * 0x9E3779B97F4A7C15)
        else:
            also.append(dev(b), st.to(also.device), None if att is None else att.to(also.device),
                        tag=n * 0x9E3779B97F4A7C15)
        same_words(ref, also)
        seen["wrapped"] += int(ref.ctrl[DL.C_HEAD]) > E
        seen["dropped"] += int(ref.ctrl[DL.C_DROPPED]) > before
        seen["over"] += K > E
        if n % 2:
            for max_letters, drain in ((None, False), (3, True), (None, True)):
                want = ref.take(max_letters, drain)
                got = also.take(max_letters, drain)
                if isinstance(also, Oracle):
                    assert want["n"] == len(got) and want["torn"] == 0
                    assert want["seq"].tolist() == [r[1] for r in got]
                    assert (want["row"].astype(np.int64) & 0xFFFFFFFF).tolist() == [r[2] & 0xFFFFFFFF for r in got]
                    assert (want["a0"].view(np.uint64)).tolist() == [r[4] for r in got]
                else:
                    assert (got.n, got.ticket, got.torn) == (want["n"], want["ticket"], 0)
                    for c in DL.COLUMNS:
                        assert np.array_equal(getattr(got, c).cpu().numpy(), want[c]), c
                same_words(ref, also)
                seen["drained"] += want["n"] > 0
    return seen


@pytest.mark.parametrize("E", [64, 256])
def test_the_model_against_the_oracle(E):
    ref, orc = DL.DeadLetterRef(E), Oracle(E, DL.DEFAULT_MASK)
    seen = run_sequence(ref, orc, E)
    assert all(v > 0 for v in seen.values()), seen
    assert ref.read() == {"entries": E, "appended": orc.head, "unread": 0, "dropped": orc.dropped,
                          "sends": len(ks_of(E)), "torn": 0}


@pytest.mark.parametrize("M", [0, 1, 63, 65, 4097])
def test_random_statuses_against_the_oracle(M):
    mask = DL.DEFAULT_MASK | 1 << STATUS_THROTTLED
    ref, orc = DL.DeadLetterRef(64, mask), Oracle(64, mask)
    for n in range(3):
        b, st, att = random_send(M, 100 + n, attempts=n == 1)
        ref.append(b, st, att, tag=n)
        orc.append(b, st, att, tag=n)
        same_words(ref, orc)


def test_dropped_and_tail_by_hand():
    ref = DL.DeadLetterRef(64)
    b, st, _ = random_send(200, 1, k=50)
    ref.append(b, st)
    assert ref.read() == {"entries": 64, "appended": 50, "unread": 50, "dropped": 0, "sends": 1, "torn": 0}
    ref.append(b, st)  # 100 letters in a ring of 64: tickets 0 .. 35 are gone
    assert ref.read()["dropped"] == 36 and int(ref.ctrl[DL.C_TAIL]) == 36 and ref.read()["unread"] == 64
    assert ref.take(10)["ticket"] == 36 and int(ref.ctrl[DL.C_TAIL]) == 46
    ref.append(b, st)  # head 150: tail -> 86, tickets 46 .. 85 dropped
    assert ref.read()["dropped"] == 76 and int(ref.ctrl[DL.C_TAIL]) == 86
    got = ref.take()
    assert got["n"] == 64 and got["torn"] == 0 and got["seq"].tolist() == [2] * 14 + [3] * 50
    assert ref.take()["n"] == 0 and ref.read()["unread"] == 0
    # a Send without a letter, and an empty one: counted, the ring untouched
    ring = ref.ring.copy()
    ref.append(*random_send(100, 2, k=0)[:2])
    ref.append(*random_send(0, 3, k=0)[:2])
    assert np.array_equal(ring, ref.ring) and ref.read()["sends"] == 5 and ref.read()["appended"] == 150


def test_more_letters_than_entries_in_one_send():
    E, M = 64, 3 * 64 + 5
    ref = DL.DeadLetterRef(E)
    b, st, _ = random_send(M, 4, k=M)
    ref.append(b, st)
    got = ref.take()
    assert got["n"] == E and got["row"].tolist() == list(range(M - E, M)) and got["torn"] == 0
    assert ref.read()["dropped"] == M - E and ref.read()["appended"] == M
    assert sorted(ref.ring[:, DL.W_TICKET].tolist()) == list(range(M - E + 1, M + 1))  # no slot written twice


# ---------------------------------------------------------------- mask and settings
def test_mask_validation():
    assert DL.dead_letter_mask(None) == DL.DEFAULT_MASK == 0b1111110
    assert DL.dead_letter_mask([STATUS_FAILED, STATUS_BREAKER_OPEN, STATUS_THROTTLED]) == 0b110000100
    assert DL.dead_letter_mask(2) == 2 and DL.dead_letter_mask(2**32 - 2) == 2**32 - 2
    for bad in (0, 1, 3, 2**32, -2, [STATUS_OK], [-1], [40], [2, 32]):
        with pytest.raises(ValueError):
            DL.dead_letter_mask(bad)
    for bad in (0, 32, 63, 65, 96, 2**24 + 1, 2**25):
        with pytest.raises(ValueError):
            DL.DeadLetterRef(bad)
    assert DL.DeadLetterRef(2**6).entries == 64


def test_statuses_outside_the_mask_word_are_never_letters():
    ref = DL.DeadLetterRef(64, 2**32 - 2)  # every nameable status
    st = torch.tensor([-1, 40, 32, -2**31, 2**31 - 1, 0, 31, 1], dtype=torch.int32)
    b = MsgBatch(torch.arange(8, dtype=torch.int32), torch.arange(8), None, None, METHOD_ECHO)
    ref.append(b, st)
    got = ref.take()
    assert got["row"].tolist() == [6, 7] and got["status"].tolist() == [31, 1]


def test_column_variants_and_the_record_by_hand():
    st = torch.tensor([0, 2, 0, 3], dtype=torch.int32)
    actor = torch.tensor([5, -1, 7, 2**31 - 1], dtype=torch.int32)
    a0 = torch.tensor([10, -11, 12, 13])
    ref = DL.DeadLetterRef(64)
    ref.append(MsgBatch(actor, a0, None, None, 0x1ABCD), st, tag=-1)  # (the method is read as u16)
    assert ref.ring[0].tolist() == [1, 1, 1 | 2 << 32, 0xFFFFFFFF | 0xABCD << 32 | 1 << 48, (-11) & U64, 0, 0, U64]
    assert ref.ring[1].tolist() == [2, 1, 3 | 3 << 32, 0x7FFFFFFF | 0xABCD << 32 | 1 << 48, 13, 0, 0, U64]
    col = DL.DeadLetterRef(64)
    col.append(MsgBatch(actor, a0, torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64),
                        torch.full((4,), 0xABCD - 65536, dtype=torch.int16)), st,
               torch.zeros(4, dtype=torch.int32), tag=U64)
    assert np.array_equal(col.ring, ref.ring)  # absent a1 / a2: 0; a uniform method: a column; no attempts: 0 before
    got = ref.take()
    assert got["method"].tolist() == [0xABCD - 65536] * 2 and got["actor"].tolist() == [-1, 2**31 - 1]
    assert got["status"].tolist() == [2, 3] and got["a0"].tolist() == [-11, 13] and got["tag"].tolist() == [-1, -1]


def test_attempts_saturate():
    st = torch.full((5,), STATUS_FAILED, dtype=torch.int32)
    b = MsgBatch(torch.arange(5, dtype=torch.int32), torch.arange(5), None, None, METHOD_ECHO)
    ref = DL.DeadLetterRef(64)
    ref.append(b, st, torch.tensor([0, 65533, 65534, 65535, -1], dtype=torch.int32))
    assert ref.take()["attempts"].tolist() == [1, 65534, 65535, 65535, 65535]


def test_bad_columns_are_refused():
    b = MsgBatch(torch.arange(4, dtype=torch.int32), torch.arange(4), None, None, METHOD_ECHO)
    ref = DL.DeadLetterRef(64)
    with pytest.raises(TypeError):
        ref.append(b, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError):
        ref.append(b, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError):
        ref.append(b, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64))


def test_fnv1a64():
    assert DL.fnv1a64("") == 0xCBF29CE484222325 and DL.fnv1a64("a") == 0xAF63DC4C8601EC8C


# ---------------------------------------------------------------- a runtime (shared with the GPU tests)
def mixed_batch(dev="cpu"):
    """Rows that fail for good (unregistered actors, an unknown method), rows that pass
    at their third and second attempt (``METHOD_RETRY_TEST``: an actor's a0-th call is the
    first to succeed) and rows that pass at once."""
    actor = torch.tensor([0, 1, 900, 3, 4, 5, 901, 7, 8, 9], dtype=torch.int32)
    method = torch.tensor([METHOD_ECHO, METHOD_RETRY_TEST, METHOD_ECHO, 99, METHOD_RETRY_TEST, METHOD_CALC_MULTIPLY,
                           METHOD_CALC_MULTIPLY, METHOD_RETRY_TEST, METHOD_ECHO, METHOD_RETRY_TEST], dtype=torch.int16)
    a0 = torch.tensor([40, 3, 42, 43, 2, 45, 46, 1, 48, 3])
    a1 = torch.tensor([0, 0, 0, 0, 0, -6, 7, 0, 0, 0])
    want = [0, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NO_METHOD, STATUS_FAILED, 0, STATUS_NO_ACTOR, 0, 0, STATUS_FAILED]
    return MsgBatch(actor.to(dev), a0.to(dev), a1.to(dev), None, method.to(dev)), want


def letters_of(rt, **kw):
    got = rt.dead_letters(**kw)
    assert got.torn == 0
    return {c: getattr(got, c).cpu().tolist() for c in DL.COLUMNS}


def dead_letter_scenario(rt, dev="cpu", send=None, redrive=None, tag=0):
    """A Send with every kind of failure, ``dead_letters()``, then redrives until the
    retry-test rows have passed; what fails for good is back with one more attempt each
    time, and a final drain leaves the queue empty."""
    send = send or (lambda b: rt.send("calculator", b, dead_letter=True))
    redrive = redrive or (lambda **kw: rt.redrive("calculator", **kw))
    b, want = mixed_batch(dev)
    val, st = send(b)
    assert st.cpu().tolist() == want and val.cpu().tolist()[5] == -270
    bad = [i for i, s in enumerate(want) if s]
    lt = letters_of(rt)
    assert lt["row"] == bad and lt["status"] == [want[i] for i in bad] and lt["seq"] == [1] * 6
    for c, t in (("actor", b.actor), ("a0", b.a0), ("a1", b.a1), ("method", b.method)):
        assert lt[c] == t.cpu()[bad].tolist(), c
    assert lt["a2"] == [0] * 6 and lt["attempts"] == [1] * 6 and lt["tag"] == [tag - (1 << 64) if tag >> 63 else tag] * 6
    assert letters_of(rt) == lt  # a look takes nothing
    assert letters_of(rt, max_letters=2)["row"] == bad[:2]
    # redrive 1: rows 1, 4, 9 (the letters 0, 3, 5) call again; the a0 = 2 row passes
    r = redrive()
    assert r.n == 6 and r.letters.row.cpu().tolist() == bad
    assert r.status.cpu().tolist() == [STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NO_METHOD, 0, STATUS_NO_ACTOR, STATUS_FAILED]
    assert int(r.value.cpu()[3]) == 2
    lt = letters_of(rt)
    assert lt["actor"] == [1, 900, 3, 901, 9] and lt["attempts"] == [2] * 5 and lt["seq"] == [2] * 5
    assert lt["row"] == [0, 1, 2, 4, 5]  # the row within the redriven batch
    # redrive 2, two letters at a time: the queue keeps its order
    r = redrive(max_letters=2)
    assert r.n == 2 and r.status.cpu().tolist() == [0, STATUS_NO_ACTOR] and int(r.value.cpu()[0]) == 3
    r = redrive()
    assert r.n == 4 and r.status.cpu().tolist() == [STATUS_NO_METHOD, STATUS_NO_ACTOR, 0, STATUS_NO_ACTOR]
    lt = letters_of(rt)
    assert lt["actor"] == [3, 901, 900] and lt["attempts"] == [3, 3, 4] and lt["seq"] == [4, 4, 4]
    d = rt.stats()["dead_letters"]
    assert (d["appended"], d["unread"], d["dropped"], d["sends"], d["redrives"], d["redriven"], d["torn"]) == (
        15, 3, 0, 4, 3, 12, 0)
    assert rt.dead_letters(drain=True).n == 3 and rt.dead_letters().n == 0
    r = redrive()  # nothing to re-send: at world 1 no Send at all
    assert r.n == 0 and r.status.numel() == 0 and rt.stats()["dead_letters"]["sends"] == 4 + (rt.world > 1)
    assert rt.stats()["dead_letters"]["unread"] == 0


def test_runtime_send_dead_letters_and_redrive_cpu():
    rt = runtime(dead_letters=True, dead_letter_entries=64)
    dead_letter_scenario(rt)
    assert rt.stats()["dead_letters"]["entries"] == 64


def redrive_alone_scenario(rt, dev="cpu"):
    b = MsgBatch(torch.arange(8, dtype=torch.int32).to(dev), torch.tensor([1, 2, 3, 4, 1, 2, 3, 4]).to(dev), None, None,
                 METHOD_RETRY_TEST)
    rt.send("calculator", b)  # no argument: the runtime's setting
    assert letters_of(rt)["row"] == [1, 2, 3, 5, 6, 7]
    unread = []
    for _ in range(3):
        rt.redrive("calculator")
        unread.append(rt.stats()["dead_letters"]["unread"])
    assert unread == [4, 2, 0] and rt.state[:8].tolist() == [1, 2, 3, 4, 1, 2, 3, 4]
    rt.send("calculator", b, dead_letter=False)
    assert rt.stats()["dead_letters"]["sends"] == 4


def retries_scenario(rt, dev="cpu"):
    """Only what still failed after the retries is a letter."""
    b = MsgBatch(torch.arange(6, dtype=torch.int32).to(dev), torch.tensor([1, 2, 3, 4, 5, 3]).to(dev), None, None,
                 METHOD_RETRY_TEST)
    val, st = rt.send("calculator", b, retries=2)
    assert st.cpu().tolist() == [0, 0, 0, STATUS_FAILED, STATUS_FAILED, 0]
    lt = letters_of(rt, drain=True)
    assert lt["row"] == [3, 4] and lt["attempts"] == [1, 1] and lt["status"] == [STATUS_FAILED] * 2


def followers_scenario(rt, dev="cpu"):
    """The append runs after coalescing's fan-out: a failed leader's followers each get a letter."""
    actor = torch.tensor([5, 700, 5, 700, 700, 6], dtype=torch.int32)
    b = MsgBatch(actor.to(dev), torch.tensor([2, 3, 2, 3, 3, 2]).to(dev), torch.tensor([4, 5, 4, 5, 5, 4]).to(dev), None,
                 METHOD_CALC_MULTIPLY)
    val, st = rt.send("calculator", b, coalesce=True)
    assert rt.stats()["coalesce"]["executed"] == 3
    assert st.cpu().tolist() == [0, STATUS_NO_ACTOR, 0] + [STATUS_NO_ACTOR] * 2 + [0]
    lt = letters_of(rt, drain=True)
    assert lt["row"] == [1, 3, 4] and lt["actor"] == [700] * 3 and lt["a1"] == [5] * 3


def named_mask(named):
    return DL.DEFAULT_MASK | (1 << STATUS_BREAKER_OPEN | 1 << STATUS_THROTTLED if named else 0)


def breaker_and_limiter_scenario(rt, named, dev="cpu"):
    """``rt``: ``dead_letter_mask=named_mask(named), breaker_threshold=1, limit_burst=2``.  The
    limiter's status 8 and the breaker's status 7 are letters only when the mask names them."""
    b = MsgBatch(torch.tensor([3, 3, 3, 4], dtype=torch.int32).to(dev), torch.tensor([9, 9, 9, 1]).to(dev), None, None,
                 METHOD_RETRY_TEST)
    st = rt.send("calculator", b, limit=True)[1]
    assert st.cpu().tolist() == [STATUS_FAILED, STATUS_FAILED, STATUS_THROTTLED, 0]
    lt = letters_of(rt, drain=True)
    assert lt["row"] == ([0, 1, 2] if named else [0, 1])
    assert lt["status"] == [STATUS_FAILED] * 2 + ([STATUS_THROTTLED] if named else [])
    assert rt.send("calculator", b, breaker=True)[1].cpu().tolist() == [STATUS_FAILED] * 3 + [0]  # trips actor 3
    assert letters_of(rt, drain=True)["row"] == [0, 1, 2]
    assert rt.send("calculator", b, breaker=True)[1].cpu().tolist() == [STATUS_BREAKER_OPEN] * 3 + [0]
    lt = letters_of(rt, drain=True)
    assert lt["row"] == ([0, 1, 2] if named else []) and lt["status"] == ([STATUS_BREAKER_OPEN] * 3 if named else [])
    assert rt.stats()["dead_letters"]["sends"] == 3 and rt.stats()["dead_letters"]["unread"] == 0


def no_queue_scenario(rt, dev="cpu"):
    """``rt`` without the setting: a plain Send creates no queue, asking for one raises."""
    b, _ = mixed_batch(dev)
    rt.send("calculator", b)
    assert rt._dlq is None
    assert rt.stats()["dead_letters"] == {"entries": 0, "appended": 0, "unread": 0, "dropped": 0, "sends": 0,
                                          "torn": 0, "redrives": 0, "redriven": 0}
    for call in (lambda: rt.send("calculator", b, dead_letter=True), rt.dead_letters,
                 lambda: rt.redrive("calculator")):
        with pytest.raises(ValueError, match="dead-letter queue"):
            call()
    rt.send("calculator", b, dead_letter=False)


def test_redrive_alone_empties_the_queue_cpu():
    redrive_alone_scenario(runtime(dead_letters=True))


def test_only_final_failures_are_letters_with_retries_cpu():
    retries_scenario(runtime(dead_letters=True))


def test_followers_of_a_failed_leader_are_letters_cpu():
    followers_scenario(runtime(dead_letters=True))


@pytest.mark.parametrize("named", [False, True])
def test_breaker_and_limiter_answers_are_letters_only_when_named_cpu(named):
    breaker_and_limiter_scenario(runtime(dead_letters=True, dead_letter_mask=named_mask(named), breaker_threshold=1,
                                         limit_burst=2), named)


def test_with_every_other_wrapper_the_ledger_and_a_gather_cpu():
    from ptype_amd.ops.gather import Gather

    rt = runtime(dead_letters=True, ledger=True, breaker_threshold=100, limit_burst=100)
    plain = runtime()
    b, want = mixed_batch()
    g = Gather(torch.zeros(b.M, dtype=torch.int32), 1, "sum")
    val, st = rt.send("calculator", b, coalesce=True, cache=True, breaker=True, limit=True, gather=g)
    pv, ps = plain.send("calculator", b)
    assert torch.equal(st, ps) and st.tolist() == want and torch.equal(val, pv)
    assert letters_of(rt)["row"] == [i for i, s in enumerate(want) if s]
    assert rt.stats()["ledger"]["messages"] == b.M and int(g.n_ok[0]) == want.count(0)


def test_dead_letter_without_a_queue_raises_and_a_plain_send_creates_none_cpu():
    no_queue_scenario(runtime())


def test_a_refused_redrive_leaves_the_queue_as_it_was_cpu():
    """What the Send would refuse is refused before a letter is taken."""
    from ptype_amd.ops.gather import Gather

    rt = runtime(dead_letters=True)
    rt.send("calculator", mixed_batch()[0])
    before = (letters_of(rt), rt.stats()["dead_letters"])
    bad = [({"account": True}, ValueError, "ledger"), ({"no_such_keyword": 1}, TypeError, "no_such_keyword"),
           ({"gather": Gather(torch.zeros(5, dtype=torch.int32), 1, "sum")}, ValueError, None),
           ({"retries": 2, "resend_overflow": False}, ValueError, "resend_overflow"),
           ({"retries": 1, "retry_on": (STATUS_OK,)}, ValueError, "retry_on"), ({"retries": -1}, ValueError, "retries")]
    for kw, err, match in bad:
        with pytest.raises(err, match=match):
            rt.redrive("calculator", **kw)
    with pytest.raises(ValueError, match="hosts"):
        rt.redrive("another-service")
    assert (letters_of(rt), rt.stats()["dead_letters"]) == before
    g = Gather(torch.zeros(6, dtype=torch.int32), 1, "sum")  # the size of what is taken: accepted
    assert rt.redrive("calculator", gather=g).n == 6 and int(g.count[0]) == 6


def test_redrive_keywords_and_capture_cpu():
    rt = runtime(dead_letters=True)
    b, want = mixed_batch()
    rt.send("calculator", b)
    for kw in ({"dead_letter": False}, {"dead_letter_attempts": None}):
        with pytest.raises(ValueError, match="its own"):
            rt.redrive("calculator", **kw)
    rt.exchange._capturing = True  # as inside ActorExchange.capture
    try:
        with pytest.raises(ValueError, match="captur"):
            rt.redrive("calculator")
        rt.send("calculator", b)  # dead-lettering alone reads nothing on the host
    finally:
        rt.exchange._capturing = False
    # (the a0 = 2 row passed at its second call: 6 + 5 letters)
    assert rt.stats()["dead_letters"]["sends"] == 2 and rt.stats()["dead_letters"]["unread"] == 11
    r = rt.redrive("calculator", retries=2, dead_letter_tag=77)  # every keyword of send
    lt = letters_of(rt)
    assert r.n == 11 and lt["tag"] == [77] * 6 and sorted(lt["actor"]) == [3, 3, 900, 900, 901, 901]


def test_bad_runtime_settings_are_refused():
    for kw in ({"dead_letter_entries": 0}, {"dead_letter_entries": 100}, {"dead_letter_entries": 2**25},
               {"dead_letter_mask": 1}, {"dead_letter_mask": 3}, {"dead_letter_mask": 2**32}, {"dead_letter_mask": [0]}):
        with pytest.raises(ValueError):
            runtime(**kw)


# ---------------------------------------------------------------- the public API and the config keys
def test_client_dead_letters_and_redrive_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3, dead_letters=True,
                              dead_letter_entries=128, dead_letter_mask=0b1111110)
    try:
        rt = c.runtime
        assert rt._dlq is not None and (rt._dlq.entries, rt._dlq.mask) == (128, 0b1111110)
        client = c.NewClient("w1", C.ConnConfig())
        dead_letter_scenario(rt, send=lambda b: client.Send(b, dead_letter=True), redrive=client.Redrive,
                             tag=DL.fnv1a64("w1"))
        assert client.DeadLetters().n == 0 and c.Stats()["runtime"]["dead_letters"]["redrives"] == 4
        # an Ask's calls go through Send: its letters carry the client's tag too
        from ptype_amd.ops.scatter import Scatter

        sc = Scatter.members(torch.tensor([0, 2]), torch.tensor([5, 950], dtype=torch.int32), capacity=64)
        ans = client.Ask(MsgBatch(torch.tensor([0], dtype=torch.int32), torch.tensor([7]), None, None, METHOD_ECHO), sc)
        assert ans.st.tolist() == [0, STATUS_NO_ACTOR]
        lt = letters_of(rt, drain=True)
        tag = DL.fnv1a64("w1")
        assert lt["actor"] == [950] and lt["a0"] == [7] and lt["tag"] == [tag - (1 << 64) if tag >> 63 else tag]
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_no_queue_without_the_key_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports)
    try:
        client = c.NewClient("w1", C.ConnConfig())
        client.Send(mixed_batch()[0])
        assert c.runtime._dlq is None and c.Stats()["runtime"]["dead_letters"]["sends"] == 0
        with pytest.raises(ValueError, match="dead-letter queue"):
            client.Send(mixed_batch()[0], dead_letter=True)
        with pytest.raises(ValueError, match="dead-letter queue"):
            client.DeadLetters()
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_dead_letter_keys(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\n"
                 "gpu: {dead_letters: true, dead_letter_entries: 16777216, dead_letter_mask: 4294967294}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.dead_letters is True and (g.dead_letter_entries, g.dead_letter_mask) == (2**24, 2**32 - 2)
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu: {dead_letter_entries: 64, dead_letter_mask: 2}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.dead_letters is False and (g.dead_letter_entries, g.dead_letter_mask) == (64, 2)
    d = C.Config().gpu
    assert d.dead_letters is False and (d.dead_letter_entries, d.dead_letter_mask) == (1 << 16, 0)
    for bad in ("dead_letters: 3", "dead_letter_entries: 0", "dead_letter_entries: 32", "dead_letter_entries: 100",
                "dead_letter_entries: 33554432", "dead_letter_entries: many", "dead_letter_mask: 0",
                "dead_letter_mask: 1", "dead_letter_mask: 3", "dead_letter_mask: -2", "dead_letter_mask: 4294967296",
                "dead_letter_mask: true"):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\ngpu:\n  {bad}\n")
        with pytest.raises(C.ConfigError):
            C.ConfigFromFile(str(p))
