"""The Forward / device-outbox contract, written once: plain Python ints and numpy.

Every implementation of a handler that sends -- the HIP dispatchers that compile
``run_handler`` with an outbox (csrc/hip/handlers.hpp) and the CPU reference
(``ops.batch._handler_ref`` + ``DeviceOutbox.emit_cpu``) -- is tested against this
file; it imports nothing from ``ptype_amd.ops.batch``.

A ``Forward`` row (actor, a0 = next hop, a1 = hops left, a2 = stride | n << 32) that
reaches mailbox ``mb < n_state`` counts one visit (reply: the count it made).  While
``a1 > 0`` it sends: with an outbox bound it appends the record

    (actor_field(a0), METHOD_FORWARD, next, a1 - 1, a2)

where, in u64 wrapping arithmetic (the device's), ``w = a2 mod 2^64``,
``stride = w & 0xffffffff``, ``n = w >> 32`` and ``next = ((a0 mod 2^64 + stride) mod 2^64) % n``
(``a0`` itself if ``n == 0``), reinterpreted as int64.  ``actor_field(a0)`` is ``a0`` for
``0 <= a0 < 2^32 - 1`` and ``0xffffffff`` (which names no actor) otherwise: a hop outside
the id space is never sent to the actor its low 32 bits spell.  The row answers OK even
if the outbox was full -- a drop shows in the count words only; without an outbox it
answers FAILED, the visit still counted.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD, METHOD_FORWARD, METHOD_SEQ_FOLD = 1, 3, 5, 6, 7
OK, FAILED, NO_ACTOR, OVERFLOW = 0, 2, 3, 4
FOLD_MUL = 0x100000001B3
U64 = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
NO_ACTOR_FIELD = 0xFFFFFFFF


def i64(x: int) -> int:
    """The low 64 bits of x as a signed integer."""
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def actor_field(a0: int) -> int:
    return a0 if 0 <= a0 < NO_ACTOR_FIELD else NO_ACTOR_FIELD


def next_hop(a0: int, a2: int) -> int:
    w = a2 & U64
    stride, n = w & 0xFFFFFFFF, w >> 32
    return i64((((a0 & U64) + stride) & U64) % n) if n else a0


def emitted_record(a0: int, a1: int, a2: int) -> tuple:
    return (actor_field(a0), METHOD_FORWARD, next_hop(a0, a2), a1 - 1, a2)


class ForwardSpec:
    """What one Send must have done (see ``forward_spec``)."""

    def __init__(self, M, n_state, state0):
        self.M = M
        self.status = [NO_ACTOR] * M
        self.value = [None] * M          # exact replies (ordered runs; stateless methods always)
        self.value_sets = {}             # unordered: mailbox -> (row indices, sorted expected replies)
        self.visits = [0] * n_state      # Forward visits per mailbox
        self.state_after = [int(s) for s in state0]
        self.emitted = []                # the multiset of records, as a list of 5-tuples
        self.emitters = []               # the rows that emitted

    @property
    def E(self) -> int:
        return len(self.emitted)

    def outbox_after(self, cap: int) -> dict:
        """The count words and the number of filled slots of an outbox of ``cap`` slots."""
        return {"count": (self.E, max(0, self.E - cap)), "filled": min(self.E, cap)}

    def check_outbox(self, cap: int, count, records) -> None:
        """``count``: the two count words; ``records``: the first ``min(E, cap)`` slots as
        5-tuples.  (That the other slots are untouched is the caller's guard check.)"""
        want = self.outbox_after(cap)
        assert (int(count[0]), int(count[1])) == want["count"], (tuple(int(c) for c in count), want)
        got = Counter(tuple(int(x) for x in r) for r in records)
        assert sum(got.values()) == want["filled"], (sum(got.values()), want)
        ref = Counter(self.emitted)
        if self.E <= cap:
            if got != ref:
                extra, missing = got - ref, ref - got
                raise AssertionError(f"outbox records differ: {sum(extra.values())} unexpected "
                                     f"{sorted(extra.items())[:4]}, {sum(missing.values())} missing "
                                     f"{sorted(missing.items())[:4]}")
        else:
            extra = got - ref
            assert not extra, f"outbox holds records no row emitted: {sorted(extra.items())[:4]}"

    def check_replies(self, status, value) -> None:
        """Exact statuses; replies on OK rows (exact, or per mailbox as a multiset)."""
        status = [int(s) for s in status]
        bad = [i for i in range(self.M) if status[i] != self.status[i]]
        assert not bad, f"{len(bad)} statuses differ, first rows {[(i, status[i], self.status[i]) for i in bad[:6]]}"
        self.check_values(value)

    def check_values(self, value) -> None:
        """The replies of this spec's OK rows (its other rows are not looked at)."""
        value = [int(v) for v in value]
        bad = [i for i in range(self.M) if self.status[i] == OK and self.value[i] is not None
               and value[i] != self.value[i]]
        assert not bad, f"{len(bad)} replies differ, first rows {[(i, value[i], self.value[i]) for i in bad[:6]]}"
        for mb, (rows, want) in self.value_sets.items():
            got = sorted(value[i] for i in rows)
            assert got == want, f"mailbox {mb}: replies {got[:6]}.. are not {want[:6]}.. ({len(rows)} rows)"


def forward_spec(rows, resolve, n_state, state0, outbox_bound, ran=None, ordered=False) -> ForwardSpec:
    """``rows = (actor, method, a0, a1, a2)``: columns (``method`` one id or a column,
    ``a1`` / ``a2`` None = zeros); ``resolve[i]``: row i's mailbox on this rank or None;
    ``state0``: ``n_state`` initial values; ``ran``: mask of the resolved rows that ran
    (default all; a resolved row that did not run answers OVERFLOW and does nothing).
    ``ordered``: each mailbox ran its rows one at a time in message order, so every reply
    is exact; otherwise a mailbox's state-touching rows must all add the same amount and
    their replies are checked as a multiset (any other mix has no order-free answer)."""
    actor, method, a0, a1, a2 = rows
    M = len(a0)
    col = (lambda c: [0] * M if c is None else [int(x) for x in c])
    a0, a1, a2 = col(a0), col(a1), col(a2)
    method = [int(method)] * M if isinstance(method, (int, np.integer)) else [int(x) for x in method]
    sp = ForwardSpec(M, n_state, state0)
    touched = {}  # unordered: mailbox -> [(row, delta)]
    for i in range(M):
        mb = resolve[i]
        if mb is None:
            continue
        if ran is not None and not bool(ran[i]):
            sp.status[i] = OVERFLOW
            continue
        me = method[i]
        if me == METHOD_CALC_MULTIPLY:
            sp.status[i], sp.value[i] = OK, i64(a0[i] * a1[i])
            continue
        if me == METHOD_ECHO:
            sp.status[i], sp.value[i] = OK, a0[i]
            continue
        if me not in (METHOD_COUNTER_ADD, METHOD_FORWARD, METHOD_SEQ_FOLD):
            raise ValueError(f"row {i}: method {me} is outside this spec")
        if mb >= n_state:
            continue  # NO_ACTOR: no visit, no emit
        sp.status[i] = OK
        if me == METHOD_SEQ_FOLD:
            if not ordered:
                raise ValueError("SeqFold has no order-free answer")
            sp.value[i] = sp.state_after[mb]
            sp.state_after[mb] = i64(sp.state_after[mb] * FOLD_MUL + a0[i])
            continue
        delta = 1 if me == METHOD_FORWARD else a0[i]
        sp.state_after[mb] = i64(sp.state_after[mb] + delta)
        if ordered:
            sp.value[i] = sp.state_after[mb]
        else:
            touched.setdefault(mb, []).append((i, delta))
        if me == METHOD_FORWARD:
            sp.visits[mb] += 1
            if a1[i] > 0:
                if outbox_bound:
                    sp.emitted.append(emitted_record(a0[i], a1[i], a2[i]))
                    sp.emitters.append(i)
                else:
                    sp.status[i] = FAILED
    for mb, hits in touched.items():
        deltas = {d for _, d in hits}
        if len(deltas) != 1:
            raise ValueError(f"mailbox {mb}: rows adding {sorted(deltas)} have no order-free replies")
        d, s0 = deltas.pop(), int(state0[mb])
        ok_rows = [i for i, _ in hits if sp.status[i] == OK]
        if len(ok_rows) == len(hits):
            sp.value_sets[mb] = (ok_rows, sorted(i64(s0 + d * (j + 1)) for j in range(len(hits))))
        # (rows that answered FAILED carry no reply: which of the counts they took is unknown,
        # so such a mailbox is held to its final state only)
    return sp


# ---------------------------------------------------------------------------------------------
A1_SILENT = [INT64_MIN, -1, 0]
A1_EMIT = [1, 2, INT64_MAX]
CADD_DELTA = 7  # every CounterAdd row of a corpus adds this (order-free replies)


def _a0_edges(N):
    return [0, N - 1, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 5, -1, -3, INT64_MIN, INT64_MAX]


def _a2_edges(N):
    return [0,
            5,                                    # stride only: n = 0
            3 | (1 << 32),                        # n = 1
            i64((2**32 - 1) | ((2**32 - 1) << 32)),  # stride = n = 2^32 - 1 (the word is -1)
            i64((1 << 63) | (9 << 32) | 4),       # top bit set: n >= 2^31 as u64
            (2**32 - 1) | (1000 << 32)]           # with a0 = -1, -3: a0 + stride wraps 2^64


def wants_emit(M: int) -> np.ndarray:
    """The emit-lane pattern, per 64-row group: tile 2 of every 3 (1024 rows) is silent;
    block 3 of every 4 (256 rows) has one emitting wave; the other groups cycle through
    all lanes, none, lane 0 only, lane 63 only and alternating lanes."""
    i = np.arange(M)
    lane, g, blk, tile = i % 64, i // 64, i // 256, i // 1024
    cyc = g % 5
    w = np.select([cyc == 0, cyc == 1, cyc == 2, cyc == 3], [np.ones(M, bool), np.zeros(M, bool), lane == 0, lane == 63],
                  lane % 2 == 0)
    w = np.where(blk % 4 == 3, g % 4 == 1, w)
    return np.where(tile % 3 == 2, False, w)


def forward_corpus(M, N, n_state, seed, method_column=False, two_args=False, emit="pattern", max_a1=None,
                   narrow=False, identity=False) -> dict:
    """A hostile batch of M rows over registered actors [0, N) (on a permuted mailbox map)
    and unknown ids [N, N + N/10), for a state of ``n_state < N`` mailboxes.

    ``emit``: "pattern" (``wants_emit``) or "all" (every row reaches a counted mailbox and
    sends).  ``max_a1`` caps a1 (terminating chains).  ``narrow``: in-range a0 and small a1
    only, except a handful of rows (values that fit narrow record fields, and a few that
    do not).  ``identity``: actor id = mailbox (an affine registry) instead of the permuted
    map.  Returns the columns (numpy), ``mbox_of`` (int64[N]) and ``resolve``."""
    rng = np.random.default_rng(seed)
    mbox_of = rng.permutation(N).astype(np.int64)
    if identity:
        mbox_of = np.arange(N, dtype=np.int64)
    good = np.nonzero(mbox_of < n_state)[0]   # registered, and inside the state
    emits = wants_emit(M) if emit == "pattern" else np.ones(M, bool)
    actor = rng.integers(0, N + max(1, N // 10), M)
    # the emitting lanes of the sparse patterns, and of "all", reach a counted mailbox
    g = np.arange(M) // 64
    sparse = emits & ((g % 5 >= 2) | ((np.arange(M) // 256) % 4 == 3)) if emit == "pattern" else emits
    actor = np.where(sparse, good[rng.integers(0, len(good), M)], actor)
    hot = int(good[0])
    actor[rng.permutation(M)[: min(200, M // 4)]] = hot

    a1_emit = A1_EMIT + [int(x) for x in rng.integers(1, 40, 5)]
    a1_silent = A1_SILENT + [int(x) for x in -rng.integers(1, 40, 2)]
    if max_a1 is not None or narrow:
        cap = 3 if max_a1 is None else max_a1
        a1_emit = [x for x in a1_emit if x <= cap] or [1]
    if narrow:
        a1_silent = [-1, 0]
    a1 = np.array([a1_emit[k % len(a1_emit)] if e else a1_silent[k % len(a1_silent)]
                   for k, e in zip(rng.integers(0, 1 << 30, M), emits)], dtype=np.int64)

    a0 = rng.integers(0, N + max(1, N // 10), M).astype(np.int64)
    edges0 = np.array(_a0_edges(N), dtype=np.int64)
    if narrow:
        pick = rng.permutation(M)[: min(M, 12)]
        a0[pick] = edges0[np.arange(len(pick)) % len(edges0)]
    else:
        pick = rng.random(M) < 0.4
        a0[pick] = edges0[rng.integers(0, len(edges0), int(pick.sum()))]

    ring = np.int64(7 | (N << 32))  # the ordinary ring word
    a2 = np.full(M, ring, dtype=np.int64)
    edges2 = np.array(_a2_edges(N), dtype=np.int64)
    pick = rng.random(M) < 0.4
    a2[pick] = edges2[rng.integers(0, len(edges2), int(pick.sum()))]

    method = METHOD_FORWARD
    if method_column:
        method = np.full(M, METHOD_FORWARD, dtype=np.int64)
        other = (rng.random(M) < 0.3) & ~sparse
        kinds = np.array([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD])
        method[other] = kinds[rng.integers(0, 3, int(other.sum()))]
        cadd = method == METHOD_COUNTER_ADD
        # CounterAdd rows keep to mailboxes no Forward row visits, and all add CADD_DELTA
        reserved = good[-max(1, len(good) // 8):]
        fwd_hits = (method == METHOD_FORWARD) & np.isin(actor, reserved)
        actor[fwd_hits] = hot
        actor[cadd] = reserved[rng.integers(0, len(reserved), int(cadd.sum()))]
        a0[cadd] = CADD_DELTA
    resolve = [int(mbox_of[a]) if a < N else None for a in actor]
    return {"actor": actor.astype(np.int32), "method": method, "a0": a0, "a1": a1, "a2": None if two_args else a2,
            "mbox_of": mbox_of, "resolve": resolve, "N": N, "n_state": n_state, "emits": emits}


def corpus_rows(c: dict) -> tuple:
    return (c["actor"], c["method"], c["a0"], c["a1"], c["a2"])


def simulate_pump(c: dict, state0, max_epochs=64):
    """``ActorExchange.pump`` over the corpus, iterating the spec epoch by epoch: the
    emitted records are the next epoch's batch.  Returns (epochs, delivered, final state)."""
    rows, resolve = corpus_rows(c), c["resolve"]
    state = [int(s) for s in state0]
    epochs, delivered = 0, len(c["a0"])
    mbox_of, N = c["mbox_of"], c["N"]
    while True:
        sp = forward_spec(rows, resolve, c["n_state"], state, True)
        state = sp.state_after
        if not sp.E or epochs >= max_epochs:
            return epochs, delivered, state
        epochs += 1
        delivered += sp.E
        cols = list(zip(*sp.emitted))
        rows = (cols[0], METHOD_FORWARD, cols[2], cols[3], cols[4])
        resolve = [int(mbox_of[a]) if a < N else None for a in cols[0]]
