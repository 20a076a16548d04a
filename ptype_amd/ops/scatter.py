"""Call scatter: Q questions expanded into the T calls of one Send, on the device.

The scatter half of the reference's scatter-gather (``splitWork``, coordinator.go:67-73;
``ops/gather.py`` is the gather half, ``watchReplies``, :91-98).  A ``Scatter`` is a rule
that turns question q of a short ``MsgBatch`` into ``n[q] >= 0`` calls.  ``first[q]`` is
the exclusive prefix of ``n``: question q owns the rows ``first[q] .. first[q] + n[q] - 1``
of the expanded batch, in question order, and ``group[row] = q``.  With ``k = row -
first[q]`` the three rules are

``Scatter.ranges(step, n_actors, first_lo=None, actor_base=0)`` -- ``splitWork`` for any
step.  ``t = a0[q]``; ``n[q] = 0`` for ``t <= 0``, else ``(t - 1) // step + 1`` (unsigned:
``t`` near ``INT64_MAX`` cannot overflow).  A row gets ``actor = (actor_base + row) %
n_actors`` (the global row, as ``models.optimus.FanOut`` does), ``a0 = k * step`` (``first_lo``
at ``k == 0`` when one is given), ``a1 = (k + 1) * step``, ``a2 = t``.  The question's own
``actor``, ``a1`` and ``a2`` are ignored.

``Scatter.members(offsets, members)`` -- one call to every member of a group (Akka's
``BroadcastRouter``, a pub/sub topic).  The CSR ``offsets`` int64[G + 1] / ``members``
int32[offsets[G]] lists every group's actor ids; the question's ``actor`` column names
the group ``g`` and ``n[q] = offsets[g + 1] - offsets[g]``.  A group id outside ``[0, G)``
gives ``n[q] = 0`` and is counted in ``oob``.  A row gets ``actor = members[offsets[g] +
k]`` and the question's own ``a0``, ``a1``, ``a2``.  Keeping the CSR in step with a store is
the caller's business; ``set_members`` replaces it.

``Scatter.topics(table)`` -- one call to every subscriber of a topic, from strided segments
(``ops/topics.py``: a ``TopicTable`` that follows the subscriptions kept in the replicated
store; no per-subscriber list exists anywhere).  The table is four arrays: ``seg_off``
int64[G + 1] (topic ``g`` owns the segments ``seg_off[g] .. seg_off[g + 1] - 1``), ``row_off``
int64[S + 1] (the exclusive prefix of the segment counts, every count >= 1), ``seg_start`` and
``seg_stride`` int32[S].  The question's ``actor`` column names the topic ``g``; ``n[q] =
row_off[seg_off[g + 1]] - row_off[seg_off[g]]``, 0 for ``g`` outside ``[0, G)`` (counted in
``oob``; a topic without a subscriber gives 0 and is not out of range).  Row ``k`` belongs to
the segment ``s`` of ``g`` with ``row_off[s] <= row_off[seg_off[g]] + k < row_off[s + 1]`` and
gets ``actor = seg_start[s] + seg_stride[s] * (row_off[seg_off[g]] + k - row_off[s])`` and
the question's own ``a0``, ``a1``, ``a2``.  Every expand reads the table as it then stands.

Queue subscriptions (``Scatter.topics(table, by="key")``, ``expand(questions, key=None)``).  The
table may also hold queue subscriptions (competing consumers; ``ops/topics.py``): ``q_off``
int64[G + 1] (topic ``g`` owns the queue subscriptions ``q_off[g] .. q_off[g + 1] - 1``) and
``q_seg`` int64[NQ + 1] (queue subscription ``j`` owns the segments ``q_seg[j] .. q_seg[j + 1] -
1``, which follow the ordinary ones in the segment arrays, and their ``c = row_off[q_seg[j + 1]]
- row_off[q_seg[j]]`` members).  After the rows of its topic's ordinary subscriptions a question
gets ONE row per queue subscription of the topic, in ``q_off``'s order, so ``n[q]`` grows by
``q_off[g + 1] - q_off[g]``.  That row goes to member ``m`` of the subscription -- the segment
``s`` with ``row_off[s] <= row_off[q_seg[j]] + m < row_off[s + 1]`` -- where

* ``by="key"`` (default): ``m = ((mix64(uint64(key[q])) >> 32) * c) >> 32`` in unsigned 64-bit
  arithmetic (``ops.table.mix64``; multiply-shift, not ``%``: a 64-bit remainder is a long
  emulated sequence on the device).  ``key`` is an int64[Q] column given to ``expand``, by
  default the questions' ``a0``.  The same key and the same membership always give the same
  member: per-key ordering.
* ``by="index"``: ``m = ((seq + q) mod 2**64) mod c``; ``seq`` is a u64 counter of the Scatter
  that starts at 0 and advances by Q after every expansion that used it (one over a table
  with a queue subscription): the replica router's round robin applied to publications.

A table without a queue subscription launches exactly the kernels it always did.

Either way the method is the question's: one id, or an int16 column copied per row.

``expand(questions)`` returns an ``Expansion`` whose tensors are views, of length T and
Q, of buffers the ``Scatter`` owns -- allocated once, for ``capacity`` rows and
``q_capacity`` questions, on the device of the first questions; valid in stream order,
overwritten by the next ``expand`` of the same object (``Gather``'s contract).  The
kernels (``csrc/hip/scatter.hip``: count, scan, first, expand) place rows without atomics,
so the result equals ``scatter_ref`` bit for bit.  ``expand`` reads 16 bytes on the host
between the third and the fourth launch: the total (u64, saturating) and ``oob``.  It is
therefore refused under graph capture, and a total above ``capacity`` raises before any
row is written (``first`` and ``n`` then hold the refused questions' counts).  A prepared
``Expansion`` carries no host read: ``Send(exp.batch, gather=exp.gather(op, sentinel))``
is an ordinary, capturable Send.  CPU tensors run ``scatter_ref``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from .batch import MsgBatch
from .gather import Gather

RULES = ("ranges", "members", "topics")  # scatter.hpp kScatterRanges, kScatterMembers, kScatterTopics
QUESTION_TILE = 1024            # scatter.hip kScatterQTile
TILE = 2048                     # scatter.hip kScatterTile
MAX_ROWS = (1 << 31) - 2        # scatter.hpp kScatterMaxRows
MAX_QUESTIONS = 1 << 26         # scatter.hpp kScatterMaxQuestions
MAX_STEP = (1 << 31) - 1        # scatter.hpp kScatterMaxStep
MAX_SEGMENTS = 1 << 24          # scatter.hpp kScatterMaxSegments
MAX_QUEUES = 1 << 24            # scatter.hpp kScatterMaxQueues
U64_MAX = (1 << 64) - 1
I32_MAX = (1 << 31) - 1


def _np(t, dtype):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


def scatter_counts(rule: "Scatter", questions: MsgBatch):
    """``(n, total, oob)``: the rows of every question as Python-int-safe uint64[Q], their
    sum saturating at ``2**64 - 1`` and the out-of-range group ids."""
    if rule.rule == "ranges":
        t = _np(questions.a0, np.int64)
        pos = t > 0
        n = np.zeros(t.size, dtype=np.uint64)
        n[pos] = (t[pos].astype(np.uint64) - np.uint64(1)) // np.uint64(rule.step) + np.uint64(1)
        oob = 0
    elif rule.rule == "topics":
        t = rule.table.host
        g = _np(questions.actor, np.int64)
        inside = (g >= 0) & (g < t["seg_off"].size - 1)
        gi = np.where(inside, g, 0)
        rows = t["row_off"][t["seg_off"][gi + 1]] - t["row_off"][t["seg_off"][gi]]
        if "q_off" in t:  # one row per queue subscription of the topic
            rows = rows + (t["q_off"][gi + 1] - t["q_off"][gi])
        n = np.where(inside, rows, 0).astype(np.uint64)
        oob = int((~inside).sum())
    else:
        g = _np(questions.actor, np.int64)
        inside = (g >= 0) & (g < rule.G)
        off = rule.offsets_host
        gi = np.where(inside, g, 0)
        n = np.where(inside, off[gi + 1] - off[gi], 0).astype(np.uint64) if rule.G else np.zeros(g.size, dtype=np.uint64)
        oob = int((~inside).sum())
    total = min(sum(int(x) for x in n), U64_MAX)
    return n, total, oob


def queue_pick(c, key=None, index=None) -> np.ndarray:
    """The member (uint64, in ``[0, c)``) of a queue subscription of ``c`` members (``1 <= c <=
    2**31 - 1``; a scalar or an array) that a publication reaches: by ``key`` (int64),
    ``((mix64(uint64(key)) >> 32) * c) >> 32``, or by ``index`` (``(seq + q) mod 2**64`` as
    uint64), ``index mod c``."""
    from .table import mix64

    c = np.asarray(c).astype(np.uint64)
    if (key is None) == (index is None):
        raise ValueError("queue_pick: exactly one of key= and index=")
    if index is not None:
        return np.asarray(index).astype(np.uint64) % c
    h = mix64(np.asarray(key).astype(np.int64).astype(np.uint64))
    return ((h >> np.uint64(32)) * c) >> np.uint64(32)  # ((< 2**32) * (< 2**31): no overflow)


def scatter_ref(rule: "Scatter", questions: MsgBatch, key=None) -> dict:
    """The spec in numpy: ``{"actor" int32[T], "a0" / "a1" / "a2" int64[T] (members, topics: None
    where the questions have none), "method" (the id, or int16[T]), "group" int32[T],
    "first" int64[Q], "n" int32[Q], "total", "oob"}`` as CPU tensors and Python ints.  Topics
    with queue subscriptions: ``key`` is the int64[Q] key column (default: ``a0``) of
    ``by="key"``; ``by="index"`` reads ``rule.seq`` and leaves it as it is."""
    n64, total, oob = scatter_counts(rule, questions)
    if total > MAX_ROWS:
        raise ValueError(f"scatter: {total} rows exceed the most one expansion holds ({MAX_ROWS})")
    n = n64.astype(np.int64)
    Q = n.size
    first = np.cumsum(n) - n
    group = np.repeat(np.arange(Q, dtype=np.int64), n)
    row = np.arange(total, dtype=np.int64)
    k = row - first[group]
    if rule.rule == "ranges":
        actor = (rule.actor_base + row) % rule.n_actors
        a0 = k * rule.step
        if rule.first_lo is not None:
            a0 = np.where(k == 0, np.int64(rule.first_lo), a0)
        a1 = (k + 1) * rule.step
        a2 = _np(questions.a0, np.int64)[group]
    else:
        g = _np(questions.actor, np.int64)[group]
        if not total:
            actor = np.zeros(0, dtype=np.int64)
        elif rule.rule == "members":
            actor = rule.members_host[rule.offsets_host[g] + k]
        else:
            t = rule.table.host
            at = t["row_off"][t["seg_off"][g]] + k
            if "q_off" in t and t["q_seg"].size > 1:
                ordinary = t["row_off"][t["seg_off"][g + 1]] - t["row_off"][t["seg_off"][g]]
                isq = k >= ordinary  # the queue rows follow the topic's ordinary rows
                j = (t["q_off"][g] + (k - ordinary))[isq]
                lo = t["row_off"][t["q_seg"][j]]
                c = t["row_off"][t["q_seg"][j + 1]] - lo
                gq = group[isq]
                if rule.by == "index":
                    with np.errstate(over="ignore"):
                        m = queue_pick(c, index=np.uint64(rule.seq) + gq.astype(np.uint64))
                else:
                    kcol = _np(questions.a0 if key is None else key, np.int64)
                    m = queue_pick(c, key=kcol[gq])
                at[isq] = lo + m.astype(np.int64)
            seg = np.searchsorted(t["row_off"], at, side="right") - 1  # (row_off is strictly increasing)
            actor = t["seg_start"][seg].astype(np.int64) + t["seg_stride"][seg].astype(np.int64) * (at - t["row_off"][seg])
        a0 = _np(questions.a0, np.int64)[group]
        a1 = None if questions.a1 is None else _np(questions.a1, np.int64)[group]
        a2 = None if questions.a2 is None else _np(questions.a2, np.int64)[group]
    method = questions.method
    if not isinstance(method, int):
        method = torch.from_numpy(_np(method, np.int16)[group])
    t = (lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)))
    return {"actor": t(actor, np.int32), "a0": t(a0, np.int64), "a1": t(a1, np.int64), "a2": t(a2, np.int64),
            "method": method, "group": t(group, np.int32), "first": t(first, np.int64),
            "n": t(np.minimum(n, I32_MAX), np.int32), "total": int(total), "oob": int(oob)}


@dataclass
class Expansion:
    """One ``Scatter.expand``: ``batch`` (T rows), ``group`` int32[T] (the question index),
    ``first`` int64[Q], ``n`` int32[Q], ``total`` and ``oob`` (Python ints).  Views of the
    Scatter's buffers: overwritten by its next ``expand``."""

    scatter: "Scatter"
    batch: MsgBatch
    group: torch.Tensor
    first: torch.Tensor
    n: torch.Tensor
    total: int
    oob: int

    @property
    def Q(self) -> int:
        return int(self.n.numel())

    def gather(self, op: str, sentinel=None) -> Gather:
        """``Gather(group, Q, op, sentinel)`` for a Send of ``batch``: one result per
        question (a question without rows: count 0, the op's identity or its sentinel,
        ``STATUS_OK``).  Kept per ``(Q, op)`` on the Scatter and re-pointed at this
        expansion, so repeated Asks of one shape allocate nothing."""
        return self.scatter._gather(self, op, sentinel)


@dataclass
class Answer:
    """What ``DeviceRuntime.ask`` / ``Client.Ask`` return: per question the Gather's
    ``value`` int64[Q], ``status`` / ``n_ok`` / ``count`` / ``bad_row`` int32[Q] (the
    Gather's own tensors: overwritten by the next Ask of that shape and op) and the
    expansion's ``first`` int64[Q], ``n`` int32[Q] and ``oob``; per call the ``(val, st)``
    the Send returned."""

    value: torch.Tensor
    status: torch.Tensor
    n_ok: torch.Tensor
    count: torch.Tensor
    bad_row: torch.Tensor
    first: torch.Tensor
    n: torch.Tensor
    oob: int
    val: torch.Tensor
    st: torch.Tensor


class Scatter:
    """A scatter rule with its output buffers (module docstring).  Build one with
    ``Scatter.ranges``, ``Scatter.members`` or ``Scatter.topics``."""

    def __init__(self, rule: str, capacity: int, q_capacity: int | None):
        if rule not in RULES:
            raise ValueError(f"Scatter: rule must be one of {RULES}")
        self.rule = rule
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= MAX_ROWS:
            raise ValueError(f"Scatter: capacity must be in [1, {MAX_ROWS}]")
        self.q_capacity = min(self.capacity, MAX_QUESTIONS) if q_capacity is None else int(q_capacity)
        if not 1 <= self.q_capacity <= MAX_QUESTIONS:
            raise ValueError(f"Scatter: q_capacity must be in [1, {MAX_QUESTIONS}]")
        self.device = None  # the buffers are allocated by the first expand, on its questions' device
        self._gathers: dict = {}
        # ranges
        self.step, self.n_actors, self.first_lo, self.actor_base = 1, 1, None, 0
        # members
        self.G, self.offsets, self.members_, self.offsets_host, self.members_host = 0, None, None, None, None
        # topics; queue subscriptions: the member by the key's hash or by index, the index counter (u64)
        self.table = None
        self.by, self.seq = "key", 0

    # ------------------------------------------------------------------ the three rules
    @classmethod
    def ranges(cls, step: int, n_actors: int, first_lo: int | None = None, actor_base: int = 0,
               capacity: int = 1 << 20, q_capacity: int | None = None) -> "Scatter":
        step, n_actors = int(step), int(n_actors)
        if not 1 <= step <= MAX_STEP:
            raise ValueError(f"Scatter.ranges: step must be in [1, {MAX_STEP}]")
        if not 1 <= n_actors <= I32_MAX:
            raise ValueError(f"Scatter.ranges: n_actors must be in [1, {I32_MAX}]")
        if first_lo is not None and not -(1 << 63) <= int(first_lo) < 1 << 63:
            raise ValueError("Scatter.ranges: first_lo must be an int64")
        s = cls("ranges", capacity, q_capacity)
        s.step, s.n_actors = step, n_actors
        s.first_lo = None if first_lo is None else int(first_lo)
        s.actor_base = int(actor_base) % n_actors
        return s

    @classmethod
    def members(cls, offsets: torch.Tensor, members: torch.Tensor, capacity: int = 1 << 20,
                q_capacity: int | None = None) -> "Scatter":
        s = cls("members", capacity, q_capacity)
        s.set_members(offsets, members)
        return s

    @classmethod
    def topics(cls, table, capacity: int = 1 << 20, q_capacity: int | None = None, by: str = "key") -> "Scatter":
        """``table``: an ``ops.topics.TopicTable`` (or anything with its ``host`` dict of numpy
        arrays, ``device_arrays(device)`` and ``max_topics``); ``set_table`` replaces it.  ``by``:
        how a queue subscription's member is picked, ``"key"`` or ``"index"`` (module docstring)."""
        if by not in ("key", "index"):
            raise ValueError('Scatter.topics: by must be "key" or "index"')
        s = cls("topics", capacity, q_capacity)
        s.by = by
        s.set_table(table)
        return s

    def set_table(self, table) -> None:
        if self.rule != "topics":
            raise ValueError("Scatter.set_table: not a topics rule")
        if not hasattr(table, "host") or not hasattr(table, "device_arrays"):
            raise ValueError("Scatter.topics: the table is an ops.topics.TopicTable")
        self.table = table

    def set_members(self, offsets: torch.Tensor, members: torch.Tensor) -> None:
        """Replace the group table (validated here, once: one host read of the CSR)."""
        if self.rule != "members":
            raise ValueError("Scatter.set_members: not a members rule")
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or \
                offsets.numel() < 1:
            raise ValueError("Scatter.members: offsets must be an int64[G + 1] tensor")
        if not isinstance(members, torch.Tensor) or members.dtype != torch.int32 or members.dim() != 1:
            raise ValueError("Scatter.members: members must be an int32 tensor of actor ids")
        if offsets.device != members.device:
            raise ValueError("Scatter.members: offsets and members live on different devices")
        if self.device is not None and offsets.device != self.device:
            raise ValueError("Scatter.members: the group table lives on another device than the buffers")
        off = _np(offsets, np.int64)
        if int(off[0]) != 0 or bool((np.diff(off) < 0).any()):
            raise ValueError("Scatter.members: offsets must start at 0 and never decrease")
        if int(off[-1]) != int(members.numel()):
            raise ValueError(f"Scatter.members: offsets end at {int(off[-1])}, members has {int(members.numel())}")
        if int(members.numel()) > MAX_ROWS or off.size - 1 > I32_MAX:
            raise ValueError("Scatter.members: the group table is too large")
        self.G = off.size - 1
        self.offsets, self.members_ = offsets.contiguous(), members.contiguous()
        self.offsets_host, self.members_host = off, _np(members, np.int64)

    # ------------------------------------------------------------------ buffers
    def _allocate(self, device) -> None:
        if self.rule == "members" and self.offsets.device != device:
            raise ValueError("Scatter: the questions live on another device than the group table")
        self.device = device
        new = (lambda k, dt: torch.empty(k, dtype=dt, device=device))
        C, QC = self.capacity, self.q_capacity
        self.actor, self.group = new(C, torch.int32), new(C, torch.int32)
        self.a0, self.a1, self.a2 = new(C, torch.int64), new(C, torch.int64), new(C, torch.int64)
        self.method = None  # int16[C], allocated by the first questions with a method column
        self.first, self.n = new(QC, torch.int64), new(QC, torch.int32)
        if device.type == "cuda":
            self.tile_cap = -(-QC // QUESTION_TILE)
            self.tsum, self.toob = new(self.tile_cap, torch.int64), new(self.tile_cap, torch.int64)
            self.ctr = torch.zeros(2, dtype=torch.int64, device=device)

    def _check(self, qs: MsgBatch) -> int:
        if not isinstance(qs, MsgBatch):
            raise ValueError("Scatter.expand: the questions are a MsgBatch")
        if qs.actor.dtype != torch.int32 or qs.a0.dtype != torch.int64:
            raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
        Q = int(qs.actor.numel())
        cols = [qs.a0, qs.a1, qs.a2] + ([] if isinstance(qs.method, int) else [qs.method])
        for c in cols:
            if c is None:
                continue
            if c.numel() != Q or c.device != qs.actor.device:
                raise ValueError("Scatter.expand: the question columns differ in length or device")
        for c in (qs.a1, qs.a2):
            if c is not None and c.dtype != torch.int64:
                raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
        if not isinstance(qs.method, int) and qs.method.dtype != torch.int16:
            raise TypeError("MsgBatch: a method column must be int16")
        if Q > self.q_capacity:
            raise ValueError(f"Scatter.expand: {Q} questions exceed q_capacity {self.q_capacity}")
        return Q

    def _queues(self) -> bool:
        """Whether the rule reads a table that holds a queue subscription."""
        return self.rule == "topics" and int(self.table.host.get("q_seg", np.zeros(1)).size) > 1

    def expand(self, questions: MsgBatch, key: torch.Tensor | None = None) -> Expansion:
        """Expand ``questions`` into the buffers (module docstring).  On a GPU: four
        launches on the current stream and one 16-byte host read.  ``key``: the int64[Q] key
        column of a topics rule's queue subscriptions (default: the questions' ``a0``)."""
        Q = self._check(questions)
        dev = questions.actor.device
        if key is not None:
            if self.rule != "topics":
                raise ValueError("Scatter.expand: key= belongs to the topics rule")
            if not isinstance(key, torch.Tensor) or key.dtype != torch.int64 or key.dim() != 1 or key.numel() != Q or \
                    key.device != dev:
                raise ValueError("Scatter.expand: key must be an int64[Q] tensor on the questions' device")
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise ValueError("Scatter.expand inside a captured Send: the total of the expansion is read on the host "
                             "(expand first, capture the Send of the prepared Expansion)")
        if self.device is None:
            self._allocate(dev)
        elif dev != self.device:
            raise ValueError("Scatter.expand: the questions live on another device than the buffers")
        mcol = not isinstance(questions.method, int)
        members = self.rule != "ranges"  # (members and topics copy the question's columns)
        has1 = not members or questions.a1 is not None
        has2 = not members or questions.a2 is not None
        if dev.type != "cuda":
            _, total, oob = scatter_counts(self, questions)
            self._refuse(total)
            ref = scatter_ref(self, questions, key=key)
            if mcol and self.method is None:
                self.method = torch.empty(self.capacity, dtype=torch.int16)
            for name in ("actor", "a0", "a1", "a2", "group"):
                if ref[name] is not None:
                    getattr(self, name)[:total].copy_(ref[name])
            if mcol:
                self.method[:total].copy_(ref["method"])
            self.first[:Q].copy_(ref["first"])
            self.n[:Q].copy_(ref["n"])
        elif Q == 0:
            total = oob = 0
        else:
            c = (lambda t: None if t is None else t.contiguous())
            cols = (c(questions.actor), c(questions.a0), c(questions.a1) if members else None,
                    c(questions.a2) if members else None, c(questions.method) if mcol else None)
            if self._queues() and self.by == "key":
                cols += (cols[1] if key is None else key.contiguous(),)
            self._count(cols, Q)
            ctr = self.ctr.cpu()  # the host read of an expansion: 16 bytes
            total, oob = int(ctr[0]) & U64_MAX, int(ctr[1])
            self._refuse(total)
            if mcol and self.method is None:
                self.method = torch.empty(self.capacity, dtype=torch.int16, device=dev)
            if total:
                self._fill(cols, Q, total)
        if Q and self.by == "index" and self._queues():
            self.seq = (self.seq + Q) & U64_MAX  # (after every expansion that used it, refused ones apart)
        batch = MsgBatch(self.actor[:total], self.a0[:total], self.a1[:total] if has1 else None,
                         self.a2[:total] if has2 else None, self.method[:total] if mcol else int(questions.method))
        return Expansion(self, batch, self.group[:total], self.first[:Q], self.n[:Q], total, oob)

    def _count(self, cols, Q: int) -> None:
        """The count, scan and first launches over the question columns ``cols`` (actor, a0,
        a1, a2, method; contiguous or None): ``n``, ``first`` and ``ctr`` on the device."""
        if self.rule == "topics":
            seg_off, G, row_off, n_segs, _, _, q_off, _, n_queues, _ = self._table_args()
            hip().scatter_count(2, _ptr(cols[0]), _ptr(cols[1]), Q, 1, seg_off, G, _ptr(self.n), _ptr(self.first),
                                _ptr(self.tsum), _ptr(self.toob), self.tile_cap, _ptr(self.ctr), raw_stream(self.device),
                                row_off, n_segs, q_off if n_queues else 0, n_queues)
            return
        hip().scatter_count(RULES.index(self.rule), _ptr(cols[0]), _ptr(cols[1]), Q, self.step, _ptr(self.offsets),
                            self.G, _ptr(self.n), _ptr(self.first), _ptr(self.tsum), _ptr(self.toob), self.tile_cap,
                            _ptr(self.ctr), raw_stream(self.device))

    def _fill(self, cols, Q: int, total: int) -> None:
        """The expand launch: ``total`` (what ``_count`` left in ``ctr[0]``, read and checked
        by the caller) rows of the batch columns and of ``group``."""
        members = self.rule != "ranges"
        out = (lambda buf, col: _ptr(buf) if not members or col is not None else 0)
        if self.rule == "topics":
            seg_off, G, row_off, n_segs, seg_start, seg_stride, q_off, q_seg, n_queues, n_all = self._table_args()
            queue = () if not n_queues else (q_off, q_seg, n_queues, n_all, 0 if self.by == "index" else _ptr(cols[5]),
                                             self.seq if self.by == "index" else 0, self.by == "index")
            hip().scatter_expand(2, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), _ptr(cols[4]), Q, 1, 1, 0,
                                 False, 0, seg_off, 0, G, 0, _ptr(self.first), _ptr(self.n), total, self.capacity,
                                 _ptr(self.actor), _ptr(self.a0), out(self.a1, cols[2]), out(self.a2, cols[3]),
                                 0 if cols[4] is None else _ptr(self.method), _ptr(self.group), raw_stream(self.device),
                                 row_off, seg_start, seg_stride, n_segs, *queue)
            return
        hip().scatter_expand(RULES.index(self.rule), _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]),
                             _ptr(cols[4]), Q, self.step, self.n_actors, self.actor_base, self.first_lo is not None,
                             self.first_lo or 0, _ptr(self.offsets), _ptr(self.members_), self.G,
                             0 if self.members_ is None else int(self.members_.numel()), _ptr(self.first), _ptr(self.n),
                             total, self.capacity, _ptr(self.actor), _ptr(self.a0), out(self.a1, cols[2]),
                             out(self.a2, cols[3]), 0 if cols[4] is None else _ptr(self.method), _ptr(self.group),
                             raw_stream(self.device))

    def _table_args(self):
        """``TopicTable.launch_args`` (a table of four arrays has no queue subscription)."""
        a = tuple(self.table.launch_args(self.device))
        return a if len(a) >= 10 else a[:6] + (0, 0, 0, a[3])

    def _refuse(self, total: int) -> None:
        if total > self.capacity:
            raise ValueError(f"Scatter.expand: the questions expand into {total} rows, the capacity is {self.capacity}")

    # ------------------------------------------------------------------ the gather of an expansion
    def _gather(self, exp: Expansion, op: str, sentinel) -> Gather:
        Q = exp.Q
        if Q < 1:
            raise ValueError("Expansion.gather: no questions, nothing to gather")
        sen = sentinel
        if op == "first_ne" and sentinel is not None and not isinstance(sentinel, torch.Tensor):
            # (a buffer of the Scatter's own: a caller's tensor is used as it is, never written)
            sen = self._gathers.get((Q, "sentinel"))
            if sen is None:
                sen = self._gathers[(Q, "sentinel")] = torch.empty(Q, dtype=torch.int64, device=self.device)
            sen.fill_(int(sentinel))
        g = self._gathers.get((Q, op))
        if g is None:
            g = self._gathers[(Q, op)] = Gather(exp.group, Q, op, sen)
            return g
        g.group, g.M = exp.group, int(exp.group.numel())
        if op == "first_ne":
            if sen is None:
                raise ValueError("Gather: first_ne needs a sentinel (int64[groups] or one int)")
            if sen.dtype != torch.int64 or sen.numel() not in (1, Q):
                raise ValueError("Gather: sentinel must be int64[groups] (or one int)")
            if sen.device != self.device:
                raise ValueError("Gather: the sentinel lives on another device than group")
            g.sentinel = sen.reshape(-1).expand(Q).contiguous()
        return g
