"""Dead-letter queue of a rank's Sends, kept on the device.

protoactor publishes a ``DeadLetterEvent`` for a message nobody could take, Akka
keeps ``deadLetters``; a message-queue user knows the matching redrive: re-send
what is in the queue and drop a letter only once it succeeded.  A batched Send
returns before the host has seen one status, and ``batch`` belongs to the caller,
so the letters live in HBM and carry the whole call.

A ``DeadLetters`` queue is a ring of ``entries`` 64-byte records plus one 64-byte
control line (layout: ``csrc/hip/dead_letters.hpp``, mirrored below).  ``append``
files the rows of a Send whose final status is in ``mask`` -- two kernel launches
(``csrc/hip/dead_letters.hip``), no host read, no atomics, capturable -- and ``take``
is the only place the host reads ``head`` and ``tail``:

* the rows ``i`` with ``status[i]`` in the mask take tickets ``head, head + 1, ...``
  in ascending ``i``; letter ``t`` lives in slot ``t % entries``
* of ``K > entries`` letters in one Send only the last ``entries`` are written (no
  slot is written twice in one Send)
* afterwards ``sends += 1``, ``head += K``, ``dropped`` grows by the number of tickets
  in ``[tail, head - entries)`` and ``tail = max(tail, head - entries)``
* a Send without a letter (an empty one too) counts as a Send and leaves every ring
  word alone

Record (u64 words, little-endian):

====  =====================================================================
w0    ticket + 1 (0: never written)
w1    ``sends`` after this Send (the first Send is 1)
w2    row ``u32`` | status ``i32`` << 32
w3    logical actor id ``u32`` | method ``u16`` << 32 | attempts ``u16`` << 48
w4    a0
w5    a1 (0 when the batch has no such column)
w6    a2 (alike)
w7    tag
====  =====================================================================

``attempts`` is 1 without a column, else ``min(u32(col[i]) + 1, 65535)``.  The queue is
the caller's view, like the ledger: a rank files the batches it sent.  CPU tensors
run the numpy model (``DeadLetterRef``), which is also what the kernels are tested
against, word for word.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from .batch import MsgBatch
from .records import STATUS_RANK_LOST, STATUS_NO_METHOD

# csrc/hip/dead_letters.hpp (checked against _hip.dead_letter_layout() by the GPU tests)
RECORD_WORDS, CTRL_WORDS = 8, 8
W_TICKET, W_SEQ, W_ROW_STATUS, W_ACTOR_METHOD_ATTEMPTS, W_A0, W_A1, W_A2, W_TAG = range(8)
C_HEAD, C_TAIL, C_DROPPED, C_SENDS, C_BASE, C_TORN, C_SEQ = range(7)
TILE = 4096  # rows per block (compact.hpp kCompactTile)
MIN_ENTRIES, MAX_ENTRIES = 64, 1 << 24
MAX_ATTEMPTS = 65535
DEFAULT_MASK = sum(1 << s for s in range(STATUS_NO_METHOD, STATUS_RANK_LOST + 1))  # statuses 1..6
_U64 = (1 << 64) - 1
COLUMNS = ("seq", "row", "status", "actor", "method", "attempts", "a0", "a1", "a2", "tag")


def dead_letter_mask(mask=None) -> int:
    """The validated 32-bit set of statuses that make a row a dead letter: an int (bit s
    set: status s), an iterable of statuses, or None for statuses 1 to 6.  Bit 0
    (``STATUS_OK``) is refused, and so is a status outside ``[1, 32)``."""
    if mask is None:
        return DEFAULT_MASK
    if not isinstance(mask, (int, np.integer)):
        m = 0
        for s in mask:
            s = int(s)
            if not 1 <= s < 32:
                raise ValueError(f"dead_letter_mask: status {s} cannot be named (1 .. 31; STATUS_OK is no dead letter)")
            m |= 1 << s
        mask = m
    mask = int(mask)
    if not 2 <= mask < (1 << 32) or mask & 1:
        raise ValueError("dead_letter_mask: an int in [2, 2^32) with bit 0 (STATUS_OK) clear")
    return mask


def check_entries(entries: int) -> int:
    entries = int(entries)
    if not MIN_ENTRIES <= entries <= MAX_ENTRIES or entries & (entries - 1):
        raise ValueError("dead_letter_entries: a power of two in [64, 2^24]")
    return entries


def fnv1a64(s: str) -> int:
    """FNV-1a (64 bit) of a service name: the tag a ``Client`` files its letters under."""
    h = 0xCBF29CE484222325
    for b in s.encode():
        h = ((h ^ b) * 0x100000001B3) & _U64
    return h


def _validate(batch: MsgBatch, status: torch.Tensor, attempts) -> None:
    M = batch.M
    if status.dtype != torch.int32 or status.numel() != M:
        raise TypeError("dead letters: status must be int32[M]")
    if batch.actor.dtype != torch.int32 or batch.a0.dtype != torch.int64 or batch.a0.numel() != M:
        raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    for t in (batch.a1, batch.a2):
        if t is not None and (t.dtype != torch.int64 or t.numel() != M):
            raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    if not isinstance(batch.method, int) and batch.method.numel() != M:
        raise TypeError("MsgBatch: the method column must have M entries")
    if attempts is not None and (attempts.dtype != torch.int32 or attempts.numel() != M):
        raise TypeError("dead letters: attempts must be int32[M]")


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy()


def _i64(x: int) -> int:
    x &= _U64
    return x - (1 << 64) if x >> 63 else x


@dataclass
class Letters:
    """What ``take`` copied out of the ring, in ticket order: ``n`` letters as SoA columns on
    the queue's device (``seq`` int64: the Send's number; ``row`` / ``status`` / ``actor`` /
    ``attempts`` int32; ``method`` int16; ``a0`` / ``a1`` / ``a2`` / ``tag`` int64), the
    first ``ticket`` and ``torn``: slots whose ticket word was not the expected one (0)."""

    n: int
    ticket: int
    torn: int
    seq: torch.Tensor
    row: torch.Tensor
    status: torch.Tensor
    actor: torch.Tensor
    method: torch.Tensor
    attempts: torch.Tensor
    a0: torch.Tensor
    a1: torch.Tensor
    a2: torch.Tensor
    tag: torch.Tensor

    def batch(self) -> MsgBatch:
        """The letters as the calls they were: logical actor ids, a method column."""
        return MsgBatch(self.actor, self.a0, self.a1, self.a2, self.method)


@dataclass
class Redrive:
    """What ``DeviceRuntime.redrive`` did: the ``letters`` it took out of the queue and the
    re-send's ``(value, status)``, row for row (a row that failed again is a new letter)."""

    letters: Letters
    value: torch.Tensor
    status: torch.Tensor

    @property
    def n(self) -> int:
        return self.letters.n


_DTYPES = {"seq": torch.int64, "row": torch.int32, "status": torch.int32, "actor": torch.int32,
           "method": torch.int16, "attempts": torch.int32, "a0": torch.int64, "a1": torch.int64, "a2": torch.int64,
           "tag": torch.int64}


class DeadLetterRef:
    """The numpy model: ``ring`` uint64[entries, 8] and ``ctrl`` uint64[8], word for word
    what the kernels leave in HBM."""

    def __init__(self, entries: int = 1 << 16, mask=None):
        self.entries, self.mask = check_entries(entries), dead_letter_mask(mask)
        self.ring = np.zeros((self.entries, RECORD_WORDS), dtype=np.uint64)
        self.ctrl = np.zeros(CTRL_WORDS, dtype=np.uint64)

    def in_mask(self, status: np.ndarray) -> np.ndarray:
        s = status.astype(np.int64)
        inside = (s >= 0) & (s < 32)
        return inside & (((self.mask >> np.where(inside, s, 0)) & 1) != 0)

    def append(self, batch: MsgBatch, status: torch.Tensor, attempts: torch.Tensor | None = None, tag: int = 0):
        _validate(batch, status, attempts)
        st = _np(status)
        rows = np.nonzero(self.in_mask(st))[0]
        K, E = int(rows.size), self.entries
        head, tail = int(self.ctrl[C_HEAD]), int(self.ctrl[C_TAIL])
        seq = int(self.ctrl[C_SENDS]) + 1
        self.ctrl[C_BASE], self.ctrl[C_SEQ] = head, seq  # (kernel scratch)
        if K > E:  # only the last `entries` letters are written
            pos = np.arange(K - E, K, dtype=np.uint64)
            rows = rows[K - E:]
        else:
            pos = np.arange(K, dtype=np.uint64)
        if rows.size:
            u32 = (lambda a: a.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))
            if isinstance(batch.method, int):
                m = np.full(rows.size, int(batch.method) & 0xFFFF, dtype=np.uint64)
            else:
                m = _np(batch.method.to(torch.int16))[rows].astype(np.int64).astype(np.uint64) & np.uint64(0xFFFF)
            if attempts is None:
                att = np.ones(rows.size, dtype=np.uint64)
            else:
                att = np.minimum(u32(_np(attempts)[rows]) + np.uint64(1), np.uint64(MAX_ATTEMPTS))
            col = (lambda t: np.zeros(rows.size, dtype=np.uint64) if t is None else _np(t)[rows].view(np.uint64))
            ticket = np.uint64(head) + pos
            rec = np.empty((rows.size, RECORD_WORDS), dtype=np.uint64)
            rec[:, W_TICKET] = ticket + np.uint64(1)
            rec[:, W_SEQ] = seq
            rec[:, W_ROW_STATUS] = rows.astype(np.uint64) | (u32(st[rows]) << np.uint64(32))
            rec[:, W_ACTOR_METHOD_ATTEMPTS] = u32(_np(batch.actor)[rows]) | (m << np.uint64(32)) | (att << np.uint64(48))
            rec[:, W_A0], rec[:, W_A1], rec[:, W_A2] = col(batch.a0), col(batch.a1), col(batch.a2)
            rec[:, W_TAG] = int(tag) & _U64
            self.ring[(ticket & np.uint64(E - 1)).astype(np.int64)] = rec
        head += K
        self.ctrl[C_SENDS], self.ctrl[C_HEAD] = seq, head
        if head - E > tail:
            self.ctrl[C_DROPPED] += np.uint64(head - E - tail)
            self.ctrl[C_TAIL] = head - E

    def take(self, max_letters: int | None = None, drain: bool = True) -> dict:
        """``{"n", "ticket", "torn", column: numpy array}`` of the unread letters (at most
        ``max_letters``), in ticket order."""
        head, tail = int(self.ctrl[C_HEAD]), int(self.ctrl[C_TAIL])
        n = head - tail if max_letters is None else min(head - tail, max(0, int(max_letters)))
        t = np.arange(tail, tail + n, dtype=np.uint64)
        rec = self.ring[(t & np.uint64(self.entries - 1)).astype(np.int64)]
        torn = int((rec[:, W_TICKET] != t + np.uint64(1)).sum())
        self.ctrl[C_TORN] += np.uint64(torn)
        if drain:
            self.ctrl[C_TAIL] = tail + n
        w2, w3 = rec[:, W_ROW_STATUS], rec[:, W_ACTOR_METHOD_ATTEMPTS]
        lo32 = (lambda w: (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32))
        return {"n": n, "ticket": tail, "torn": torn, "seq": rec[:, W_SEQ].view(np.int64), "row": lo32(w2),
                "status": lo32(w2 >> np.uint64(32)), "actor": lo32(w3),
                "method": ((w3 >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16),
                "attempts": lo32(w3 >> np.uint64(48)), "a0": rec[:, W_A0].view(np.int64),
                "a1": rec[:, W_A1].view(np.int64), "a2": rec[:, W_A2].view(np.int64), "tag": rec[:, W_TAG].view(np.int64)}

    def read(self) -> dict:
        c = [int(x) for x in self.ctrl]
        return {"entries": self.entries, "appended": c[C_HEAD], "unread": c[C_HEAD] - c[C_TAIL],
                "dropped": c[C_DROPPED], "sends": c[C_SENDS], "torn": c[C_TORN]}

    def reset(self) -> None:
        self.ring[:] = 0
        self.ctrl[:] = 0


class _Sink:
    """A queue with the ``attempts`` column and the ``tag`` of one Send bound: what the
    exchange's ``send(dead_letters=)`` takes."""

    def __init__(self, queue, attempts, tag):
        self.queue, self.attempts, self.tag = queue, attempts, tag

    def append(self, batch: MsgBatch, status: torch.Tensor) -> None:
        self.queue.append(batch, status, self.attempts, self.tag)


class DeadLetters:
    """The dead-letter ring of one rank, on ``device``.  ``max_rows``: the largest Send it
    will file without growing its workspace (one u32 per 4096 rows; a larger Send allocates
    a new one, which is not legal under graph capture -- the warm-up Sends of a ``SendGraph``
    do it before the capture).  The ring, the control line and the workspace are state that
    outlives a Send, and the order of the launches on the stream is their only protection:
    every ``append``, ``take`` and ``reset`` of a queue must be issued on the same stream (or
    on streams the caller orders after one another)."""

    def __init__(self, device, entries: int = 1 << 16, mask=None, max_rows: int = 0):
        self.device = torch.device(device)
        self.entries, self.mask = check_entries(entries), dead_letter_mask(mask)
        self.counters = {"redrives": 0, "redriven": 0}
        self.ref = None
        if self.device.type != "cuda":
            self.ref = DeadLetterRef(self.entries, self.mask)
            return
        self.ring = torch.zeros(self.entries, RECORD_WORDS, dtype=torch.int64, device=self.device)
        self.device = self.ring.device  # ("cuda" names the current device: what the tensors report)
        self.ctrl = torch.zeros(CTRL_WORDS, dtype=torch.int64, device=self.device)
        self._counts = torch.empty(max(1, (int(max_rows) + TILE - 1) // TILE), dtype=torch.int32, device=self.device)
        self._outgrown = []

    def bound(self, attempts: torch.Tensor | None = None, tag: int = 0) -> _Sink:
        return _Sink(self, attempts, tag)

    def append(self, batch: MsgBatch, status: torch.Tensor, attempts: torch.Tensor | None = None, tag: int = 0) -> None:
        """File the rows of one Send -- its batch under the ids its caller wrote and its
        final ``status`` int32[M] -- whose status is in the mask, on the current stream of
        the queue's device.  No host read and, for contiguous columns, no allocation (a
        status view that is not 16-byte aligned is read with scalar loads); legal under
        graph capture, and every replay appends again."""
        _validate(batch, status, attempts)
        if status.device != self.device or batch.actor.device != self.device:
            raise ValueError("dead letters: the Send's tensors live on another device than the queue")
        if self.ref is not None:
            self.ref.append(batch, status, attempts, tag)
            return
        M = batch.M
        tiles = max(1, (M + TILE - 1) // TILE)
        if tiles > self._counts.numel():
            # a captured Send keeps launching into the workspace it was captured with: an outgrown
            # one is kept alive, never freed (sizes at least double, so there are few of them)
            self._outgrown.append(self._counts)
            self._counts = torch.empty(max(tiles, 2 * self._counts.numel()), dtype=torch.int32, device=self.device)
        c = (lambda t: None if t is None else t.contiguous())
        uniform = isinstance(batch.method, int)
        method = None if uniform else c(batch.method.to(torch.int16))
        hip().dlq_append(_ptr(c(status)), M, self.mask, _ptr(c(batch.actor)), _ptr(method),
                         int(batch.method) & 0xFFFF if uniform else 0, _ptr(c(attempts)), _ptr(c(batch.a0)),
                         _ptr(c(batch.a1)), _ptr(c(batch.a2)), _i64(int(tag)), _ptr(self.ring), _ptr(self.ctrl),
                         self.entries, _ptr(self._counts), raw_stream(self.device))

    def _ctrl_host(self) -> list[int]:
        return [int(x) & _U64 for x in self.ctrl.cpu().tolist()]  # (a host read)

    def take(self, max_letters: int | None = None, drain: bool = True) -> Letters:
        """The unread letters (at most ``max_letters``), in ticket order and across the wrap,
        as SoA columns; with ``drain`` they leave the queue.  Reads ``head`` and ``tail`` on
        the host (so it is no part of a captured Send), and ``torn`` with the result."""
        if self.ref is not None:
            r = self.ref.take(max_letters, drain)
            cols = {k: torch.from_numpy(np.ascontiguousarray(r[k])) for k in COLUMNS}
            return Letters(r["n"], r["ticket"], r["torn"], **cols)
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("dead letters: take reads head and tail on the host; not under graph capture")
        w = self._ctrl_host()
        head, tail = w[C_HEAD], w[C_TAIL]
        n = head - tail if max_letters is None else min(head - tail, max(0, int(max_letters)))
        cols = {k: torch.empty(n, dtype=_DTYPES[k], device=self.device) for k in COLUMNS}
        if n == 0:
            return Letters(0, tail, 0, **cols)
        hip().dlq_take(_ptr(self.ring), _ptr(self.ctrl), self.entries, tail, n, bool(drain),
                       *(_ptr(cols[k]) for k in COLUMNS), raw_stream(self.device))
        torn = (int(self.ctrl[C_TORN].item()) & _U64) - w[C_TORN]
        return Letters(n, tail, torn, **cols)

    def read(self) -> dict:
        """The counters (a host read): ``entries``, ``appended`` (head), ``unread``,
        ``dropped``, ``sends``, ``torn`` and the host's ``redrives`` / ``redriven``."""
        if self.ref is not None:
            return dict(self.ref.read(), **self.counters)
        w = self._ctrl_host()
        return dict(entries=self.entries, appended=w[C_HEAD], unread=w[C_HEAD] - w[C_TAIL], dropped=w[C_DROPPED],
                    sends=w[C_SENDS], torn=w[C_TORN], **self.counters)

    def reset(self) -> None:
        """Empty the queue and zero every counter (asynchronous fills)."""
        self.counters = {"redrives": 0, "redriven": 0}
        if self.ref is not None:
            self.ref.reset()
            return
        self.ring.zero_()
        self.ctrl.zero_()
