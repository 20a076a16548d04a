"""Reply cache (``DeviceRuntime.send(cache=True)``): pure calls answered from HBM
across the Sends of one runtime.

Coalescing (``ops/coalesce.py``) is Go's ``singleflight`` per Send; this is the
cache that sits next to it in a Go service: a question asked in Send k is not
asked again in Send k + 1.  The key is coalescing's -- ``(actor id as the caller
wrote it, method, a0, a1, a2)``, a missing ``a1`` / ``a2`` column counting as 0,
actor ids compared as uint32 -- and only a ``STATUS_OK`` reply of a method in
``records.PURE_METHODS`` is ever stored or served.

The table (``csrc/hip/reply_cache.hpp``) is direct-mapped: ``1 << n`` entries of
one 64-B line, slot = ``key_hash & mask``; the hash only picks the slot, a hit
compares all five fields.  As eight uint64 words an entry is ``k0 = actor |
method << 32``, ``a0``, ``a1``, ``a2``, ``value``, ``claim``, ``epoch`` (low 32
bits) and padding.  An entry is valid iff its epoch is the cache's; ``clear()`` is
``epoch += 1``.  Replacement is deterministic: every ``insert`` has a sequence
number, a row that may be stored (pure, ``STATUS_OK``) lowers its slot's claim
word to ``(0xFFFFFFFF - seq) << 32 | row`` and the row whose word the slot holds
afterwards writes the entry -- the newest insert always replaces, and within one
insert the lowest row wins.  When the epoch or the sequence number would wrap 32
bits the table is rewritten (every entry cleared: epoch 0, claim all ones) and
both start over.

Three steps (``csrc/hip/reply_cache.hip``), all on the Send's stream:

* ``lookup``: ``(val int64[M], st int32[M])`` -- a hit has its stored value and
  ``STATUS_OK``; a miss and every non-pure message have ``st = PENDING``, a marker
  no handler returns (``val`` is then undefined)
* the misses are compacted by ``retry.select_mask`` on that marker, sent, and their
  replies put back by ``retry.merge``
* ``insert``: the sub-batch's rows and replies into the table

CUDA tensors run the kernels; CPU tensors run ``ReplyCacheRef`` (numpy, the same
slot rule and the same winner rule), which is also what the kernels are tested
against, table word for table word.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from . import retry as RT
from .batch import MsgBatch
from .coalesce import _key_columns, key_hash
from .records import PENDING, PURE_METHODS, STATUS_OK
from .retry import _cols

MIN_LOG2, MAX_LOG2 = 4, 26  # reply_cache.hpp kReplyCacheMinLog2 / kReplyCacheMaxLog2
DEFAULT_ENTRIES = 1 << 20   # 64 MiB
WORDS = 8                   # uint64 words per entry
W_K0, W_A0, W_A1, W_A2, W_VALUE, W_CLAIM, W_EPOCH = range(7)
_U32 = 0xFFFFFFFF
_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def entries_log2(entries: int) -> int:
    """log2 of the table for ``entries``: rounded up to a power of two and clamped
    to ``[1 << 4, 1 << 26]``."""
    return min(MAX_LOG2, max(MIN_LOG2, (max(int(entries), 1) - 1).bit_length()))


def _uniform_non_pure(batch: MsgBatch) -> bool:
    return isinstance(batch.method, int) and (int(batch.method) & 0xFFFF) not in PURE_METHODS


class ReplyCacheRef:
    """The reply cache on the host: the table is ``uint64[entries, 8]`` in numpy.
    ``_start=(epoch, seq)`` starts the two counters elsewhere (the tests start them
    near the 32-bit wrap)."""

    def __init__(self, device="cpu", entries: int = DEFAULT_ENTRIES, _start=None):
        self.device = torch.device(device)
        self.log2 = entries_log2(entries)
        self.entries = 1 << self.log2
        self.epoch, self.seq = (1, 0) if _start is None else (int(_start[0]), int(_start[1]))
        if not (1 <= self.epoch <= _U32 and 0 <= self.seq <= _U32):
            raise ValueError("reply cache: epoch must be in [1, 2^32) and seq in [0, 2^32)")
        self.table = None  # allocated and cleared by the first lookup / insert
        # host counters (K is on the host anyway): cached Sends, their messages, the hits, the misses sent on
        self.counters = {"sends": 0, "messages": 0, "hits": 0, "sent": 0, "clears": 0}

    # ---- the three table operations (ReplyCache runs them on the device)
    def _rewrite(self) -> None:
        self.table = np.zeros((self.entries, WORDS), dtype=np.uint64)
        self.table[:, W_CLAIM] = _ONES

    def _lookup(self, batch: MsgBatch):
        M = batch.M
        actor, method, a0, a1, a2 = _key_columns(batch)
        pure = np.isin(method, np.array(sorted(PURE_METHODS), dtype=np.uint16))
        slot = (key_hash(actor, method, a0, a1, a2) & np.uint64(self.entries - 1)).astype(np.int64)
        e = self.table[slot]
        k0 = actor.astype(np.uint64) | (method.astype(np.uint64) << np.uint64(32))
        hit = pure & (e[:, W_K0] == k0) & ((e[:, W_EPOCH] & np.uint64(_U32)) == np.uint64(self.epoch))
        for w, x in ((W_A0, a0), (W_A1, a1), (W_A2, a2)):
            hit &= e[:, w] == np.ascontiguousarray(x).view(np.uint64)
        val = np.where(hit, e[:, W_VALUE].view(np.int64), 0).reshape(M)
        st = np.where(hit, STATUS_OK, PENDING).astype(np.int32).reshape(M)
        return torch.from_numpy(val), torch.from_numpy(st)

    def _insert(self, sub: MsgBatch, val: torch.Tensor, st: torch.Tensor, seq: int) -> None:
        actor, method, a0, a1, a2 = _key_columns(sub)
        pure = np.isin(method, np.array(sorted(PURE_METHODS), dtype=np.uint16))
        rows = np.flatnonzero(pure & (st.detach().cpu().numpy() == STATUS_OK))
        if not rows.size:
            return
        slot = (key_hash(actor, method, a0, a1, a2) & np.uint64(self.entries - 1)).astype(np.int64)[rows]
        claim = np.uint64((_U32 - seq) << 32) | rows.astype(np.uint64)
        t = self.table
        np.minimum.at(t[:, W_CLAIM], slot, claim)
        won = t[slot, W_CLAIM] == claim
        rows, slot = rows[won], slot[won]
        u64 = (lambda x: np.ascontiguousarray(x).view(np.uint64)[rows])
        t[slot, W_K0] = actor.astype(np.uint64)[rows] | (method.astype(np.uint64)[rows] << np.uint64(32))
        t[slot, W_A0], t[slot, W_A1], t[slot, W_A2] = u64(a0), u64(a1), u64(a2)
        t[slot, W_VALUE] = u64(val.detach().cpu().to(torch.int64).numpy())
        t[slot, W_EPOCH] = np.uint64(self.epoch)

    def words(self) -> np.ndarray:
        """The whole table as ``uint64[entries, 8]`` on the host."""
        self._ready()
        return self.table

    # ---- the cache
    def _ready(self) -> None:
        if self.table is None:
            self._rewrite()

    def _restart(self) -> None:
        self._rewrite()
        self.epoch, self.seq = 1, 0

    def clear(self) -> None:
        """Drop every entry: O(1), the epoch moves on (the table is rewritten only
        when the epoch would wrap)."""
        self.counters["clears"] += 1
        if self.table is None:
            return
        if self.epoch == _U32:
            self._restart()
        else:
            self.epoch += 1

    def lookup(self, batch: MsgBatch):
        """``(val int64[M], st int32[M])``: ``st[i]`` is ``STATUS_OK`` and ``val[i]`` the
        stored value for a pure message whose key the table holds; ``PENDING`` for a
        miss and for every non-pure message (``val[i]`` is then undefined)."""
        self._ready()
        return self._lookup(batch)

    def insert(self, sub: MsgBatch, val: torch.Tensor, st: torch.Tensor) -> None:
        """The rows of ``sub`` with their replies into the table: the pure rows with
        ``STATUS_OK``; per slot the lowest such row replaces whatever was there."""
        if val.numel() != sub.M or st.numel() != sub.M:
            raise ValueError("insert: val and st must have one entry per row")
        self._ready()
        if self.seq == _U32 + 1:  # the sequence number would wrap
            self._restart()
        self._insert(sub, val, st, self.seq)
        self.seq += 1

    def send(self, batch: MsgBatch, send, collective: bool = False):
        """One cached Send: look ``batch`` up, compact the misses (stably, in message
        order; a non-pure message is always a miss), ``send(sub)`` them -- ``send``
        takes a MsgBatch and returns ``(value, status, ...)``, final on return --
        store their replies and merge them with the hits.  ``send`` is called at most
        once: exactly once when ``collective`` (a rank whose batch was all hits joins
        with an empty batch), not at all for K == 0 otherwise.  A batch with a
        uniform non-pure method is handed to ``send`` as it is, untouched."""
        M = batch.M
        c = self.counters
        c["sends"] += 1
        c["messages"] += M
        if _uniform_non_pure(batch):
            c["sent"] += M
            return send(batch)
        val, st = self.lookup(batch)
        return RT.send_pending(batch, val, st, send, collective, self._count,
                               lambda sub, out: self.insert(sub, out[0], out[1]))

    def _count(self, hits: int, sent: int) -> None:
        self.counters["hits"] += hits
        self.counters["sent"] += sent


class ReplyCache(ReplyCacheRef):
    """The reply cache of one rank on ``device``: on a GPU the table lives in HBM
    (``int64[entries, 8]``, allocated by the first cached Send) and the kernels run on
    the current stream; on the CPU it is the host reference.

    One stream: the launch boundaries of one stream are the only ordering between an
    insert's claim and write launches and the next lookup, and the table outlives the
    Send.  Every ``lookup`` / ``insert`` / ``clear`` / ``send`` of one cache must be
    issued on the same stream, or on streams the caller has ordered after one another;
    no event is recorded here."""

    def _gpu(self) -> bool:
        return self.device.type == "cuda"

    def _rewrite(self) -> None:
        if not self._gpu():
            return super()._rewrite()
        if self.table is None:
            self.table = torch.empty((self.entries, WORDS), dtype=torch.int64, device=self.device)
        hip().reply_cache_clear(_ptr(self.table), self.log2, raw_stream(self.device))

    def _key_args(self, batch: MsgBatch):
        actor, a0, a1, a2, method, uniform = _cols(batch)
        return (_ptr(actor), _ptr(method), int(batch.method) & 0xFFFF if uniform else 0, _ptr(a0), _ptr(a1),
                _ptr(a2)), (actor, a0, a1, a2, method)

    def _lookup(self, batch: MsgBatch):
        if not self._gpu():
            return super()._lookup(batch)
        M = batch.M
        val = torch.empty(M, dtype=torch.int64, device=self.device)
        st = torch.empty(M, dtype=torch.int32, device=self.device)
        if M and _uniform_non_pure(batch):  # no entry would be read: no kernel either
            st.fill_(PENDING)
        elif M:
            args, keep = self._key_args(batch)
            hip().reply_cache_lookup(*args, M, _ptr(self.table), self.log2, self.epoch, _ptr(val), _ptr(st),
                                     raw_stream(self.device))
            del keep
        return val, st

    def _insert(self, sub: MsgBatch, val: torch.Tensor, st: torch.Tensor, seq: int) -> None:
        if not self._gpu():
            return super()._insert(sub, val, st, seq)
        K = sub.M
        if K == 0 or _uniform_non_pure(sub):
            return
        if val.dtype != torch.int64 or st.dtype != torch.int32:
            raise TypeError("insert: val int64, st int32")
        val, st = val.contiguous(), st.contiguous()
        args, keep = self._key_args(sub)
        hip().reply_cache_insert(*args, K, _ptr(val), _ptr(st), _ptr(self.table), self.log2, self.epoch, seq,
                                 raw_stream(self.device))
        del keep

    def words(self) -> np.ndarray:
        self._ready()
        if not self._gpu():
            return self.table
        return self.table.cpu().numpy().view(np.uint64)
