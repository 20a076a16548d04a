"""Rate limiter (``DeviceRuntime.send(limit=True)``): a token bucket per actor, across the
Sends of one runtime.

What ``golang.org/x/time/rate`` or Akka's ``throttle`` put around a call, per actor and on
the batch path: an actor gains ``rate`` tokens per limited Send and holds at most ``burst``;
every message costs one.  Of an actor whose rows in a batch exceed its tokens the first
ones in message order travel, the others are answered ``(0, STATUS_THROTTLED)`` and not
sent.

The key is the logical actor id as the caller wrote it (uint32), the method is not part
of it.  The table (``csrc/hip/limit.hpp``) is dense, ``n`` words of 64 bits: ``spent``
(bits 0..31, ``burst - tokens``) and ``last`` (bits 32..62, the tick of the last update);
the word is 0 whenever ``spent`` is 0, so a zero-filled table is every bucket full.  An id
outside ``[0, n)`` is never limited: it always passes and is counted in ``oob`` by every
limited Send.

Time is counted in limited Sends: ``tick`` starts at 1, a limited Send runs at ``now =
tick`` and then ``tick += 1``, even when the inner Send raises.  When the tick would pass
``2**31 - 1`` the limiter restarts (every word 0, tick 1).

Admission at ``now`` for an actor with ``d`` rows in the batch: ``refill = min((now - last)
* rate, 2**32 - 1)``, ``spent' = max(spent - refill, 0)`` (0 for a zero word), ``avail =
burst - spent'``, ``q = min(d, avail)``; the first ``q`` rows of the actor travel and the
new word is ``now << 32 | spent' + q``.  Tokens are spent at admission, whatever the rows'
replies turn out to be.  The counters kept with the table: ``throttled`` (rows rejected),
``oob`` and, during a Send, ``over`` (actors over their quota).

CUDA tensors run the kernels (``csrc/hip/limit.hip``); CPU tensors run ``LimiterRef``
(numpy), which is also what the kernels are tested against, word for word.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from . import retry as RT
from .batch import MsgBatch
from .records import PENDING, STATUS_THROTTLED

MAX_TICK = 2**31 - 1         # limit.hpp kLimitMaxTick
MAX_ACTORS = 1 << 28         # limit.hpp kLimitMaxActors
DIGIT = 4                    # limit.hpp kLimitDigit
MAX_HOT = (1 << 31 >> DIGIT) - 1  # limit.hpp kLimitMaxHot
HOT = 1 << 31                # limit.hpp kLimitHot
C_THROTTLED, C_OOB, C_OVER, C_TOUCHED = range(4)  # limit.hpp LimitCounter
COUNTERS = 2                 # the cumulative counters of the model (over and n_touched are 0 between Sends)
CTR_WORDS = 8 + 33           # limit.hpp kLimitCtrWords
BUSY_CAP = 1024              # limit.hpp kLimitBusyCap
_U32 = 0xFFFFFFFF
_u64 = np.uint64


def levels(M: int) -> int:
    """Levels of the radix select over the row indices of ``M`` messages (limit.hpp
    ``limit_levels``)."""
    return max(1, -(-max(M - 1, 0).bit_length() // DIGIT))


def spent_of(w):
    return (np.asarray(w, dtype=np.uint64) & _u64(_U32)).astype(np.int64)


def last_of(w):
    return ((np.asarray(w, dtype=np.uint64) >> _u64(32)) & _u64(0x7FFFFFFF)).astype(np.int64)


class LimiterRef:
    """The limiter on the host: ``table`` is ``uint64[n]`` in numpy, ``ctr`` the two
    cumulative counters.  ``_start=tick`` starts the tick elsewhere (the tests start it near
    the restart)."""

    def __init__(self, device="cpu", actors: int = 1024, rate: int = 1, burst: int = 1, _start=None):
        self.device = torch.device(device)
        self.n, self.rate, self.burst = int(actors), int(rate), int(burst)
        if not 1 <= self.n <= MAX_ACTORS:
            raise ValueError("limit: actors must be in [1, 2^28]")
        if not 1 <= self.rate <= _U32:
            raise ValueError("limit: rate must be in [1, 2^32)")
        if not 1 <= self.burst <= _U32:
            raise ValueError("limit: burst must be in [1, 2^32)")
        self.tick = 1 if _start is None else int(_start)
        if not 1 <= self.tick <= MAX_TICK + 1:
            raise ValueError("limit: the tick must be in [1, 2^31]")
        self.table = None  # allocated and cleared by the first limited Send
        self.over = 0      # actors over their quota in the last admission
        # host counters: limited Sends, their messages, the throttled ones, the ones sent on
        self.counters = {"sends": 0, "messages": 0, "rejected": 0, "sent": 0}

    # ---- the table operations (Limiter runs them on the device)
    def _clear(self) -> None:
        """Every word 0: every bucket full (``throttled`` and ``oob`` count on)."""
        if self.table is None:
            self.table = np.zeros(self.n, dtype=np.uint64)
            self.ctr = np.zeros(COUNTERS, dtype=np.uint64)
        self.table[:] = 0

    def _admit(self, batch: MsgBatch, now: int):
        """Spend the tokens of ``batch`` at ``now``.  None when no actor is over its quota
        (``self.over == 0``), else ``(val, st)``."""
        M = batch.M
        a = batch.actor.detach().cpu().contiguous().numpy().view(np.uint32).astype(np.int64)
        inb = a < self.n
        self.ctr[C_OOB] += _u64(int((~inb).sum()))
        rows = np.flatnonzero(inb)
        u, d = np.unique(a[rows], return_counts=True)
        w = self.table[u]
        refill = np.minimum((_u64(now) - last_of(w).astype(np.uint64)) * _u64(self.rate), _u64(_U32)).astype(np.int64)
        spent = np.where(w != 0, np.maximum(spent_of(w) - refill, 0), 0)
        avail = self.burst - spent
        q = np.minimum(d, avail)
        total = (spent + q).astype(np.uint64)
        self.table[u] = np.where(total != 0, (_u64(now) << _u64(32)) | total, _u64(0))
        hot = d > avail
        self.over = int(hot.sum())
        self.ctr[C_THROTTLED] += _u64(int((d - q)[hot].sum()))
        if self.over == 0:
            return None
        # the occurrence number of every row within its actor, in message order
        order = np.argsort(a[rows], kind="stable")
        start = np.cumsum(d) - d
        occurrence = np.arange(rows.size) - np.repeat(start, d)
        st = np.full(M, PENDING, dtype=np.int32)
        st[rows[order][occurrence >= np.repeat(q, d)]] = STATUS_THROTTLED
        return torch.zeros(M, dtype=torch.int64), torch.from_numpy(st)

    def words(self) -> np.ndarray:
        """The state table and the two cumulative counters (``throttled, oob``) as
        ``uint64[n + 2]`` on the host."""
        self._ready()
        return np.concatenate([self.table, self.ctr[:COUNTERS]])

    # ---- the limiter
    def _ready(self) -> None:
        if self.table is None:
            self._clear()

    def reset(self) -> None:
        """Fill every bucket (the tick goes on)."""
        if self.table is not None:
            self._clear()

    def begin(self) -> int:
        """Start a limited Send: its tick (the limiter restarts first when the tick would
        pass ``2**31 - 1``)."""
        self._ready()
        if self.tick > MAX_TICK:
            self._clear()
            self.tick = 1
        return self.tick

    def end(self) -> None:
        self.tick += 1

    def admit(self, batch: MsgBatch):
        """Spend the batch's tokens at the current tick.  None when no actor is over its
        quota: every row travels.  Else ``(val int64[M], st int32[M])``: ``st[i]`` is
        ``PENDING`` for a row that travels (a marker no handler returns) and
        ``STATUS_THROTTLED`` for a rejected one; ``val`` is 0."""
        self._ready()
        return self._admit(batch, self.tick)

    def read(self) -> dict:
        """The counters kept with the table (one host read on a GPU)."""
        w = self.words()[self.n:]
        return {"throttled": int(w[C_THROTTLED]), "oob": int(w[C_OOB])}

    def send(self, batch: MsgBatch, send, collective: bool = False):
        """One limited Send: spend the tokens, reject the rows past each actor's quota,
        compact the rest (stably, in message order), ``send(sub)`` them -- ``send`` takes
        a MsgBatch and returns ``(value, status, ...)``, final on return -- and merge
        their replies with the rejections.  With nothing over quota (one host read) the
        batch goes to ``send`` untouched.  ``send`` is called at most once: exactly once
        when ``collective`` (a rank whose batch was all throttled joins with an empty
        batch), not at all for K == 0 otherwise."""
        M = batch.M
        c = self.counters
        c["sends"] += 1
        c["messages"] += M
        self.begin()
        try:
            cut = self.admit(batch)
            if cut is None:
                c["sent"] += M
                return send(batch)
            # (an actor is over its quota, so a row is rejected: the driver's K == M case never runs here)
            return RT.send_pending(batch, cut[0], cut[1], send, collective, self._count)
        finally:
            self.end()

    def _count(self, rejected: int, sent: int) -> None:
        self.counters["rejected"] += rejected
        self.counters["sent"] += sent


class Limiter(LimiterRef):
    """The limiter of one rank on ``device``: on a GPU the tables live in HBM (28 B per
    actor, allocated by the first limited Send; the cut's scratch -- 4 B per message, 64 B
    per actor over quota -- grows with the Sends that need it) and the kernels run on the
    current stream; on the CPU it is the host reference.

    One stream: the launch boundaries of one stream are the only ordering between the
    launches of a limited Send and the next one's, and the tables outlive the Send.  Every
    call on one limiter must be issued on the same stream, or on streams the caller has
    ordered after one another; no event is recorded here."""

    def _gpu(self) -> bool:
        return self.device.type == "cuda"

    def _clear(self) -> None:
        if not self._gpu():
            return super()._clear()
        if self.table is None:
            new = (lambda dt: torch.empty(self.n, dtype=dt, device=self.device))
            self.table, self.demand = new(torch.int64), new(torch.int32)
            self.touched, self.hot_actor, self.rem, self.prefix = (new(torch.int32) for _ in range(4))
            self.ctr = torch.zeros(CTR_WORDS, dtype=torch.int64, device=self.device)
            # the busy actors of the last two Sends: a hint to the demand kernel's LDS cache
            self.busy = torch.zeros(2 * BUSY_CAP, dtype=torch.int32, device=self.device)
            # grow-only scratch of the cut; the bins are zero between Sends
            self.slot = torch.empty(0, dtype=torch.int32, device=self.device)
            self.bins = torch.zeros(0, dtype=torch.int32, device=self.device)
        hip().limit_clear(_ptr(self.table), _ptr(self.demand), _ptr(self.ctr), self.n, raw_stream(self.device))

    def _admit(self, batch: MsgBatch, now: int):
        if not self._gpu():
            return super()._admit(batch, now)
        M = batch.M
        self.over = 0
        if M == 0:
            return None
        if batch.actor.dtype != torch.int32:
            raise TypeError("MsgBatch: actor must be int32")
        actor = batch.actor.contiguous()
        h, s = hip(), raw_stream(self.device)
        h.limit_demand(_ptr(actor), M, _ptr(self.table), _ptr(self.demand), _ptr(self.touched), _ptr(self.hot_actor),
                       _ptr(self.rem), _ptr(self.prefix), _ptr(self.busy), _ptr(self.ctr), self.n, now, self.rate,
                       self.burst, s)
        over = self.over = int(self.ctr[C_OVER].item())  # the host read of a limited Send
        if over == 0:
            return None
        try:
            if self.slot.numel() < M:
                self.slot = torch.empty(M, dtype=torch.int32, device=self.device)
            if self.bins.numel() < over << DIGIT and over <= MAX_HOT:
                self.bins = torch.zeros(over << DIGIT, dtype=torch.int32, device=self.device)
            val = torch.empty(M, dtype=torch.int64, device=self.device)
            st = torch.empty(M, dtype=torch.int32, device=self.device)
            h.limit_cut(_ptr(actor), M, _ptr(self.demand), _ptr(self.hot_actor), _ptr(self.rem), _ptr(self.prefix),
                        _ptr(self.ctr), self.n, over, _ptr(self.slot), _ptr(self.bins), self.bins.numel(), _ptr(val),
                        _ptr(st), s)
        except BaseException:
            self._clear()  # (the hot slots of this Send must not outlive it: every bucket starts full again)
            raise
        return val, st

    def words(self) -> np.ndarray:
        self._ready()
        if not self._gpu():
            return super().words()
        return torch.cat([self.table, self.ctr[:COUNTERS]]).cpu().numpy().view(np.uint64)

    def at_rest(self) -> bool:
        """Whether the kernels left their workspace as a Send expects it: ``demand``,
        ``bins``, ``over`` and ``n_touched`` all zero (the tests ask after every Send)."""
        self._ready()
        if not self._gpu():
            return True
        return not (bool(self.demand.any()) or bool(self.bins.any()) or bool(self.ctr[C_OVER:C_TOUCHED + 1].any()))
