"""Circuit breaker (``DeviceRuntime.send(breaker=True)``): an actor that keeps failing
is not sent to for a while, across the Sends of one runtime.

What ``sony/gobreaker`` or Akka's ``CircuitBreaker`` put around a call, per actor and on
the batch path.  An actor whose messages failed ``threshold`` times in a row *opens*: for
``cooldown`` guarded Sends its messages are answered ``(0, STATUS_BREAKER_OPEN)`` and not
sent.  Then it is *half-open*: the lowest message of the batch that addresses it travels
as the probe, every other one is still rejected; a probe that answers ``STATUS_OK``
closes the actor, one that fails opens it for another ``cooldown`` Sends.

The key is the logical actor id as the caller wrote it (uint32), the method is not part
of it.  The table (``csrc/hip/breaker.hpp``) is dense, ``n`` words of 64 bits: ``open``
(bit 63), ``until`` (bits 32..62, a tick) and ``fails`` (bits 0..31, consecutive failed
messages, saturating); 0 is "closed, clean".  An id outside ``[0, n)`` is never guarded:
it always passes, is never observed and is counted in ``oob`` by an admit pass (a Send
with nothing open runs none).

Time is counted in guarded Sends: ``tick`` starts at 1, a guarded Send runs at ``now =
tick`` and then ``tick += 1``, even when the inner Send raises.  When the tick would pass
``2**31 - 1`` the breaker restarts (every word 0, tick 1).

Admission at ``now``: closed passes; open with ``now < until`` is rejected; open with
``now >= until`` passes only as the probe.  Observation of the admitted rows' final
replies, per actor: ``n_ok`` rows with ``STATUS_OK``, ``n_bad`` rows with a status in
``trip_on`` (other statuses count as neither), then for ``n_ok + n_bad > 0``:

* closed: any OK row resets ``fails`` to 0; otherwise ``fails = sat(fails + n_bad)``, and
  ``fails >= threshold`` opens the actor with ``until = now + cooldown``
* open: an OK row makes the word 0; else a bad row sets ``until = now + cooldown``

(``until`` is held at the last tick ``2**31 - 1``.)  The counters kept with the table:
``n_open`` (words with bit 63), ``n_dirty`` (non-zero words), ``trips`` (closed -> open),
``closes`` (open -> closed by a probe) and ``oob``.

CUDA tensors run the kernels (``csrc/hip/breaker.hip``); CPU tensors run ``BreakerRef``
(numpy), which is also what the kernels are tested against, word for word.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from . import retry as RT
from .batch import MsgBatch
from .records import PENDING, STATUS_BREAKER_OPEN, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NOT_DELIVERED, STATUS_OK

MAX_TICK = 2**31 - 1         # breaker.hpp kBreakerMaxTick
MAX_ACTORS = 1 << 28         # breaker.hpp kBreakerMaxActors
DEFAULT_TRIP_ON = (STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NOT_DELIVERED)
C_OPEN, C_DIRTY, C_TRIPS, C_CLOSES, C_OOB, C_TOUCHED = range(6)  # breaker.hpp BreakerCounter
COUNTERS = 5                 # the counters of the model (C_TOUCHED is the kernels' own)
CTR_WORDS = 8 + 33           # breaker.hpp kBreakerCtrWords
_U32 = 0xFFFFFFFF
_OPEN = np.uint64(1 << 63)
_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_u64 = np.uint64


def trip_mask(trip_on=DEFAULT_TRIP_ON) -> int:
    """The 32-bit mask of ``trip_on`` (bit s set: status s counts as a failure): any of
    the statuses 1..6."""
    if isinstance(trip_on, int):
        trip_on = (trip_on,)
    codes = [int(s) for s in trip_on]
    if not codes:
        raise ValueError("trip_on: at least one status")
    mask = 0
    for s in codes:
        if not 1 <= s <= 6:
            raise ValueError(f"trip_on: status {s} cannot trip a breaker (statuses 1..6)")
        mask |= 1 << s
    return mask


def is_open(w):
    return (np.asarray(w, dtype=np.uint64) >> _u64(63)) != 0


def until_of(w):
    return ((np.asarray(w, dtype=np.uint64) >> _u64(32)) & _u64(0x7FFFFFFF)).astype(np.int64)


def fails_of(w):
    return (np.asarray(w, dtype=np.uint64) & _u64(_U32)).astype(np.int64)


class BreakerRef:
    """The breaker on the host: ``table`` is ``uint64[n]`` in numpy, ``ctr`` the five
    counters.  ``_start=tick`` starts the tick elsewhere (the tests start it near the
    restart)."""

    def __init__(self, device="cpu", actors: int = 1024, threshold: int = 5, cooldown: int = 8, trip_on=None,
                 _start=None):
        self.device = torch.device(device)
        self.n, self.threshold, self.cooldown = int(actors), int(threshold), int(cooldown)
        if not 1 <= self.n <= MAX_ACTORS:
            raise ValueError("breaker: actors must be in [1, 2^28]")
        if not 1 <= self.threshold <= _U32:
            raise ValueError("breaker: threshold must be in [1, 2^32)")
        if not 1 <= self.cooldown <= MAX_TICK - 1:
            raise ValueError("breaker: cooldown must be in [1, 2^31 - 2]")
        self.trip_on = tuple(DEFAULT_TRIP_ON if trip_on is None else
                             ((trip_on,) if isinstance(trip_on, int) else trip_on))
        self.mask = trip_mask(self.trip_on)
        self.tick = 1 if _start is None else int(_start)
        if not 1 <= self.tick <= MAX_TICK + 1:
            raise ValueError("breaker: the tick must be in [1, 2^31]")
        self.table = None  # allocated and cleared by the first guarded Send
        # host counters: guarded Sends, their messages, the rejected ones, the ones sent on
        self.counters = {"sends": 0, "messages": 0, "rejected": 0, "sent": 0}

    # ---- the table operations (Breaker runs them on the device)
    def _clear(self) -> None:
        """Every word 0, every probe word all ones, ``n_open`` / ``n_dirty`` 0 (``trips``,
        ``closes`` and ``oob`` count on)."""
        if self.table is None:
            self.table = np.zeros(self.n, dtype=np.uint64)
            self.probe = np.empty(self.n, dtype=np.uint64)
            self.ctr = np.zeros(COUNTERS, dtype=np.uint64)
        self.table[:] = 0
        self.probe[:] = _ONES
        self.ctr[C_OPEN] = self.ctr[C_DIRTY] = 0

    def _ids(self, actor: torch.Tensor):
        a = actor.detach().cpu().contiguous().numpy().view(np.uint32).astype(np.int64)
        return a, a < self.n

    def _n_open(self) -> int:
        return int(self.ctr[C_OPEN])

    def _admit(self, batch: MsgBatch, now: int):
        M = batch.M
        a, inb = self._ids(batch.actor)
        w = self.table[np.where(inb, a, 0)]
        opened = inb & is_open(w)
        cand = opened & (now >= until_of(w))
        rows = np.flatnonzero(cand)
        claim = _u64((_U32 - now) << 32) | rows.astype(np.uint64)
        np.minimum.at(self.probe, a[rows], claim)
        won = self.probe[a[rows]] == claim
        st = np.full(M, PENDING, dtype=np.int32)
        st[opened] = STATUS_BREAKER_OPEN
        st[rows[won]] = PENDING
        self.ctr[C_OOB] += _u64(int((~inb).sum()))
        return torch.zeros(M, dtype=torch.int64), torch.from_numpy(st)

    def _observe(self, sub: MsgBatch, st: torch.Tensor, now: int) -> None:
        a, inb = self._ids(sub.actor)
        s = st.detach().cpu().numpy().astype(np.int64)
        bad = inb & (s >= 0) & (s < 32) & (((self.mask >> np.clip(s, 0, 31)) & 1) != 0)
        n_ok = np.bincount(a[inb & (s == STATUS_OK)], minlength=self.n)
        n_bad = np.bincount(a[bad], minlength=self.n)
        # an OK reply to a clean actor changes nothing: only failed rows and dirty actors are stepped
        t = np.flatnonzero((n_bad > 0) | ((n_ok > 0) & (self.table != 0)))
        if not t.size:
            return
        w = self.table[t]
        opened, ok, nb = is_open(w), n_ok[t] > 0, n_bad[t]
        until = _u64(min(now + self.cooldown, MAX_TICK))
        fails = np.minimum(fails_of(w) + nb, _U32).astype(np.uint64)
        trip = ~opened & ~ok & (fails >= _u64(self.threshold))
        closed_new = np.where(ok, _u64(0), np.where(trip, _OPEN | (until << _u64(32)) | fails, fails))
        reopened = _OPEN | (until << _u64(32)) | (w & _u64(_U32))
        open_new = np.where(ok, _u64(0), np.where(nb > 0, reopened, w))
        new = np.where(opened, open_new, closed_new).astype(np.uint64)
        self.table[t] = new
        c = self.ctr
        c[C_OPEN] = _u64(int(c[C_OPEN]) + int(is_open(new).sum()) - int(opened.sum()))
        c[C_DIRTY] = _u64(int(c[C_DIRTY]) + int((new != 0).sum()) - int((w != 0).sum()))
        c[C_TRIPS] += _u64(int(trip.sum()))
        c[C_CLOSES] += _u64(int((opened & ok).sum()))

    def words(self) -> np.ndarray:
        """The state table and the five counters (``n_open, n_dirty, trips, closes, oob``)
        as ``uint64[n + 5]`` on the host."""
        self._ready()
        return np.concatenate([self.table, self.ctr[:COUNTERS]])

    # ---- the breaker
    def _ready(self) -> None:
        if self.table is None:
            self._clear()

    def reset(self) -> None:
        """Close every actor (the tick goes on)."""
        if self.table is not None:
            self._clear()

    def begin(self) -> int:
        """Start a guarded Send: its tick (the breaker restarts first when the tick
        would pass ``2**31 - 1``)."""
        self._ready()
        if self.tick > MAX_TICK:
            self._clear()
            self.tick = 1
        return self.tick

    def end(self) -> None:
        self.tick += 1

    def admit(self, batch: MsgBatch):
        """``(val int64[M], st int32[M])`` at the current tick: ``st[i]`` is ``PENDING``
        for a row that travels (a marker no handler returns) and ``STATUS_BREAKER_OPEN``
        for a rejected one; ``val`` is 0."""
        self._ready()
        return self._admit(batch, self.tick)

    def observe(self, sub: MsgBatch, st: torch.Tensor) -> None:
        """The final statuses of the rows that travelled into the state words, at the
        current tick."""
        if st.numel() != sub.M:
            raise ValueError("observe: st must have one entry per row")
        self._ready()
        self._observe(sub, st, self.tick)

    def read(self) -> dict:
        """The counters kept with the table (one host read on a GPU)."""
        w = self.words()[self.n:]
        return {"open": int(w[C_OPEN]), "dirty": int(w[C_DIRTY]), "trips": int(w[C_TRIPS]),
                "closes": int(w[C_CLOSES]), "oob": int(w[C_OOB])}

    def send(self, batch: MsgBatch, send, collective: bool = False):
        """One guarded Send: reject the rows of open actors, compact the rest (stably, in
        message order), ``send(sub)`` them -- ``send`` takes a MsgBatch and returns
        ``(value, status, ...)``, final on return -- observe their replies and merge them
        with the rejections.  With nothing open (one host read) the batch goes to
        ``send`` untouched and is observed.  ``send`` is called at most once: exactly
        once when ``collective`` (a rank whose batch was all rejected joins with an empty
        batch), not at all for K == 0 otherwise."""
        M = batch.M
        c = self.counters
        c["sends"] += 1
        c["messages"] += M
        self.begin()
        try:
            if self._n_open() == 0:
                c["sent"] += M
                out = send(batch)
                self.observe(batch, out[1])
                return out
            val, st = self.admit(batch)
            return RT.send_pending(batch, val, st, send, collective, self._count,
                                   lambda sub, out: self.observe(sub, out[1]))
        finally:
            self.end()

    def _count(self, rejected: int, sent: int) -> None:
        self.counters["rejected"] += rejected
        self.counters["sent"] += sent


class Breaker(BreakerRef):
    """The breaker of one rank on ``device``: on a GPU the tables live in HBM (28 B per
    actor, allocated by the first guarded Send) and the kernels run on the current stream;
    on the CPU it is the host reference.

    One stream: the launch boundaries of one stream are the only ordering between the
    launches of a guarded Send and the next one's, and the tables outlive the Send.  Every
    call on one breaker must be issued on the same stream, or on streams the caller has
    ordered after one another; no event is recorded here."""

    def _gpu(self) -> bool:
        return self.device.type == "cuda"

    def _clear(self) -> None:
        if not self._gpu():
            return super()._clear()
        if self.table is None:
            new = (lambda dt: torch.empty(self.n, dtype=dt, device=self.device))
            self.table, self.obs, self.probe = new(torch.int64), new(torch.int64), new(torch.int64)
            self.touched = new(torch.int32)
            self.ctr = torch.zeros(CTR_WORDS, dtype=torch.int64, device=self.device)
        hip().breaker_clear(_ptr(self.table), _ptr(self.obs), _ptr(self.probe), _ptr(self.ctr), self.n,
                            raw_stream(self.device))

    def _n_open(self) -> int:
        if not self._gpu():
            return super()._n_open()
        return int(self.ctr[C_OPEN].item())  # the host read of a guarded Send

    def _admit(self, batch: MsgBatch, now: int):
        if not self._gpu():
            return super()._admit(batch, now)
        M = batch.M
        val = torch.empty(M, dtype=torch.int64, device=self.device)
        st = torch.empty(M, dtype=torch.int32, device=self.device)
        if M:
            if batch.actor.dtype != torch.int32:
                raise TypeError("MsgBatch: actor must be int32")
            actor = batch.actor.contiguous()
            hip().breaker_admit(_ptr(actor), M, _ptr(self.table), _ptr(self.probe), self.n, now, _ptr(self.ctr),
                                _ptr(val), _ptr(st), raw_stream(self.device))
        return val, st

    def _observe(self, sub: MsgBatch, st: torch.Tensor, now: int) -> None:
        if not self._gpu():
            return super()._observe(sub, st, now)
        K = sub.M
        if K == 0:
            return
        if sub.actor.dtype != torch.int32 or st.dtype != torch.int32:
            raise TypeError("observe: actor int32, st int32")
        actor, st = sub.actor.contiguous(), st.contiguous()
        hip().breaker_observe(_ptr(actor), _ptr(st), K, self.mask, _ptr(self.table), _ptr(self.obs),
                              _ptr(self.touched), _ptr(self.ctr), self.n, now, self.threshold, self.cooldown,
                              raw_stream(self.device))

    def words(self) -> np.ndarray:
        self._ready()
        if not self._gpu():
            return super().words()
        return torch.cat([self.table, self.ctr[:COUNTERS]]).cpu().numpy().view(np.uint64)
