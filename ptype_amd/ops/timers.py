"""Timer queue of a runtime: delayed messages kept on the device.

Akka has ``scheduler.scheduleOnce`` and actor timers, protoactor ``scheduler.SendOnce``,
SQS ``DelaySeconds``; a batched Send returns before the host has seen a row and ``batch``
belongs to the caller, so a message that is to travel later lives in HBM with its whole
call.  Time is explicit, as in the breaker and the limiter: the queue's clock counts
**ticks**, ``tick`` advances it by one, and there is no wall clock -- every word of the
queue is a function of the calls alone.

``schedule(batch, delay)`` files row ``i`` iff ``1 <= delay[i] <= horizon``; the other rows
are counted in ``refused``.  The K accepted rows form one **run**: they are stored sorted by
``(delay, row)`` -- a stable counting sort on the device, three launches
(``csrc/hip/timers.hip``) and one host read between the second and the third -- under the
tickets ``head .. head + K - 1``; record ``t`` lives in slot ``t % entries``.  A run has a
descriptor in the run table (run ``q`` in slot ``q % runs``) with ``off[d]``, the number of its
records with a delay below ``d``: the records due ``d`` ticks after the Schedule are the
tickets ``[base + off[d], base + off[d + 1])``.  A call without an accepted row files no run.
The whole call is refused with ``TimerQueueFull``, before a word of the queue is written,
when the ring lacks room (``head + K - tail > entries``) or, for K > 0, the run table is
full (``runs_head - runs_tail == runs``).

``tick()`` is ``now += 1``; the due records of every live run, in run order -- which is
ticket order -- are taken into SoA columns (``Timers``).  A run is finished once
``now >= t0 + max_delay``; ``runs_tail`` moves over the leading finished runs and ``tail``
becomes the base of the run it stops at (``head`` without one).  A long-delay run at the
tail therefore holds the ring space of the finished runs behind it; the ring is not
compacted.

Record (u64 words, little-endian; layout: ``csrc/hip/timers.hpp``, mirrored below):

====  =====================================================================
w0    ticket + 1 (0: never written)
w1    due tick
w2    row ``u32`` | delay ``u32`` << 32
w3    logical actor id ``u32`` | method ``u16`` << 32
w4    a0
w5    a1 (0 when the batch has no such column)
w6    a2 (alike)
w7    tag
====  =====================================================================

Run descriptor: a 64-byte header ``t0, base, n, max_delay, seq`` (``seq`` is ``q + 1``) and
``off[horizon + 2]`` ``u32``, padded to 64 bytes.  Control line: ``now, head, tail, runs_head,
runs_tail, refused, delivered, torn``.  The scratch line (``k, refused, max_delay, head,
runs_head, now, n_due, segs``; ``refused`` is the control word as it is after the call) is what
the kernels hand to the host and to each other and no part of the queue's state: a refused
Schedule has written its first six words.

The queue is the caller's view, like the ledger and the dead-letter queue: a rank files
what it scheduled.  CPU tensors run the numpy model (``TimerRef``), which is also what the
kernels are tested against, word for word.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from .batch import MsgBatch

# csrc/hip/timers.hpp (checked against _hip.timer_layout() by the GPU tests)
RECORD_WORDS, HEADER_WORDS, CTRL_WORDS, SCRATCH_WORDS = 8, 8, 8, 8
W_TICKET, W_DUE, W_ROW_DELAY, W_ACTOR_METHOD, W_A0, W_A1, W_A2, W_TAG = range(8)
D_T0, D_BASE, D_N, D_MAX_DELAY, D_SEQ = range(5)
C_NOW, C_HEAD, C_TAIL, C_RUNS_HEAD, C_RUNS_TAIL, C_REFUSED, C_DELIVERED, C_TORN = range(8)
S_K, S_REFUSED, S_MAX_DELAY, S_HEAD, S_RUNS_HEAD, S_NOW, S_DUE, S_SEGS = range(8)
TILE = 4096  # rows per block (compact.hpp kCompactTile)
MIN_ENTRIES, MAX_ENTRIES = 64, 1 << 24
MIN_HORIZON, MAX_HORIZON = 16, 1024
MIN_RUNS, MAX_RUNS = 4, 4096
DEFAULT_ENTRIES, DEFAULT_HORIZON, DEFAULT_RUNS = 1 << 20, 256, 256
_U64 = (1 << 64) - 1
COLUMNS = ("ticket", "row", "actor", "method", "delay", "t0", "a0", "a1", "a2", "tag")
_DTYPES = {"ticket": torch.int64, "row": torch.int32, "actor": torch.int32, "method": torch.int16,
           "delay": torch.int32, "t0": torch.int64, "a0": torch.int64, "a1": torch.int64, "a2": torch.int64,
           "tag": torch.int64}


class TimerQueueFull(RuntimeError):
    """A Schedule the ring or the run table had no room for; nothing of it was filed."""


def _pow2_in(name: str, v: int, lo: int, hi: int, text: str) -> int:
    v = int(v)
    if not lo <= v <= hi or v & (v - 1):
        raise ValueError(f"{name}: a power of two in {text}")
    return v


def check_entries(entries: int) -> int:
    return _pow2_in("timer_entries", entries, MIN_ENTRIES, MAX_ENTRIES, "[64, 2^24]")


def check_horizon(horizon: int) -> int:
    return _pow2_in("timer_horizon", horizon, MIN_HORIZON, MAX_HORIZON, "[16, 1024]")


def check_runs(runs: int) -> int:
    return _pow2_in("timer_runs", runs, MIN_RUNS, MAX_RUNS, "[4, 4096]")


def desc_words(horizon: int) -> int:
    """u64 words of one run descriptor: the header and ``off[horizon + 2]`` u32 padded to 64 B."""
    return HEADER_WORDS + (horizon + 2 + 15) // 16 * 8


def _validate(batch: MsgBatch, delay) -> None:
    M = batch.M
    if batch.actor.dtype != torch.int32 or batch.a0.dtype != torch.int64 or batch.a0.numel() != M:
        raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    for t in (batch.a1, batch.a2):
        if t is not None and (t.dtype != torch.int64 or t.numel() != M):
            raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    if not isinstance(batch.method, int) and batch.method.numel() != M:
        raise TypeError("MsgBatch: the method column must have M entries")
    if isinstance(delay, torch.Tensor):
        if delay.dtype != torch.int32 or delay.dim() != 1 or delay.numel() != M:
            raise TypeError("schedule: delay must be an int or an int32[M] column")
        if delay.device != batch.actor.device:
            raise ValueError("schedule: the delay column lives on another device than the batch")
    elif isinstance(delay, bool) or not isinstance(delay, (int, np.integer)):
        raise TypeError("schedule: delay must be an int or an int32[M] column")


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy()


def _i64(x: int) -> int:
    x &= _U64
    return x - (1 << 64) if x >> 63 else x


@dataclass
class Scheduled:
    """What a Schedule did: ``n`` rows filed under the tickets ``first_ticket ..
    first_ticket + n - 1`` (sorted by ``(delay, row)``), ``refused`` rows whose delay was
    outside ``[1, horizon]``, and the clock ``now`` the delays count from."""

    n: int
    refused: int
    first_ticket: int
    now: int


@dataclass
class Timers:
    """What a tick took out of the ring: the ``n`` due records as SoA columns on the queue's
    device, in ticket order (``ticket`` / ``t0`` / ``a0`` / ``a1`` / ``a2`` / ``tag`` int64; ``row`` /
    ``actor`` / ``delay`` int32; ``method`` int16; ``t0``: the clock at the Schedule), and
    ``torn``: slots whose ticket word was not the expected one (0).  On the device the tick
    does not wait for its take launch: ``torn`` is read from the control line when it is first
    asked for (a host read then, of the mismatches counted since this tick's own read)."""

    n: int
    torn_source: object  # an int, or a function that reads it
    ticket: torch.Tensor
    row: torch.Tensor
    actor: torch.Tensor
    method: torch.Tensor
    delay: torch.Tensor
    t0: torch.Tensor
    a0: torch.Tensor
    a1: torch.Tensor
    a2: torch.Tensor
    tag: torch.Tensor

    @property
    def torn(self) -> int:
        if callable(self.torn_source):
            self.torn_source = int(self.torn_source())
        return self.torn_source

    def batch(self) -> MsgBatch:
        """The records as the calls they were: logical actor ids, a method column."""
        return MsgBatch(self.actor, self.a0, self.a1, self.a2, self.method)


@dataclass
class Ticked:
    """What ``DeviceRuntime.tick`` did: the ``due`` records it took and their Send's
    ``(value, status)``, row for row."""

    due: Timers
    value: torch.Tensor
    status: torch.Tensor

    @property
    def n(self) -> int:
        return self.due.n


def _counters(ctrl, entries: int, horizon: int, runs: int, full: int) -> dict:
    c = [int(x) & _U64 for x in ctrl]
    return {"now": c[C_NOW], "head": c[C_HEAD], "tail": c[C_TAIL], "live": c[C_HEAD] - c[C_DELIVERED],
            "runs": c[C_RUNS_HEAD] - c[C_RUNS_TAIL], "refused": c[C_REFUSED], "delivered": c[C_DELIVERED],
            "full": full, "torn": c[C_TORN], "entries": entries, "horizon": horizon, "max_runs": runs}


class TimerRef:
    """The numpy model: ``ring`` uint64[entries, 8], ``runs`` uint64[runs, desc_words],
    ``ctrl`` uint64[8] and ``scratch`` uint64[8], word for word what the kernels leave in HBM."""

    def __init__(self, entries: int = DEFAULT_ENTRIES, horizon: int = DEFAULT_HORIZON, runs: int = DEFAULT_RUNS):
        self.entries, self.horizon, self.n_runs = check_entries(entries), check_horizon(horizon), check_runs(runs)
        self.ring = np.zeros((self.entries, RECORD_WORDS), dtype=np.uint64)
        self.runs = np.zeros((self.n_runs, desc_words(self.horizon)), dtype=np.uint64)
        self.ctrl = np.zeros(CTRL_WORDS, dtype=np.uint64)
        self.scratch = np.zeros(SCRATCH_WORDS, dtype=np.uint64)
        self.full = 0

    def off(self, slot: int) -> np.ndarray:
        """``off[0 .. horizon + 1]`` of the descriptor in ``slot``."""
        return self.runs[slot, HEADER_WORDS:].view(np.uint32)[:self.horizon + 2]

    def schedule(self, batch: MsgBatch, delay, tag: int = 0) -> Scheduled:
        _validate(batch, delay)
        M, E, H, R = batch.M, self.entries, self.horizon, self.n_runs
        if isinstance(delay, torch.Tensor):
            d = _np(delay).astype(np.int64)
        else:  # (any int: one outside the horizon refuses every row)
            d = np.full(M, int(delay) if 1 <= int(delay) <= H else 0, dtype=np.int64)
        rows = np.nonzero((d >= 1) & (d <= H))[0]
        dl = d[rows]
        order = np.argsort(dl, kind="stable")
        rows, dl = rows[order], dl[order]
        K = int(rows.size)
        now, head, tail = int(self.ctrl[C_NOW]), int(self.ctrl[C_HEAD]), int(self.ctrl[C_TAIL])
        rh, rt = int(self.ctrl[C_RUNS_HEAD]), int(self.ctrl[C_RUNS_TAIL])
        max_delay = int(dl[-1]) if K else 0
        self.scratch[[S_K, S_REFUSED, S_MAX_DELAY, S_HEAD, S_RUNS_HEAD, S_NOW]] = [
            K, int(self.ctrl[C_REFUSED]) + M - K, max_delay, head, rh, now]
        if head + K - tail > E or (K and rh - rt == R):
            self.full += 1
            raise TimerQueueFull(f"schedule: no room for {K} records (ring {head - tail} of {E}, runs {rh - rt} of {R})")
        if K:
            u32 = (lambda a: a.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))
            if isinstance(batch.method, int):
                m = np.full(K, int(batch.method) & 0xFFFF, dtype=np.uint64)
            else:
                m = _np(batch.method.to(torch.int16))[rows].astype(np.int64).astype(np.uint64) & np.uint64(0xFFFF)
            col = (lambda t: np.zeros(K, dtype=np.uint64) if t is None else _np(t)[rows].view(np.uint64))
            ticket = np.uint64(head) + np.arange(K, dtype=np.uint64)
            rec = np.empty((K, RECORD_WORDS), dtype=np.uint64)
            rec[:, W_TICKET] = ticket + np.uint64(1)
            rec[:, W_DUE] = np.uint64(now) + dl.astype(np.uint64)
            rec[:, W_ROW_DELAY] = rows.astype(np.uint64) | (dl.astype(np.uint64) << np.uint64(32))
            rec[:, W_ACTOR_METHOD] = u32(_np(batch.actor)[rows]) | (m << np.uint64(32))
            rec[:, W_A0], rec[:, W_A1], rec[:, W_A2] = col(batch.a0), col(batch.a1), col(batch.a2)
            rec[:, W_TAG] = int(tag) & _U64
            self.ring[(ticket & np.uint64(E - 1)).astype(np.int64)] = rec
            slot = rh & (R - 1)
            self.runs[slot, [D_T0, D_BASE, D_N, D_MAX_DELAY, D_SEQ]] = [now, head, K, max_delay, rh + 1]
            # off[j]: the records with a delay below j
            self.off(slot)[:] = np.concatenate([[0], np.cumsum(np.bincount(dl, minlength=H + 1)[:H + 1])])
            self.ctrl[C_HEAD], self.ctrl[C_RUNS_HEAD] = head + K, rh + 1
        self.ctrl[C_REFUSED] = self.scratch[S_REFUSED]
        return Scheduled(K, M - K, head, now)

    def _segments(self, now: int):
        """``(first ticket, length)`` of every live run's records due at ``now``, in run order."""
        R, H = self.n_runs, self.horizon
        segs = []
        for q in range(int(self.ctrl[C_RUNS_TAIL]), int(self.ctrl[C_RUNS_HEAD])):
            slot = q & (R - 1)
            d = now - int(self.runs[slot, D_T0])
            off = self.off(slot)
            base = int(self.runs[slot, D_BASE])
            segs.append((base + int(off[d]), int(off[d + 1]) - int(off[d])) if 1 <= d <= H else (base, 0))
        return segs

    def peek(self) -> int:
        """The number of records the next tick will take; no control word changes."""
        segs = self._segments(int(self.ctrl[C_NOW]) + 1)
        self.scratch[S_DUE], self.scratch[S_SEGS] = sum(n for _, n in segs), len(segs)
        return int(self.scratch[S_DUE])

    def tick(self) -> dict:
        """``now += 1``; ``{"n", "torn", column: numpy array}`` of the due records."""
        R, E = self.n_runs, self.entries
        now = int(self.ctrl[C_NOW]) + 1
        segs = self._segments(now)
        n = sum(k for _, k in segs)
        self.scratch[S_DUE], self.scratch[S_SEGS] = n, len(segs)
        rh, rt = int(self.ctrl[C_RUNS_HEAD]), int(self.ctrl[C_RUNS_TAIL])
        while rt < rh and now >= int(self.runs[rt & (R - 1), D_T0]) + int(self.runs[rt & (R - 1), D_MAX_DELAY]):
            rt += 1
        self.ctrl[C_NOW], self.ctrl[C_RUNS_TAIL] = now, rt
        self.ctrl[C_DELIVERED] += np.uint64(n)
        self.ctrl[C_TAIL] = self.runs[rt & (R - 1), D_BASE] if rt < rh else self.ctrl[C_HEAD]
        t = (np.concatenate([np.arange(s, s + k, dtype=np.uint64) for s, k in segs]) if segs
             else np.zeros(0, dtype=np.uint64))
        rec = self.ring[(t & np.uint64(E - 1)).astype(np.int64)]
        torn = int((rec[:, W_TICKET] != t + np.uint64(1)).sum())
        self.ctrl[C_TORN] += np.uint64(torn)
        w2, w3 = rec[:, W_ROW_DELAY], rec[:, W_ACTOR_METHOD]
        lo32 = (lambda w: (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32))
        return {"n": n, "torn": torn, "ticket": t.view(np.int64), "row": lo32(w2), "actor": lo32(w3),
                "method": ((w3 >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16),
                "delay": lo32(w2 >> np.uint64(32)), "t0": (rec[:, W_DUE] - (w2 >> np.uint64(32))).view(np.int64),
                "a0": rec[:, W_A0].view(np.int64), "a1": rec[:, W_A1].view(np.int64),
                "a2": rec[:, W_A2].view(np.int64), "tag": rec[:, W_TAG].view(np.int64)}

    def read(self) -> dict:
        return _counters(self.ctrl, self.entries, self.horizon, self.n_runs, self.full)

    def reset(self, ring: bool = True) -> None:
        for a in (self.ring, self.runs) * ring + (self.ctrl, self.scratch):
            a[:] = 0
        self.full = 0


class TimerQueue:
    """The timer queue of one rank, on ``device``.  ``max_rows``: the largest Schedule it
    will file without growing its histogram workspace (``horizon + 1`` u32 per 4096 rows).
    Schedule and tick read the control and the scratch line on the host, so neither is
    legal under graph capture.  The ring, the run table, the lines and the workspace are
    state that outlives a call, and the order of the launches on the stream is their only
    protection: every ``schedule``, ``tick`` and ``reset`` of a queue must be issued on the
    same stream (or on streams the caller orders after one another)."""

    def __init__(self, device, entries: int = DEFAULT_ENTRIES, horizon: int = DEFAULT_HORIZON,
                 runs: int = DEFAULT_RUNS, max_rows: int = 0):
        self.device = torch.device(device)
        self.entries, self.horizon, self.n_runs = check_entries(entries), check_horizon(horizon), check_runs(runs)
        self.ref = None
        self.full = 0
        if self.device.type != "cuda":
            self.ref = TimerRef(self.entries, self.horizon, self.n_runs)
            return
        z = (lambda *shape, dtype=torch.int64: torch.zeros(*shape, dtype=dtype, device=self.device))
        self.ring = z(self.entries, RECORD_WORDS)
        self.device = self.ring.device  # ("cuda" names the current device: what the tensors report)
        self.runs = z(self.n_runs, desc_words(self.horizon))
        self._lines = z(CTRL_WORDS + SCRATCH_WORDS)  # one host read fetches both
        self.ctrl, self.scratch = self._lines[:CTRL_WORDS], self._lines[CTRL_WORDS:]
        self._off = z(self.horizon + 2, dtype=torch.int32)
        self._seg_first = z(self.n_runs + 1, dtype=torch.int32)
        self._seg_ticket = z(self.n_runs)
        self._hist = z(max(1, (int(max_rows) + TILE - 1) // TILE) * (self.horizon + 1), dtype=torch.int32)

    def _lines_host(self) -> tuple[list[int], list[int]]:
        w = [int(x) & _U64 for x in self._lines.cpu().tolist()]  # (a host read)
        return w[:CTRL_WORDS], w[CTRL_WORDS:]

    def _no_capture(self, what: str) -> None:
        if self.ref is None and torch.cuda.is_current_stream_capturing():
            raise ValueError(f"timers: {what} reads the queue's lines on the host; not under graph capture")

    def schedule(self, batch: MsgBatch, delay, tag: int = 0) -> Scheduled:
        """File the rows of ``batch`` -- under the ids its caller wrote -- whose ``delay`` (an
        int, or an int32[M] column on the batch's device) is in ``[1, horizon]``, to be taken
        by the tick ``delay`` ticks from now.  Raises ``TimerQueueFull``, with nothing filed,
        when the ring or the run table lacks room."""
        _validate(batch, delay)
        if batch.actor.device != self.device:
            raise ValueError("timers: the batch's tensors live on another device than the queue")
        if self.ref is not None:
            try:
                return self.ref.schedule(batch, delay, tag)
            finally:
                self.full = self.ref.full
        self._no_capture("schedule")
        M, H = batch.M, self.horizon
        column = isinstance(delay, torch.Tensor)
        tiles = max(1, (M + TILE - 1) // TILE)
        if column and tiles * (H + 1) > self._hist.numel():
            self._hist = torch.empty(max(tiles * (H + 1), 2 * self._hist.numel()), dtype=torch.int32,
                                     device=self.device)
        c = (lambda t: None if t is None else t.contiguous())
        # (a view at an odd element offset stays a view: the count reads it with scalar loads)
        dcol = c(delay) if column else None
        uniform = 0 if column else max(-1, min(int(delay), 1 << 31))  # (outside the horizon: refused either way)
        stream = raw_stream(self.device)
        hip().timer_count(_ptr(dcol), uniform, M, _ptr(self.ctrl), _ptr(self.scratch), H, _ptr(self._hist),
                          self._hist.numel(), _ptr(self._off), stream)
        w, s = self._lines_host()
        K = s[S_K]
        if w[C_HEAD] + K - w[C_TAIL] > self.entries or (K and w[C_RUNS_HEAD] - w[C_RUNS_TAIL] == self.n_runs):
            self.full += 1
            raise TimerQueueFull(f"schedule: no room for {K} records (ring {w[C_HEAD] - w[C_TAIL]} of {self.entries}, "
                                 f"runs {w[C_RUNS_HEAD] - w[C_RUNS_TAIL]} of {self.n_runs})")
        uniform_method = isinstance(batch.method, int)
        method = None if uniform_method else c(batch.method.to(torch.int16))
        hip().timer_file(_ptr(dcol), uniform, M, _ptr(c(batch.actor)), _ptr(method),
                         int(batch.method) & 0xFFFF if uniform_method else 0, _ptr(c(batch.a0)), _ptr(c(batch.a1)),
                         _ptr(c(batch.a2)), _i64(int(tag)), _ptr(self.ring), _ptr(self.runs), _ptr(self.ctrl),
                         _ptr(self.scratch), self.entries, H, self.n_runs, _ptr(self._hist), self._hist.numel(),
                         _ptr(self._off), stream)
        return Scheduled(K, M - K, w[C_HEAD], w[C_NOW])

    def peek(self) -> int:
        """The number of records the next tick will take (a host read); nothing moves."""
        if self.ref is not None:
            return self.ref.peek()
        self._no_capture("peek")
        hip().timer_due(_ptr(self.runs), _ptr(self.ctrl), _ptr(self.scratch), self.horizon, self.n_runs,
                        _ptr(self._seg_first), _ptr(self._seg_ticket), False, raw_stream(self.device))
        return self._lines_host()[1][S_DUE]

    def tick(self) -> Timers:
        """``now += 1`` and the records that are due, in ticket order, as SoA columns; they
        have left the queue.  Reads ``n_due`` on the host (one read of the lines) and does not
        wait for the take launch; the result's ``torn`` reads the control line when asked for."""
        if self.ref is not None:
            r = self.ref.tick()
            return Timers(r["n"], r["torn"], **{k: torch.from_numpy(np.ascontiguousarray(r[k])) for k in COLUMNS})
        self._no_capture("tick")
        stream = raw_stream(self.device)
        hip().timer_due(_ptr(self.runs), _ptr(self.ctrl), _ptr(self.scratch), self.horizon, self.n_runs,
                        _ptr(self._seg_first), _ptr(self._seg_ticket), True, stream)
        w, s = self._lines_host()
        n = s[S_DUE]
        cols = {k: torch.empty(n, dtype=_DTYPES[k], device=self.device) for k in COLUMNS}
        if n == 0:
            return Timers(0, 0, **cols)
        hip().timer_take(_ptr(self.ring), _ptr(self.ctrl), self.entries, _ptr(self._seg_first),
                         _ptr(self._seg_ticket), s[S_SEGS], self.n_runs, n, *(_ptr(cols[k]) for k in COLUMNS), stream)
        ctrl, before = self.ctrl, w[C_TORN]
        return Timers(n, lambda: (int(ctrl[C_TORN].item()) & _U64) - before, **cols)

    def read(self) -> dict:
        """The counters (a host read): ``now``, ``head``, ``tail``, ``live`` (records filed and not
        yet due), ``runs`` (pending), ``refused``, ``delivered``, ``full`` (Schedules refused with
        ``TimerQueueFull``), ``torn``, and the sizes ``entries``, ``horizon``, ``max_runs``."""
        if self.ref is not None:
            return self.ref.read()
        return _counters(self._lines_host()[0], self.entries, self.horizon, self.n_runs, self.full)

    def reset(self, ring: bool = True) -> None:
        """Empty the queue, set the clock to 0 and zero every counter (asynchronous fills).
        Without ``ring`` only the two lines are zeroed -- the queue is as empty, the ring and
        the run table keep stale words nothing will read -- which spares the fill of a ring
        of up to 1 GiB."""
        self.full = 0
        if self.ref is not None:
            self.ref.reset(ring)
            return
        if ring:
            self.ring.zero_()
            self.runs.zero_()
        self._lines.zero_()
