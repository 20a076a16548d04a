#!/usr/bin/env python3
"""What the timer queue (ops/timers.py, csrc/hip/timers.hip) costs.

Schedule and Tick at each ``--msgs`` size with ``--horizon`` 256, for delays drawn uniformly
from ``[1, horizon]`` (a delay column) and for one single delay (an int, and the same as a
column: the histogram's worst case, every row of a tile in one bin), against the torch
sequence a caller writes without the feature on the same device:

* Schedule: ``torch.sort(delay, stable=True)`` and an ``index_select`` of the five columns
  (actor, method, a0, a1, a2) by the sort's indices -- the batch kept sorted by delay;
* Tick: two ``searchsorted`` on the sorted delays, their results read on the host, and a copy
  of the due slice of every column (the kept batch is sorted, so what is due is a slice).

Both Schedules read on the host (ours K and the control line, between its second and third
launch; torch's reads nothing), both Ticks read their count on the host, so everything is
timed with the host clock around the call and a device synchronise, the two sides alternating
in one process.  Before anything is timed the due rows of every tick are compared for exact
equality, column by column.

    python tools/timers_cost.py [--msgs 65536 1048576 8388608] [--iters 10] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import timers as TM  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402

ACTORS = 1 << 20
GATHERED = 4 + 4 + 2 + 8 + 8 + 8  # delay, actor, method, a0, a1, a2 of one row
TAKEN = 8 + 4 + 4 + 2 + 4 + 8 + 8 + 8 + 8 + 8  # the ten columns a tick writes per record
TICKS_TIMED = 8


def stat(ts) -> str:
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


class TorchTimers:
    """The batch kept sorted by delay with torch ops; a tick is a slice."""

    def schedule(self, b: MsgBatch, delay: torch.Tensor) -> None:
        self.delay, idx = torch.sort(delay, stable=True)
        self.row = idx
        self.cols = [c.index_select(0, idx) for c in (b.actor, b.method, b.a0, b.a1, b.a2)]
        self.now = 0

    def tick(self):
        self.now += 1
        lo, hi = torch.searchsorted(self.delay, torch.tensor([self.now, self.now + 1], dtype=torch.int32,
                                                             device=self.delay.device)).tolist()  # (a host read)
        return [self.row[lo:hi]] + [c[lo:hi].clone() for c in self.cols]


def empty(q: TM.TimerQueue) -> None:
    """The queue as new, without the fill of a ring of up to 1 GiB: the lines alone."""
    q.reset(ring=False)


def same_or_die(due: TM.Timers, want, what: str) -> None:
    got = [due.row.to(torch.int64), due.actor, due.method, due.a0, due.a1, due.a2]
    for name, g, w in zip(("row", "actor", "method", "a0", "a1", "a2"), got, want):
        if not torch.equal(g, w):
            raise RuntimeError(f"timers_cost: {what}: {name} of the due rows differs from the torch sequence's")
    if due.torn:
        raise RuntimeError(f"timers_cost: {what}: torn records")


def rows(M: int, H: int, iters: int, floor_tbs: float, dev) -> list[str]:
    gen = torch.Generator().manual_seed(M & 0xFFFF)
    big = (lambda: torch.randint(-2**62, 2**62, (M,), generator=gen).to(dev))
    b = MsgBatch(torch.randint(0, ACTORS, (M,), generator=gen).to(torch.int32).to(dev), big(), big(), big(),
                 torch.randint(0, 8, (M,), generator=gen).to(torch.int16).to(dev))
    entries = max(64, 1 << (M - 1).bit_length())
    q, t = TM.TimerQueue(dev, entries, H, 4, max_rows=M), TorchTimers()
    out = []
    for kind in ("uniform random", "one delay", "one delay (column)"):
        single = 7
        column = (torch.randint(1, H + 1, (M,), generator=gen) if kind == "uniform random"
                  else torch.full((M,), single)).to(torch.int32).to(dev)
        delay = single if kind == "one delay" else column
        first = 1 if kind == "uniform random" else single  # the first tick with anything due
        # equality first: every tick of the horizon (one delay: up to its tick)
        empty(q)
        q.schedule(b, delay)
        t.schedule(b, column)
        n = 0
        for k in range(H if kind == "uniform random" else single):
            due = q.tick()
            same_or_die(due, t.tick(), f"M={M} {kind} tick {k + 1}")
            n += due.n
        if n != M:
            raise RuntimeError(f"timers_cost: M={M} {kind}: {n} rows were due, not {M}")
        ts = {"sched": [], "torch sched": [], "tick": [], "torch tick": []}
        per_tick = 0
        for it in range(iters + 2):
            empty(q)
            a = timed(lambda: q.schedule(b, delay))
            o = timed(lambda: t.schedule(b, column))
            for _ in range(first - 1):
                q.tick()
                t.tick()
            ticks = TICKS_TIMED if kind == "uniform random" else 1
            ta, to, per_tick = [], [], 0
            for _ in range(ticks):
                ta.append(timed(lambda: q.tick()))
                to.append(timed(lambda: t.tick()))
            per_tick = (q.read()["delivered"]) // ticks
            if it >= 2:
                ts["sched"].append(a)
                ts["torch sched"].append(o)
                ts["tick"].append(statistics.median(ta))
                ts["torch tick"].append(statistics.median(to))
        med = {k: statistics.median(v) for k, v in ts.items()}
        s_bytes = M * (GATHERED - 4 + 64) if kind == "one delay" else M * (4 + GATHERED + 64)
        t_bytes = per_tick * (64 + TAKEN)
        out.append(f"| {M} | {kind} | {stat(ts['sched'])} | {stat(ts['torch sched'])} | "
                   f"{med['sched'] / med['torch sched']:.2f} | {s_bytes / (floor_tbs * 1e12) * 1e6:.1f} | {per_tick} | "
                   f"{stat(ts['tick'])} | {stat(ts['torch tick'])} | {med['tick'] / med['torch tick']:.2f} | "
                   f"{t_bytes / (floor_tbs * 1e12) * 1e6:.2f} |")
    del q, t
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="*", default=[1 << 16, 1 << 20, 8 << 20])
    ap.add_argument("--horizon", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--floor-tbs", type=float, default=4.0)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("timers_cost: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = []

    def emit(new):  # printed section by section: a failure later keeps what was measured
        print("\n".join(new), flush=True)
        lines.extend(new)
        if a.md:
            os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
            with open(a.md, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(["# Timer queue: what Schedule and Tick cost", "",
          f"Measured with `python tools/timers_cost.py` (horizon {a.horizon}, a ring of the next power of two at or above "
          "M, a1 / a2 and an int16 method column present).  Sides: `TimerQueue.schedule` (count, scan, one host read of "
          "the two lines, file; an int delay skips the count; `one delay (column)` is the same delay in every row of a "
          "column) and `TimerQueue.tick` (due, one host read, take; "
          "`csrc/hip/timers.hip`) against the torch sequence a caller writes without the feature: for Schedule "
          "`torch.sort(delay, stable=True)` and an `index_select` of the five columns, which reads nothing on the host; "
          "for Tick two `searchsorted` on the kept sorted delays, read on the host, and a copy of the due slice of the "
          "five columns.  The due rows of every tick of both sides are compared for exact equality before anything is "
          "timed.", "",
          f"One MI355X, profiler off.  Host clock around each call and a device synchronise, {a.iters} rounds per side "
          "after 2 warm-up rounds, the two sides alternating in one process; the queue is emptied (its two lines "
          f"zeroed) before every Schedule.  Tick: the median of the first {TICKS_TIMED} ticks of a round for random "
          "delays (M / horizon rows each), the one tick that takes all M rows for one delay.  Cells: median "
          "(min .. max) in us.", "",
          f"Bytes the kernels move per row: Schedule reads the delay twice with a column (count and file) and "
          f"{GATHERED - 4} B of the other columns and stores 64 B: {4 + GATHERED + 64} B with a delay column, "
          f"{GATHERED - 4 + 64} B with an int delay; the per-tile histograms add (horizon + 1) x 4 B per 4096 rows, "
          f"written once and read twice.  Tick reads 64 B and stores {TAKEN} B per due row: {64 + TAKEN} B.  The torch "
          f"Schedule moves at least 4 + 12 B per row in the sort (more in its radix passes) and 8 + 2 x width per column "
          f"gathered: at least {16 + 5 * 8 + 2 * (GATHERED - 4)} B; its Tick copies {GATHERED - 4} B per due row twice "
          f"(read and write).  The floor columns are the kernels' bytes at {a.floor_tbs} TB/s.", "",
          "| M | delays | schedule us | torch sort + index_select us | schedule / torch | schedule floor us | rows per "
          "tick | tick us | torch tick us | tick / torch | tick floor us |",
          "|---|---|---|---|---|---|---|---|---|---|---|"])
    for M in a.msgs:
        emit(rows(M, a.horizon, a.iters, a.floor_tbs, dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
