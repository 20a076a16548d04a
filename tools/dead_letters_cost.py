#!/usr/bin/env python3
"""What the dead-letter queue (ops/dead_letters.py, csrc/hip/dead_letters.hip) costs.

1.  The append alone (both launches) at each ``--msgs`` size and each ``--shares`` share of
    failed rows, on a ring of ``--entries`` records, against
    (b) the torch sequence a caller writes without it: ``nonzero`` on the status mask (a
        host wait for K), ``index_select`` per column, then an indexed copy into ring
        columns (SoA, slot = ticket mod entries; of K > entries rows the last ``entries``);
    (c) the byte floor: 4 B of status per row, plus per written letter 64 B stored and
        34 B gathered (status, actor, method, a0, a1, a2), at ``--floor-tbs`` TB/s (the
        README's streaming rate of the ring-order drain).
    The sides alternate inside one process, device events around ``--reps`` calls; both
    sides start from an empty ring and their rings are compared for exact equality, field
    by field, before anything is timed.
2.  What ``dead_letter=True`` adds to a world-1 Send (eager ``send_all``, host clock
    around the Send plus a device synchronise, the two variants alternating), with no
    failed row and with one unknown actor in a thousand.

    python tools/dead_letters_cost.py [--msgs 1048576 8388608] [--iters 10] [--reps 10] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import dead_letters as DL  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK  # noqa: E402
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402

ACTORS = 1 << 20
GATHERED = 4 + 4 + 2 + 8 + 8 + 8  # status, actor, method, a0, a1, a2 of one letter


def stat(ts) -> str:
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def alternate_events(variants, iters: int, reps: int) -> dict:
    """us per call of every variant: device events around ``reps`` calls, the variants
    alternating, ``iters`` groups each after two warm-up rounds."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {name: [] for name, _ in variants}
    for it in range(iters + 2):
        for name, fn in variants:
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            if it >= 2:
                ts[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return ts


def alternate_host(variants, iters: int) -> dict:
    ts = {name: [] for name, _ in variants}
    for it in range(iters + 3):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 3:
                ts[name].append((time.perf_counter() - t0) * 1e6)
    return ts


class TorchRing:
    """(b): the ring as SoA columns, filled with torch ops."""

    FIELDS = ("row", "status", "actor", "method", "a0", "a1", "a2")

    def __init__(self, entries: int, dev):
        self.E, self.head = entries, 0
        z = (lambda dt: torch.zeros(entries, dtype=dt, device=dev))
        self.ticket = z(torch.int64)
        self.cols = {"row": z(torch.int64), "status": z(torch.int32), "actor": z(torch.int32), "method": z(torch.int16),
                     "a0": z(torch.int64), "a1": z(torch.int64), "a2": z(torch.int64)}

    def append(self, b: MsgBatch, st: torch.Tensor) -> None:
        idx = torch.nonzero((st >= 1) & (st <= 6)).flatten()  # (the host waits for K here)
        K = int(idx.numel())
        first = max(0, K - self.E)
        idx = idx[first:]
        t = self.head + first + torch.arange(idx.numel(), device=st.device)
        slot = t & (self.E - 1)
        src = {"row": idx, "status": st, "actor": b.actor, "method": b.method, "a0": b.a0, "a1": b.a1, "a2": b.a2}
        self.ticket[slot] = t + 1
        for f in self.FIELDS:
            self.cols[f][slot] = idx if f == "row" else src[f].index_select(0, idx)
        self.head += K


def rings_equal_or_die(q: DL.DeadLetters, t: TorchRing, what: str) -> None:
    torch.cuda.synchronize()
    ring = q.ring
    w2, w3 = ring[:, DL.W_ROW_STATUS], ring[:, DL.W_ACTOR_METHOD_ATTEMPTS]
    mine = {"row": w2 & 0xFFFFFFFF, "status": (w2 >> 32).to(torch.int32), "actor": w3.to(torch.int32),
            "method": (w3 >> 32).to(torch.int16), "a0": ring[:, DL.W_A0], "a1": ring[:, DL.W_A1], "a2": ring[:, DL.W_A2]}
    if not torch.equal(ring[:, DL.W_TICKET], t.ticket) or q.read()["appended"] != t.head:
        raise RuntimeError(f"dead_letters_cost: {what}: tickets differ from the torch ring's")
    for f in TorchRing.FIELDS:
        if not torch.equal(mine[f], t.cols[f]):
            raise RuntimeError(f"dead_letters_cost: {what}: {f} differs from the torch ring's")


def append_rows(M: int, shares, entries: int, iters: int, reps: int, floor_tbs: float, dev) -> list[str]:
    gen = torch.Generator().manual_seed(M & 0xFFFF)
    lines = [f"### the append alone, M = {M} rows, ring of {entries} records", "",
             "| share of failed rows | K | dlq append us | (b) torch us | append / torch | (c) floor us | append / floor |"
             " status pass alone us (4 B x M at the floor rate) |",
             "|---|---|---|---|---|---|---|---|"]
    b = MsgBatch(torch.randint(0, ACTORS, (M,), generator=gen).to(torch.int32).to(dev),
                 torch.randint(-2**62, 2**62, (M,), generator=gen).to(dev),
                 torch.randint(-2**62, 2**62, (M,), generator=gen).to(dev),
                 torch.randint(-2**62, 2**62, (M,), generator=gen).to(dev),
                 torch.randint(0, 8, (M,), generator=gen).to(torch.int16).to(dev))
    for share in shares:
        if share >= 1:
            st = torch.full((M,), STATUS_FAILED, dtype=torch.int32)
        else:
            st = torch.where(torch.rand(M, generator=gen) < share, STATUS_FAILED, STATUS_OK).to(torch.int32)
        K = int((st != 0).sum())
        st = st.to(dev)
        q, t = DL.DeadLetters(dev, entries, max_rows=M), TorchRing(entries, dev)
        for _ in range(2):  # two Sends: the second starts from a head that is not 0
            q.append(b, st)
            t.append(b, st)
        rings_equal_or_die(q, t, f"M={M} share={share}")
        ts = alternate_events([("dlq", lambda: q.append(b, st)), ("torch", lambda: t.append(b, st))], iters, reps)
        floor = (4 * M + min(K, entries) * (64 + GATHERED)) / (floor_tbs * 1e12) * 1e6
        a, o = statistics.median(ts["dlq"]), statistics.median(ts["torch"])
        lines.append(f"| {share:g} | {K} | {stat(ts['dlq'])} | {stat(ts['torch'])} | {a / o:.3f} | {floor:.1f} | "
                     f"{a / floor:.2f} | {4 * M / (floor_tbs * 1e12) * 1e6:.1f} |")
        del q, t
    return lines + [""]


def send_rows(M: int, iters: int, entries: int, dev) -> list[str]:
    tab = RegistryTable(2 * ACTORS, device=dev)
    ids = torch.arange(ACTORS)
    tab.upsert(actor_keys(ids), torch.zeros(ACTORS, dtype=torch.int32), ids.to(torch.int32))
    tab.enable_directory(ACTORS, affine_world=1)
    ex = ActorExchange(tab, M, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev))
    gen = torch.Generator().manual_seed(5)
    lines = [f"### what `dead_letter=True` adds to a world-1 Send, M = {M} (`Calculator.Multiply` over {ACTORS} actors)",
             "", "| unknown actors | letters per Send | plain Send us | dead-lettered Send us | added us (median - median) |",
             "|---|---|---|---|---|"]
    for share in (0.0, 1e-3):
        actor = torch.randint(0, ACTORS, (M,), generator=gen).to(torch.int32)
        actor[torch.rand(M, generator=gen) < share] = ACTORS + 7
        b = MsgBatch(actor.to(dev), torch.randint(-2**31, 2**31, (M,), generator=gen).to(dev),
                     torch.randint(-2**31, 2**31, (M,), generator=gen).to(dev), None, METHOD_CALC_MULTIPLY)
        q = DL.DeadLetters(dev, entries, max_rows=M)
        pv, ps = ex.send_all(b)
        val, st = ex.send_all(b, dead_letters=q)
        torch.cuda.synchronize()
        K = int((actor == ACTORS + 7).sum())
        if not torch.equal(val, pv) or not torch.equal(st, ps) or int((st == STATUS_NO_ACTOR).sum()) != K:
            raise RuntimeError("dead_letters_cost: the dead-lettered Send's replies differ from the plain Send's")
        ref = DL.DeadLetterRef(entries)
        ref.append(b, st)
        if not torch.equal(q.ring.cpu(), torch.from_numpy(ref.ring.view("int64"))) or q.read()["appended"] != K:
            raise RuntimeError("dead_letters_cost: the ring differs from the model's")
        ts = alternate_host([("plain", lambda: ex.send_all(b)), ("dlq", lambda: ex.send_all(b, dead_letters=q))], iters)
        added = statistics.median(ts["dlq"]) - statistics.median(ts["plain"])
        lines.append(f"| {share:g} | {K} | {stat(ts['plain'])} | {stat(ts['dlq'])} | {added:+.1f} |")
        del q
    return lines + [""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="*", default=[1 << 20, 8 << 20])
    ap.add_argument("--shares", type=float, nargs="*", default=[0, 1e-5, 1e-3, 1e-2, 1])
    ap.add_argument("--entries", type=int, default=1 << 16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--floor-tbs", type=float, default=4.0)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("dead_letters_cost: no GPU", file=sys.stderr)
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

    emit(["# Dead-letter queue: what the append costs, and what `dead_letter=True` adds to a Send", "",
          f"Measured with `python tools/dead_letters_cost.py` (a ring of {a.entries} records, statuses 0 or "
          "`STATUS_FAILED`, a1 / a2 and an int16 method column present).  Sides: the append (both launches of "
          "`DeadLetters.append`, `csrc/hip/dead_letters.hip`); (b) the torch sequence a caller writes without the "
          "feature (`nonzero` on the status mask, which waits on the host for K, `index_select` per column, an indexed "
          "copy into SoA ring columns; of K > entries rows the last `entries`); (c) the byte floor: 4 B of status per "
          f"row, plus 64 B stored and {GATHERED} B gathered per written letter, at {a.floor_tbs} TB/s, the rate the "
          "ring-order drain streams at.  Every side starts from an empty ring and files two Sends, and the rings are "
          "compared field by field for exact equality before anything is timed.", ""])
    emit([f"One MI355X, profiler off.  The append: device events around {a.reps} calls, {a.iters} groups per side after 2 "
          "warm-up rounds, the two sides alternating in one process; both rings compared for exact equality first.  The "
          "torch side waits on the host for K inside every call (`nonzero`), which its time includes.  The Send: host "
          "clock around `send_all` + a device synchronise, plain and dead-lettered alternating.  Cells: median "
          "(min .. max).", ""])
    for M in a.msgs:
        emit(append_rows(M, a.shares, a.entries, a.iters, a.reps, a.floor_tbs, dev))
    for M in a.msgs:
        emit(send_rows(M, max(5, a.iters), a.entries, dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
