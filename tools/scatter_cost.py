#!/usr/bin/env python3
"""What the call scatter (ops/scatter.py, csrc/hip/scatter.hip) costs.

1.  ``Scatter.expand`` at each shape against the torch sequence it replaces: for
    ``ranges`` the body of ``models.optimus.FanOut.__init__`` (``repeat_interleave``,
    ``cumsum``, two ``arange``, ``where``, a modulo, an index gather, one host read), for
    ``members`` its obvious equivalent (``repeat_interleave`` plus index gathers).  Both
    sides contain one host read, so both are timed with the host clock around the call
    plus a device synchronise, alternating in one process; the columns are compared for
    exact equality before anything is timed.  Next to them the expand's launches by
    device events -- the three before the host read (count, scan, first) and the expand
    launch alone -- and the byte floor: 32 B written per row (``members`` with two argument
    columns: 24 B written and the 4-B member id read) plus about 24 B read per question, at
    ``--floor-tbs`` TB/s (the streaming rate profiles/gather.md uses).
2.  What one ``DeviceRuntime.ask`` adds over ``send(prebuilt batch, gather=)`` at those
    shapes on a world-1 runtime: the expand plus its host read.

    python tools/scatter_cost.py [--iters 10] [--reps 10] [--md FILE] [--small] [--only TEXT] [--no-ask]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.models import optimus  # noqa: E402
from ptype_amd.ops import scatter as S  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_PRIME_CHECK  # noqa: E402

ACTORS = 1 << 20


def stat(ts) -> str:
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def alternate_host(variants, iters: int) -> dict:
    """us per call by the host clock (the call plus a device synchronise), the variants
    alternating, ``iters`` rounds after three warm-up rounds."""
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


def events(fn, iters: int, reps: int) -> list:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for it in range(iters + 2):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        if it >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return ts


def torch_members(offsets, members, qs: MsgBatch):
    """The members rule with torch ops (group ids all valid)."""
    g = qs.actor.to(torch.int64)
    lo = offsets[g]
    n = offsets[g + 1] - lo
    total = int(n.sum())
    Q = g.numel()
    tid = torch.repeat_interleave(torch.arange(Q, device=g.device), n)
    first = torch.cumsum(n, 0) - n
    k = torch.arange(total, device=g.device) - first[tid]
    return MsgBatch(members[lo[tid] + k], qs.a0[tid], qs.a1[tid], None, qs.method), tid.to(torch.int32), first, n


def shapes(small: bool, dev):
    """(name, Scatter, questions, the torch side -> (batch, group, first, n))."""
    k = 16 if small else 1
    gen = torch.Generator().manual_seed(7)
    out = []
    for name, tg in (("ranges, 1024 targets (optimus_fanout)", torch.arange(1024) * 2 + 80_001 // k),
                     ("ranges, 8192 targets", torch.arange(8192) * 2 + 2_001 // k),
                     ("ranges, one giant target", torch.tensor([83_000_000 // k]))):
        tg = tg.to(torch.int64).to(dev)
        rows = int(((tg + 9) // 10).sum())
        sc = S.Scatter.ranges(10, ACTORS, first_lo=2, capacity=rows, q_capacity=max(int(tg.numel()), 1))
        qs = MsgBatch(torch.zeros(tg.numel(), dtype=torch.int32, device=dev), tg, None, None, METHOD_PRIME_CHECK)

        def side(tg=tg):
            f = optimus.FanOut(tg, ACTORS, dev)
            return f.batch, None, f.first, f.n

        out.append((name, sc, qs, side))
    for rows in ((1 << 20) // k, (8 << 20) // k):
        for kind in ("uniform", "Zipf"):
            G = rows // 64
            if kind == "uniform":
                sizes = torch.full((G,), 64, dtype=torch.int64)
            else:  # sizes ~ 1 / rank^1.1, scaled to the same total, in random group order
                w = torch.arange(1, G + 1, dtype=torch.float64).pow(-1.1)
                sizes = torch.floor(w / w.sum() * rows).to(torch.int64)[torch.randperm(G, generator=gen)]
            offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)]).to(dev)
            members = torch.randint(0, ACTORS, (int(sizes.sum()),), generator=gen).to(torch.int32).to(dev)
            sc = S.Scatter.members(offsets, members, capacity=max(int(sizes.sum()), 1), q_capacity=G)
            qs = MsgBatch(torch.randperm(G, generator=gen).to(torch.int32).to(dev),
                          torch.randint(-2**31, 2**31, (G,), generator=gen).to(dev),
                          torch.randint(-2**31, 2**31, (G,), generator=gen).to(dev), None, METHOD_CALC_MULTIPLY)

            def side(offsets=offsets, members=members, qs=qs):
                return torch_members(offsets, members, qs)

            out.append((f"members, {kind} sizes, {G} groups", sc, qs, side))
    return out


def equal_or_die(exp: S.Expansion, other, what: str) -> None:
    batch, group, first, n = other
    torch.cuda.synchronize()
    pairs = [(exp.batch.actor, batch.actor), (exp.batch.a0, batch.a0), (exp.batch.a1, batch.a1),
             (exp.batch.a2, batch.a2), (exp.first, first), (exp.n.to(torch.int64), n)]
    if group is not None:
        pairs.append((exp.group, group))
    for i, (a, b) in enumerate(pairs):
        if (a is None) != (b is None) or (a is not None and not torch.equal(a, b)):
            raise RuntimeError(f"scatter_cost: {what}: column {i} differs from the torch side's")
    if exp.batch.method != batch.method:
        raise RuntimeError(f"scatter_cost: {what}: the method differs")


def expand_rows(cases, iters: int, reps: int, floor_tbs: float) -> list[str]:
    lines = ["### expand against the torch sequence it replaces", "",
             "| shape | Q | rows | expand us | torch us | expand / torch | count + scan + first us | expand launch us | "
             "byte floor us | expand launch / floor |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, sc, qs, side in cases:
        exp = sc.expand(qs)
        equal_or_die(exp, side(), name)
        Q, rows = exp.Q, exp.total
        ts = alternate_host([("expand", lambda: sc.expand(qs)), ("torch", side)], iters)
        members = sc.rule == "members"
        cols = (qs.actor, qs.a0, qs.a1 if members else None, qs.a2 if members else None, None)
        t_count = events(lambda: sc._count(cols, Q), iters, reps)
        t_fill = events(lambda: sc._fill(cols, Q, rows), iters, reps)
        # written per row: actor, group and the int64 columns (ranges 32 B; members 8 + 8 per column the
        # questions have, plus the 4-B member id it reads); per question about 24 B of reads
        row_bytes = 32 if not members else 8 + 8 * sum(c is not None for c in cols[1:4]) + 4
        floor = (row_bytes * rows + 24 * Q) / (floor_tbs * 1e12) * 1e6
        a, b = statistics.median(ts["expand"]), statistics.median(ts["torch"])
        lines.append(f"| {name} | {Q} | {rows} | {stat(ts['expand'])} | {stat(ts['torch'])} | {a / b:.2f} | {stat(t_count)} | "
                     f"{stat(t_fill)} | {floor:.1f} | {statistics.median(t_fill) / floor:.2f} |")
        print(lines[-1], flush=True)
    return lines + [""]


def ask_rows(cases, iters: int, dev) -> list[str]:
    from ptype_amd.runtime import DeviceRuntime

    lines = ["### what one `ask` adds over `send(prebuilt batch, gather=)`, world 1", "",
             "| shape | rows | op | Send us | Ask us | added us (median - median) |", "|---|---|---|---|---|---|"]
    for name, sc, qs, _ in cases:
        exp = sc.expand(qs)
        rt = DeviceRuntime(dev, actors=ACTORS, service="calculator", shm=False, max_batch=max(exp.total, 1))
        rt.place_local()
        rt.host(optimus.SERVICE)
        try:
            ranges = sc.rule == "ranges"
            service, op, sen = (optimus.SERVICE, "first_ne", qs.a0) if ranges else ("calculator", "sum", None)
            g = exp.gather(op, sen)
            ts = alternate_host([("send", lambda: rt.send(service, exp.batch, gather=g)),
                                 ("ask", lambda: rt.ask(service, qs, sc, op=op, sentinel=sen))], iters)
            added = statistics.median(ts["ask"]) - statistics.median(ts["send"])
            lines.append(f"| {name} | {exp.total} | {op} | {stat(ts['send'])} | {stat(ts['ask'])} | {added:+.1f} |")
            print(lines[-1], flush=True)
        finally:
            rt.close()
    return lines + [""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--floor-tbs", type=float, default=4.0)
    ap.add_argument("--small", action="store_true", help="every shape at 1/16 of its rows (a quick look)")
    ap.add_argument("--only", default="", help="only the shapes whose name contains this text (a profiled run)")
    ap.add_argument("--no-ask", action="store_true", help="skip the Ask section")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("scatter_cost: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = []

    def emit(new):  # written section by section: a failure later keeps what was measured
        lines.extend(new)
        if a.md:
            os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
            with open(a.md, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit([f"One MI355X, profiler off.  expand, the torch side, Send and Ask: host clock around the call + a device "
          f"synchronise, {a.iters} rounds per side after 3 warm-up rounds, the two sides alternating in one process; the "
          f"columns compared for exact equality first.  The launches: device events around {a.reps} calls, {a.iters} "
          "groups after 2 warm-up groups.  Cells: median (min .. max).", ""])
    cases = [c for c in shapes(a.small, dev) if a.only in c[0]]
    emit(expand_rows(cases, a.iters, a.reps, a.floor_tbs))
    if not a.no_ask:
        emit(ask_rows(cases, max(5, a.iters), dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
