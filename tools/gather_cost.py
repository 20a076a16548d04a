#!/usr/bin/env python3
"""What the reply gather (ops/gather.py, csrc/hip/gather.hip) costs.

1.  The reduce alone (both launches) at each ``--msgs`` size, on three layouts --
    contiguous runs (a fan-out's layout, mean run about 100), uniformly random ids
    over 1024 groups and over 1 Mi groups -- against
    (a) ``prime_gather`` (csrc/hip/optimus.hip), on the runs layout with ``first_ne``;
    (b) the torch sequence a caller writes without it: ``index_add_`` /
        ``scatter_reduce_`` on the masked replies for value, count and n_ok, plus the
        ``amin`` of the failed rows and the gather of their statuses;
    (c) the byte floor: 16 B per message at ``--floor-tbs`` TB/s (the README's
        streaming rate of the ring-order drain).
    Two more rows time the reduce on views that are not 16-byte aligned (scalar
    loads) against the aligned reduce of the same data.
    The sides alternate inside one process, device events around ``--reps`` calls;
    every side's outputs are compared for exact equality before anything is timed.
2.  What ``gather=`` adds to a world-1 Send (eager ``send_all``, host clock around
    the Send plus a device synchronise, the two variants alternating).

    python tools/gather_cost.py [--msgs 1048576 8388608] [--iters 10] [--reps 10] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import gather as G  # noqa: E402
from ptype_amd.ops import hip, raw_stream  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_FAILED, STATUS_OK  # noqa: E402
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402

ACTORS = 1 << 20
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


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


def torch_gather(val, st, group64, groups: int, op: str, rows, ones):
    """(b): what a caller writes with torch ops for value / count / n_ok / bad_row / status."""
    M = val.numel()
    ok = st == STATUS_OK
    if op == "sum":
        value = torch.zeros(groups, dtype=torch.int64, device=val.device).index_add_(0, group64, torch.where(ok, val, 0))
    else:
        ident = I64_MAX if op == "min" else I64_MIN
        value = torch.full((groups,), ident, dtype=torch.int64, device=val.device).scatter_reduce_(
            0, group64, torch.where(ok, val, ident), "amin" if op == "min" else "amax")
    count = torch.zeros(groups, dtype=torch.int32, device=val.device).index_add_(0, group64, ones)
    n_ok = torch.zeros(groups, dtype=torch.int32, device=val.device).index_add_(0, group64, ok.to(torch.int32))
    bad = torch.full((groups,), M, dtype=torch.int64, device=val.device).scatter_reduce_(
        0, group64, torch.where(ok, M, rows), "amin")
    status = torch.where(bad < M, st[bad.clamp(max=M - 1)], STATUS_OK)
    return value, status, n_ok, count, torch.where(bad < M, bad, -1).to(torch.int32)


def equal_or_die(g: G.Gather, other, what: str) -> None:
    torch.cuda.synchronize()
    for name, t in zip(("value", "status", "n_ok", "count", "bad_row"), other):
        if not torch.equal(getattr(g, name), t):
            raise RuntimeError(f"gather_cost: {what}: {name} differs from the Gather's")


def replies(M: int, gen, dev):
    val = torch.randint(-2**62, 2**62, (M,), generator=gen)
    st = torch.where(torch.rand(M, generator=gen) < 0.001, STATUS_FAILED, STATUS_OK).to(torch.int32)
    return val.to(dev), st.to(dev)


def reduce_rows(M: int, iters: int, reps: int, floor_tbs: float, dev) -> list[str]:
    gen = torch.Generator().manual_seed(M & 0xFFFF)
    floor = 16 * M / (floor_tbs * 1e12) * 1e6
    lines = [f"### the reduce alone, M = {M} messages (byte floor (c): 16 B x M at {floor_tbs} TB/s = {floor:.1f} us)", "",
             "| layout | G | op | reply_gather us | other side | other side us | gather / other | gather / floor |",
             "|---|---|---|---|---|---|---|---|"]

    def row(layout, groups, op, name, ts):
        a, b = statistics.median(ts["gather"]), statistics.median(ts[name])
        lines.append(f"| {layout} | {groups} | {op} | {stat(ts['gather'])} | {name} | {stat(ts[name])} | {a / b:.2f} | "
                     f"{a / floor:.2f} |")

    # contiguous runs, mean length about 100: the FanOut layout
    lens = torch.randint(1, 200, (M // 100 + 1,), generator=gen)
    lens = lens[torch.cumsum(lens, 0) <= M]
    lens[-1] += M - int(lens.sum())
    T = int(lens.numel())
    first = (torch.cumsum(lens, 0) - lens).to(dev)
    group = torch.repeat_interleave(torch.arange(T, dtype=torch.int32), lens).to(dev)
    group64, rows, ones = group.to(torch.int64), torch.arange(M, device=dev), torch.ones(M, dtype=torch.int32, device=dev)
    targets = torch.randint(2, 2**40, (T,), generator=gen).to(dev)
    val, st = replies(M, gen, dev)
    # a fan-out's replies: the target, but for one divisor row in about half of the groups
    pv = targets[group64].clone()
    hit_rows = (first + (torch.rand(T, generator=gen).to(dev) * lens.to(dev)).to(torch.int64))[::2]
    pv[hit_rows] = 7
    answer = torch.empty(T, dtype=torch.int64, device=dev)
    ans_st = torch.empty(T, dtype=torch.int32, device=dev)
    lens_d = lens.to(dev)
    g = G.Gather(group, T, "first_ne", targets)
    prime = (lambda: hip().prime_gather(pv.data_ptr(), st.data_ptr(), first.data_ptr(), lens_d.data_ptr(),
                                        targets.data_ptr(), T, answer.data_ptr(), ans_st.data_ptr(), 0, raw_stream(dev)))
    g.reduce(pv, st)
    prime()
    torch.cuda.synchronize()
    if not torch.equal(g.value, answer) or not torch.equal(g.status, ans_st):
        raise RuntimeError("gather_cost: first_ne differs from prime_gather")
    ts = alternate_events([("gather", lambda: g.reduce(pv, st)), ("(a) prime_gather", prime)], iters, reps)
    row("runs ~100", T, "first_ne", "(a) prime_gather", ts)
    del g
    for layout, groups, grp in (("runs ~100", T, group), ("random", 1024, None), ("random", 1 << 20, None)):
        if grp is None:
            grp = torch.randint(0, groups, (M,), generator=gen).to(torch.int32).to(dev)
        grp64 = grp.to(torch.int64)
        for op in ("sum", "min"):
            g = G.Gather(grp, groups, op)
            g.reduce(val, st)
            equal_or_die(g, torch_gather(val, st, grp64, groups, op, rows, ones), f"{layout} G={groups} {op}")
            ts = alternate_events([("gather", lambda: g.reduce(val, st)),
                                   ("(b) torch", lambda: torch_gather(val, st, grp64, groups, op, rows, ones))],
                                  iters, reps)
            row(layout, groups, op, "(b) torch", ts)
            del g
    # views that are not 16-byte aligned (every column at an odd element offset): the same
    # layout with scalar loads, against the aligned reduce of the same data
    for layout, groups, grp in (("runs ~100, [1:] views", T, group), ("random, [1:] views", 1024, None)):
        if grp is None:
            grp = torch.randint(0, groups, (M,), generator=gen).to(torch.int32).to(dev)
        pad = (lambda t: torch.cat([t[:1], t])[1:])
        val1, st1, grp1 = pad(val), pad(st), pad(grp)
        if not (val1.data_ptr() % 16 and st1.data_ptr() % 16 and grp1.data_ptr() % 16):
            raise RuntimeError("gather_cost: the views are aligned")
        g, g1 = G.Gather(grp, groups, "sum"), G.Gather(grp1, groups, "sum")
        g.reduce(val, st)
        g1.reduce(val1, st1)
        equal_or_die(g, [getattr(g1, f) for f in ("value", "status", "n_ok", "count", "bad_row")], f"{layout}")
        ts = alternate_events([("gather", lambda: g1.reduce(val1, st1)), ("aligned reply_gather", lambda: g.reduce(val, st))],
                              iters, reps)
        row(layout, groups, "sum", "aligned reply_gather", ts)
        del g, g1
    return lines + [""]


def send_rows(M: int, iters: int, dev) -> list[str]:
    tab = RegistryTable(2 * ACTORS, device=dev)
    ids = torch.arange(ACTORS)
    tab.upsert(actor_keys(ids), torch.zeros(ACTORS, dtype=torch.int32), ids.to(torch.int32))
    tab.enable_directory(ACTORS, affine_world=1)
    ex = ActorExchange(tab, M, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev))
    gen = torch.Generator().manual_seed(5)
    b = MsgBatch(torch.randint(0, ACTORS, (M,), generator=gen).to(torch.int32).to(dev),
                 torch.randint(-2**31, 2**31, (M,), generator=gen).to(dev),
                 torch.randint(-2**31, 2**31, (M,), generator=gen).to(dev), None, METHOD_CALC_MULTIPLY)
    lines = [f"### what `gather=` adds to a world-1 Send, M = {M} (`Calculator.Multiply` over {ACTORS} actors)", "",
             "| gather | G | Send us | added us (median - the plain Send's median) |", "|---|---|---|---|"]
    cases = [("runs of 100, sum", (torch.arange(M, dtype=torch.int32) // 100).to(dev), (M + 99) // 100, "sum"),
             ("random, G = 1024, sum", torch.randint(0, 1024, (M,), generator=gen).to(torch.int32).to(dev), 1024, "sum"),
             ("random, G = 1 Mi, sum", torch.randint(0, 1 << 20, (M,), generator=gen).to(torch.int32).to(dev), 1 << 20,
              "sum")]
    for name, grp, groups, op in cases:
        g = G.Gather(grp, groups, op)
        val, st = ex.send_all(b, gather=g)
        torch.cuda.synchronize()
        want = G.gather_ref(val, st, grp, groups, op)
        for f in G.Gather.FIELDS:
            if not torch.equal(getattr(g, f).cpu(), want[f]):
                raise RuntimeError(f"gather_cost: Send(gather=) {name}: {f} differs from gather_ref")
        ts = alternate_host([("plain", lambda: ex.send_all(b)), ("gathered", lambda: ex.send_all(b, gather=g))], iters)
        added = statistics.median(ts["gathered"]) - statistics.median(ts["plain"])
        lines.append(f"| off | | {stat(ts['plain'])} | |")
        lines.append(f"| {name} | {groups} | {stat(ts['gathered'])} | {added:+.1f} |")
        del g
    return lines + [""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="*", default=[1 << 20, 8 << 20])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--floor-tbs", type=float, default=4.0)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("gather_cost: no GPU", file=sys.stderr)
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

    emit([f"One MI355X, profiler off.  The reduce: device events around {a.reps} calls, {a.iters} groups per side after 2 "
          "warm-up rounds, the two sides alternating in one process; every side's outputs compared for exact equality "
          "first.  The Send: host clock around `send_all` + a device synchronise, plain and gathered alternating.  "
          "Cells: median (min .. max).", ""])
    for M in a.msgs:
        emit(reduce_rows(M, a.iters, a.reps, a.floor_tbs, dev))
    for M in a.msgs:
        emit(send_rows(M, max(5, a.iters), dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
