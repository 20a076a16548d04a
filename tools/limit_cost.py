#!/usr/bin/env python3
"""What the rate limiter (ops/limit.py, csrc/hip/limit.hip) costs and saves.

Every row compares the plain Send with the limited Send of the same batch, the two
alternating inside one process (the baseline is always the plain Send of this run),
world 1, eager ``send_all``, ``--actors`` actors.  Results are compared first: a limited
reply is the plain one or ``(0, STATUS_THROTTLED)``, and the throttled rows are the
numpy model's.  ``rate == burst`` in every case, so each Send finds full buckets and every
Send of a case does the same work.

a.  ``Calculator.Multiply``, nothing over quota, uniform and Zipf(1.1) ids: the price every
    limited Send pays (the demand and step launches, the host read of ``over``).
b.  One hot actor: 10 % of the batch, ``burst`` at half its demand.
c.  Every actor over quota: ``burst = 1``.
d.  ``Prime.Check`` with a per-candidate delay (``--delay-us``), Zipf ids, ``--prime-msgs``
    messages, ``burst = --prime-burst``: the slow handler the limiter keeps a hot actor from.

The parts are timed on their own: the demand and step launches with device events, the
whole admission (launches, host reads) with a host clock.  ``--kernels CASE`` runs only
``--iters`` admissions of one case (a, a-zipf, b, c), for a kernel trace of their own.

    python tools/limit_cost.py [--msgs 8388608] [--iters 20] [--reps 10] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import _ptr, hip, raw_stream  # noqa: E402
from ptype_amd.ops import limit as LM  # noqa: E402
from ptype_amd.ops.batch import MsgBatch, zipf_actors  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_PRIME_CHECK, STATUS_OK, STATUS_THROTTLED  # noqa: E402
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402


def table(n: int, dev) -> RegistryTable:
    tab = RegistryTable(2 * n, device=dev)
    ids = torch.arange(n)
    tab.upsert(actor_keys(ids), torch.zeros(n, dtype=torch.int32), ids.to(torch.int32))
    tab.enable_directory(n, affine_world=1)
    return tab


def stat(ts) -> str:
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def events(fn, reps: int) -> list[float]:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        fn()
    per = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / reps)
    return per


def alternate(variants, iters: int) -> dict:
    """Host clock around each variant + a device synchronise, the variants alternating."""
    ts = {name: [] for name, _ in variants}
    for it in range(iters + 3):  # 3 warm-up rounds
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 3:
                ts[name].append((time.perf_counter() - t0) * 1e6)
    return ts


def ids_of(case: str, M: int, n: int, dev, g) -> torch.Tensor:
    if case == "a-zipf" or case == "d":
        return zipf_actors(M, n, 1.1, 5, dev)
    ids = torch.randint(0, n, (M,), generator=g).to(torch.int32)
    if case == "b":  # every tenth row to actor 0
        ids[::10] = 0
    return ids.to(dev)


def burst_of(case: str, ids: torch.Tensor, a) -> int:
    if case == "b":
        return max(1, int((ids == 0).sum()) // 2)
    if case == "c":
        return 1
    if case == "d":
        return a.prime_burst
    return 2**31  # nothing is ever over quota


def check(out, want, b: MsgBatch, lim: LM.Limiter, what: str) -> int:
    """A limited reply is the plain one or a rejection, and the rejections are the model's."""
    torch.cuda.synchronize()
    ref = LM.LimiterRef(actors=lim.n, rate=lim.rate, burst=lim.burst)
    cut = ref.admit(MsgBatch(b.actor.cpu(), b.a0.cpu(), None, None, b.method))
    thr = out[1] == STATUS_THROTTLED
    same = (out[1] == want[1]) & ((out[0] == want[0]) | (want[1] != STATUS_OK))
    model = torch.zeros_like(thr) if cut is None else (cut[1] == STATUS_THROTTLED).to(thr.device)
    if not bool((same | (thr & (out[0] == 0))).all()) or not torch.equal(thr, model):
        raise RuntimeError(f"limit_cost: {what}: the limited Send's replies differ from the plain Send's or the model's")
    return int(thr.sum())


def demand_only(lim: LM.Limiter, actor: torch.Tensor):
    """The demand and step launches alone, and what re-arms them when actors are hot."""
    M, s = actor.numel(), raw_stream(lim.device)

    def fn():
        hip().limit_demand(_ptr(actor), M, _ptr(lim.table), _ptr(lim.demand), _ptr(lim.touched), _ptr(lim.hot_actor),
                           _ptr(lim.rem), _ptr(lim.prefix), _ptr(lim.busy), _ptr(lim.ctr), lim.n, lim.begin(), lim.rate,
                           lim.burst, s)
        lim.end()

    return fn


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="+", default=[1 << 23])
    ap.add_argument("--actors", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--delay-us", type=int, default=2)
    ap.add_argument("--prime-msgs", type=int, default=1 << 18)
    ap.add_argument("--prime-burst", type=int, default=8)
    ap.add_argument("--kernels", default="", help="run only --iters admissions of this case (a, a-zipf, b, c)")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = a.actors
    g = torch.Generator().manual_seed(7)

    if a.kernels:
        M = a.msgs[0]
        ids = ids_of(a.kernels, M, n, dev, g)
        burst = burst_of(a.kernels, ids, a)
        lim = LM.Limiter(dev, actors=n, rate=burst, burst=burst)
        b = MsgBatch(ids, torch.zeros(M, dtype=torch.int64, device=dev), None, None, METHOD_CALC_MULTIPLY)
        for _ in range(a.iters):
            lim.begin()
            lim.admit(b)
            lim.end()
        torch.cuda.synchronize()
        print(f"limit_cost: {a.iters} admissions of case {a.kernels}, M = {M}, over = {lim.over}, digit = {LM.DIGIT}")
        return 0

    lines = ["# Rate limiter: what a limited Send costs and saves", "",
             f"`python tools/limit_cost.py --msgs {' '.join(map(str, a.msgs))} --actors {n} --iters {a.iters}` on "
             f"{torch.cuda.get_device_name(0)}.  Microseconds, median (min .. max) of {a.iters} Sends; plain and "
             f"limited Sends alternate in one process.  rate = burst; {LM.DIGIT} bits of the row index per level of the "
             "radix select.", ""]
    say = (lambda s="": (print(s, flush=True), lines.append(s)))

    say("## Calculator.Multiply")
    say()
    say("| messages | case | burst | actors over quota | plain Send | limited Send | throttled | admission alone (host "
        "clock, with its reads) | demand + step launches (device) | levels |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for M in a.msgs:
        for case, name in (("a", "(a) nothing over quota, uniform ids"), ("a-zipf", "(a) nothing over quota, Zipf(1.1) ids"),
                           ("b", "(b) one hot actor with 10 % of the rows"), ("c", "(c) every actor over quota")):
            ids = ids_of(case, M, n, dev, g)
            b = MsgBatch(ids, torch.randint(-9, 9, (M,), generator=g).to(dev),
                         torch.randint(-9, 9, (M,), generator=g).to(dev), None, METHOD_CALC_MULTIPLY)
            ex = ActorExchange(table(n, dev), M, chunks=1, state=torch.zeros(n, dtype=torch.int64, device=dev),
                               delivery="direct")
            burst = burst_of(case, ids, a)
            lim = LM.Limiter(dev, actors=n, rate=burst, burst=burst)
            want = ex.send_all(b)
            out = lim.send(b, ex.send_all)
            throttled = check(out, want, b, lim, name)
            over = lim.over
            ts = alternate([("plain", lambda: ex.send_all(b)), ("limited", lambda: lim.send(b, ex.send_all))], a.iters)

            def admit():
                lim.begin()
                lim.admit(b)
                lim.end()

            adm = alternate([("admit", admit)], a.iters)["admit"]
            dem = "-"
            if over == 0:  # (with hot actors the launches leave slots that only the cut re-arms)
                dem = stat(events(demand_only(lim, ids), a.reps))
            say(f"| {M} | {name} | {burst} | {over} | {stat(ts['plain'])} | {stat(ts['limited'])} | {throttled} | "
                f"{stat(adm)} | {dem} | {LM.levels(M)} |")
            del ex, lim
    say()

    if a.delay_us > 0:
        M = a.prime_msgs
        say(f"## (d) Prime.Check, delay_us = {a.delay_us} per candidate (at most 8 candidates per call), Zipf(1.1) ids, "
            f"M = {M}")
        say()
        say("| burst | actors over quota | plain Send | limited Send | throttled | limited / plain |")
        say("|---|---|---|---|---|---|")
        ids = ids_of("d", M, n, dev, g)
        b = MsgBatch(ids, torch.full((M,), 2, dtype=torch.int64, device=dev),
                     torch.full((M,), 10, dtype=torch.int64, device=dev), 1009 + 2 * torch.arange(M, device=dev),
                     METHOD_PRIME_CHECK)
        ex = ActorExchange(table(n, dev), M, state=torch.zeros(n, dtype=torch.int64, device=dev), delay_us=a.delay_us)
        lim = LM.Limiter(dev, actors=n, rate=a.prime_burst, burst=a.prime_burst)
        want = ex.send_all(b)
        out = lim.send(b, ex.send_all)
        throttled = check(out, want, b, lim, "Prime.Check")
        ts = alternate([("plain", lambda: ex.send_all(b)), ("limited", lambda: lim.send(b, ex.send_all))],
                       max(3, a.iters // 4))
        p, q = statistics.median(ts["plain"]), statistics.median(ts["limited"])
        say(f"| {a.prime_burst} | {lim.over} | {stat(ts['plain'])} | {stat(ts['limited'])} | {throttled} | {q / p:.2f} |")
        say()
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
