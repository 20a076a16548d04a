#!/usr/bin/env python3
"""What the circuit breaker (ops/breaker.py, csrc/hip/breaker.hip) costs and saves.

Every row compares the plain Send with the guarded Send of the same batch, the two
alternating inside one process (the baseline is always the plain Send of this run),
world 1, eager ``send_all``, ``--actors`` actors with uniform random ids.  Results are
compared first: a guarded reply is the plain one, or ``STATUS_BREAKER_OPEN`` where the
plain Send answered a status that trips.

1.  ``Calculator.Multiply`` at each ``--msgs`` size: nothing failing; 1 % of the actors
    unregistered (``STATUS_NO_ACTOR``: they trip and stay open); every actor open.  The
    healthy row's parts are timed on their own: the three observation launches with
    device events, the host read of ``n_open`` with a host clock.
2.  ``RPCRetryTest`` with ``retries=3`` and 1 % / 10 % of the actors never passing: the
    guarded Send, once the breakers have tripped, against the plain retried Send.
3.  All messages to one failing actor: the observation launches alone.

    python tools/breaker_cost.py [--msgs 1048576 8388608] [--iters 20] [--reps 10] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import breaker as BR  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_RETRY_TEST, STATUS_BREAKER_OPEN, STATUS_FAILED,  # noqa: E402
                                   STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402

COOLDOWN = 1 << 20  # an open actor stays open for the whole measurement


def table(n: int, dev, skip_every: int = 0, none: bool = False) -> RegistryTable:
    """``n`` actors registered, except every ``skip_every``-th id (or none at all)."""
    tab = RegistryTable(2 * n, device=dev)
    ids = torch.arange(n)
    if skip_every:
        ids = ids[ids % skip_every != 0]
    if none:
        ids = ids[:1] + n  # (one id past the batch's range keeps the table non-empty)
    tab.upsert(actor_keys(ids), torch.zeros(ids.numel(), dtype=torch.int32), ids.to(torch.int32) % n)
    tab.enable_directory(2 * n, affine_world=1)
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


def check(out, want, trip_mask: int, what: str) -> int:
    """A guarded reply is the plain one, or a rejection of a row whose plain status trips."""
    torch.cuda.synchronize()
    rej = out[1] == STATUS_BREAKER_OPEN
    same = (out[1] == want[1]) & ((out[0] == want[0]) | (want[1] != STATUS_OK))
    tripping = ((trip_mask >> want[1].clamp(0, 31).to(torch.int64)) & 1) != 0
    if not bool((same | (rej & tripping & (out[0] == 0))).all()):
        raise RuntimeError(f"breaker_cost: {what}: the guarded Send's replies differ from the plain Send's")
    return int(rej.sum())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="+", default=[1 << 20, 1 << 23])
    ap.add_argument("--actors", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = a.actors
    lines = ["# Circuit breaker: what a guarded Send costs and saves", "",
             f"`python tools/breaker_cost.py --msgs {' '.join(map(str, a.msgs))} --actors {n} --iters {a.iters}` on "
             f"{torch.cuda.get_device_name(0)}.  Microseconds, median (min .. max) of {a.iters} Sends; plain and "
             "guarded Sends alternate in one process.  threshold 5; an open actor stays open while it is measured.", ""]
    say = (lambda s="": (print(s, flush=True), lines.append(s)))
    g = torch.Generator().manual_seed(7)
    mask = BR.trip_mask()

    # ---- 1. Calculator.Multiply
    say("## Calculator.Multiply, uniform ids")
    say()
    say("| messages | case | plain Send | guarded Send | rejected | observe launches alone | n_open read alone |")
    say("|---|---|---|---|---|---|---|")
    for M in a.msgs:
        ids = torch.randint(0, n, (M,), generator=g).to(torch.int32).to(dev)
        b = MsgBatch(ids, torch.randint(-9, 9, (M,), generator=g).to(dev), torch.randint(-9, 9, (M,), generator=g).to(dev),
                     None, METHOD_CALC_MULTIPLY)
        for case, tab in (("nothing failing", table(n, dev)), ("1 % of the actors failing", table(n, dev, skip_every=100)),
                          ("every actor open", table(n, dev, none=True))):
            ex = ActorExchange(tab, M, chunks=1, state=torch.zeros(n, dtype=torch.int64, device=dev), delivery="direct")
            br = BR.Breaker(dev, actors=n, threshold=5, cooldown=COOLDOWN)
            want = ex.send_all(b)
            for _ in range(6):  # the failing actors trip (one with few messages per Send needs more than one)
                out = br.send(b, ex.send_all)
            rejected = check(out, want, mask, case)
            ts = alternate([("plain", lambda: ex.send_all(b)), ("guarded", lambda: br.send(b, ex.send_all))], a.iters)
            obs = read = "-"
            if case == "nothing failing":
                st = want[1]
                br.begin()
                obs = stat(events(lambda: br.observe(b, st), a.reps))
                t = []
                for _ in range(50):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    br._n_open()
                    t.append((time.perf_counter() - t0) * 1e6)
                read = stat(t)
            say(f"| {M} | {case} | {stat(ts['plain'])} | {stat(ts['guarded'])} | {rejected} | {obs} | {read} |")
            del ex, br
    say()
    say("The healthy guarded Send's floor is the bad-row pass streaming 4 B per message (32 MB at 8 Mi: about 8 us at "
        "4 TB/s) plus two near-empty launches and the `n_open` read.")
    say()

    # ---- 2. RPCRetryTest with retries=3
    say("## RPCRetryTest, retries=3, actors that never pass")
    say()
    say("| messages | failing actors | plain retried Send | guarded Send (tripped) | rejected |")
    say("|---|---|---|---|---|")
    for M in a.msgs:
        ids = torch.randint(0, n, (M,), generator=g).to(torch.int32).to(dev)
        for pct, every in ((1, 100), (10, 10)):
            a0 = torch.where(ids % every == 0, 10**12, 0)
            b = MsgBatch(ids, a0, None, None, METHOD_RETRY_TEST)
            ex = ActorExchange(table(n, dev), M, chunks=1, state=torch.zeros(n, dtype=torch.int64, device=dev),
                               delivery="direct")
            br = BR.Breaker(dev, actors=n, threshold=5, cooldown=COOLDOWN)
            plain = (lambda: ex.send_all(b, retries=3))
            plain_sub = (lambda sub: ex.send_all(sub, retries=3))
            want = plain()
            for _ in range(6):  # (an actor with few messages per Send needs more than one to trip)
                out = br.send(b, plain_sub)
            torch.cuda.synchronize()
            rej = out[1] == STATUS_BREAKER_OPEN
            if not bool(torch.where(rej, want[1] == STATUS_FAILED, out[1] == want[1]).all()):
                raise RuntimeError("breaker_cost: retries: the guarded Send rejects other rows than the plain Send fails")
            ts = alternate([("plain", plain), ("guarded", lambda: br.send(b, plain_sub))], a.iters)
            say(f"| {M} | {pct} % | {stat(ts['plain'])} | {stat(ts['guarded'])} | {int(rej.sum())} |")
            del ex, br
    say()

    # ---- 3. the observation launches alone
    say("## The observation launches alone (bad-row pass, ok pass, step)")
    say()
    say("| messages | statuses | device time |")
    say("|---|---|---|")
    for M in a.msgs:
        ids = torch.randint(0, n, (M,), generator=g).to(torch.int32).to(dev)
        one = torch.full((M,), 7, dtype=torch.int32, device=dev)
        ok = torch.zeros(M, dtype=torch.int32, device=dev)
        bad = torch.full((M,), STATUS_FAILED, dtype=torch.int32, device=dev)
        for what, col, st in (("all OK, uniform ids", ids, ok), ("all failed, uniform ids", ids, bad),
                              ("all failed, one actor", one, bad), ("all OK, one dirty actor", one, ok)):
            br = BR.Breaker(dev, actors=n, threshold=2**32 - 1, cooldown=COOLDOWN)  # (never trips: every call does the work)
            br.begin()
            batch = MsgBatch(col, ids.to(torch.int64), None, None, METHOD_RETRY_TEST)
            if what == "all OK, one dirty actor":
                keep = MsgBatch(one[:1], ids[:1].to(torch.int64), None, None, METHOD_RETRY_TEST)
                fn = (lambda: (br.observe(keep, bad[:1]), br.observe(batch, st)))  # (an OK resets: dirty it again each time)
            else:
                fn = (lambda: br.observe(batch, st))
            say(f"| {M} | {what} | {stat(events(fn, a.reps))} |")
            del br
    say()
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
