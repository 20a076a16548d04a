#!/usr/bin/env python3
"""What the Send ledger (ops/ledger.py, csrc/hip/ledger.hip) adds to a Send.

Eager world-1 ``send_all`` of pre-generated ``Calculator.Multiply`` batches on one
GPU, at each size in four variants that alternate inside one process:

    off        no ledger (the Send as it was)
    ledger     a ledger without the per-actor load table
    load       a ledger with the load table, uniform actor ids
    zipf-off   no ledger, ``zipf_actors(s=1.1)`` ids
    zipf-load  a ledger with the load table, the same Zipf ids

Every call is timed with a host clock around ``send_all`` + a device synchronise,
after warm-up; the table gives medians with min / max as the spread.  The
accounting kernel alone is timed with device events around ``--reps`` launches
back to back, and its rate is the bytes the pass needs (12 B of status + value
per message, 16 B of a0 + a1 for the audit, 4 B of actor ids with a load table)
over that time.  On a tree without ``ptype_amd.ops.ledger`` only the two ledger-off
rows are measured: the yardstick for the same Send before the feature.

    python tools/ledger_cost.py [--msgs 1048576 8388608] [--iters 40] [--reps 20] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import batch as B  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_OK  # noqa: E402
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402

try:
    from ptype_amd.ops.ledger import Ledger
except ImportError:  # the tree before the feature: ledger-off rows only
    Ledger = None

ACTORS = 1 << 20


def measure(M: int, iters: int, reps: int, dev) -> list[str]:
    tab = RegistryTable(2 * ACTORS, device=dev)
    ids = torch.arange(ACTORS)
    tab.upsert(actor_keys(ids), torch.zeros(ACTORS, dtype=torch.int32), ids.to(torch.int32))
    tab.enable_directory(ACTORS)
    ex = ActorExchange(tab, M, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev))
    uni = B.gen_requests(M, ACTORS, METHOD_CALC_MULTIPLY, seed=1, device=dev)
    zipf = B.gen_zipf_requests(M, ACTORS, s=1.1, seed=2, device=dev)
    out = (torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, dtype=torch.int32, device=dev))
    variants = [("off", uni, None), ("zipf-off", zipf, None)]
    if Ledger is not None:
        plain, load = Ledger(dev), Ledger(dev, actors=ACTORS)
        variants = [("off", uni, None), ("ledger", uni, plain), ("load", uni, load), ("zipf-off", zipf, None),
                    ("zipf-load", zipf, load)]

    def send(batch, led):
        if led is None:
            return ex.send_all(batch, out=out)
        return ex.send_all(batch, out=out, ledger=led)

    for _ in range(5):
        for _, batch, led in variants:
            val, st = send(batch, led)
    torch.cuda.synchronize()
    if not bool((st == STATUS_OK).all()) or not torch.equal(val, zipf.a0 * zipf.a1):
        raise RuntimeError("ledger_cost: wrong replies")
    ts = {name: [] for name, _, _ in variants}
    for _ in range(iters):  # the variants alternate: drift hits all alike
        for name, batch, led in variants:
            t0 = time.perf_counter()
            send(batch, led)
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e6)
    med = {k: statistics.median(v) for k, v in ts.items()}
    base = {"off": "off", "ledger": "off", "load": "off", "zipf-off": "zipf-off", "zipf-load": "zipf-off"}
    lines = [f"### M = {M} messages", "",
             "| variant | Send median us | min us | max us | added us (median - its ledger-off median) |",
             "|---|---|---|---|---|"]
    for name, _, _ in variants:
        added = "" if base[name] == name else f"{med[name] - med[base[name]]:+.1f}"
        lines.append(f"| {name} | {med[name]:.1f} | {min(ts[name]):.1f} | {max(ts[name]):.1f} | {added} |")
    if Ledger is not None:
        lines += ["", "| accounting kernel alone | us per launch | bytes per message | GB/s |", "|---|---|---|---|"]
        for name, batch, led, nbytes in (("ledger", uni, plain, 28), ("load", uni, load, 32),
                                         ("zipf-load", zipf, load, 32)):
            val, st = send(batch, None)  # this batch's replies
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                led.account(batch, val, st)
            per = []
            for _ in range(5):
                e0.record()
                for _ in range(reps):
                    led.account(batch, val, st)
                e1.record()
                e1.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / reps)
            us = statistics.median(per)
            lines.append(f"| {name} | {us:.1f} (min {min(per):.1f}, max {max(per):.1f}) | {nbytes} | "
                         f"{M * nbytes / us / 1e3:.0f} |")
        r = load.read(top=1)
        lines += ["", f"(load ledger afterwards: sends {r['sends']}, mismatch {r['mismatch']}, load_oob {r['load_oob']}, "
                  f"busiest actor {r['hot'][0][0]} with {r['hot'][0][1]} messages)"]
        if r["mismatch"] or r["load_oob"]:
            raise RuntimeError("ledger_cost: the ledger saw mismatches")
    return lines + [""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="+", default=[1 << 20, 8 << 20])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("ledger_cost: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = [f"world 1, eager `send_all` of pre-generated Calculator.Multiply batches over {ACTORS} actors; "
             f"{a.iters} timed calls per variant after 5 warm-up rounds, variants alternating in one process, host clock "
             "around the Send + a device synchronise; " +
             ("ledger variants included." if Ledger is not None else "a tree without the ledger: ledger-off rows only."),
             ""]
    for M in a.msgs:
        lines += measure(M, a.iters, a.reps, dev)
    text = "\n".join(lines)
    print(text)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
