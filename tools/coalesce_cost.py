#!/usr/bin/env python3
"""What coalescing (ops/coalesce.py, csrc/hip/coalesce.hip) costs and saves.

Three measurements, each comparing the plain Send with the coalesced Send of the
same batches, alternating inside one process (the baseline is always the plain
Send of this run):

1.  World 1, eager ``send_all`` of ``Calculator.Multiply`` batches whose share of
    duplicate messages is 0, 0.5, 0.9 or everything (one key), at each ``--msgs``
    size: host clock around the Send + a device synchronise, medians with min /
    max.  The three passes are timed on their own -- grouping and fan-out with
    device events around ``--reps`` launches, the selection with a host clock (it
    ends in the host read of K) -- next to a bare 4-byte device-to-host read.
2.  ``Prime.Check`` with a per-candidate delay (``--delay-us``), duplicate share 0.9.
3.  ``--loopback`` in-process ranks (FakeComm), Zipf actor ids and arguments from a
    small range: wire bytes per message and re-send rounds with and without
    coalescing.

    python tools/coalesce_cost.py [--msgs 1048576 8388608] [--iters 20] [--reps 10] [--loopback 8] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import coalesce as CO  # noqa: E402
from ptype_amd.ops import hip  # noqa: E402
from ptype_amd.ops.batch import MsgBatch, gen_zipf_requests  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_PRIME_CHECK  # noqa: E402
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402

ACTORS = 1 << 20
SHARES = (("0", 0.0), ("0.5", 0.5), ("0.9", 0.9), ("all identical", None))


def dup_batch(M: int, share, dev, seed: int, method=METHOD_CALC_MULTIPLY) -> tuple[MsgBatch, int]:
    """M messages over K = M * (1 - share) distinct keys (every key at least once,
    the rest drawn uniformly, shuffled); ``share`` None: one key."""
    g = torch.Generator(device=dev).manual_seed(seed)
    K = 1 if share is None else max(1, round(M * (1.0 - share)))
    pick = torch.cat([torch.arange(K, device=dev), torch.randint(0, K, (M - K,), device=dev, generator=g)])
    pick = pick[torch.randperm(M, device=dev, generator=g)]
    actor = torch.randint(0, ACTORS, (K,), device=dev, generator=g).to(torch.int32)
    if method == METHOD_PRIME_CHECK:  # first divisor of n in [2, 10): n = 1009 + 2 k, distinct per key
        n = 1009 + 2 * torch.arange(K, device=dev)
        return MsgBatch(actor[pick], torch.full((M,), 2, dtype=torch.int64, device=dev),
                        torch.full((M,), 10, dtype=torch.int64, device=dev), n[pick], method), K
    a0 = torch.arange(K, device=dev) - K // 2  # distinct per key
    a1 = torch.randint(0, 0x10000, (K,), device=dev, generator=g)
    return MsgBatch(actor[pick], a0[pick], a1[pick], None, method), K


def table(n: int, world: int, dev) -> RegistryTable:
    tab = RegistryTable(2 * n, device=dev)
    ids = torch.arange(n)
    tab.upsert(actor_keys(ids), (ids % world).to(torch.int32), (ids // world).to(torch.int32))
    tab.enable_directory(n, affine_world=world)
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
    for _ in range(3):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(iters):  # the variants alternate: drift hits all alike
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e6)
    return ts


def world1(M: int, iters: int, reps: int, dev, method=METHOD_CALC_MULTIPLY, delay_us: int = 0, shares=SHARES):
    ex = ActorExchange(table(ACTORS, 1, dev), M, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev),
                       delay_us=delay_us)
    co = CO.Coalescer(dev, M)
    lines = ["| duplicate share | K | plain Send us | coalesced Send us | coalesced / plain | group us | select us "
             "(with the host read) | fan-out us |", "|---|---|---|---|---|---|---|---|"]
    for i, (name, share) in enumerate(shares):
        b, K = dup_batch(M, share, dev, 10 + i, method)
        want = ex.send_all(b)
        co.counters.update(sends=0, messages=0, executed=0)
        (val, st), _ = co.send(b, ex.send_all)
        torch.cuda.synchronize()
        if not torch.equal(val, want[0]) or not torch.equal(st, want[1]) or co.counters["executed"] != K:
            raise RuntimeError("coalesce_cost: the coalesced Send's replies differ from the plain Send's")
        ts = alternate([("plain", lambda: ex.send_all(b)), ("coalesce", lambda: co.send(b, ex.send_all))], iters)
        lead = CO.group(b, co)
        sub, _, pos, _ = CO.select(b, lead)
        v2, s2 = ex.send_all(sub)
        grp = events(lambda: CO.group(b, co), reps)
        fan = events(lambda: CO.fanout(lead, pos, v2, s2), reps)
        sel = alternate([("select", lambda: CO.select(b, lead))], iters)["select"]
        ratio = statistics.median(ts["coalesce"]) / statistics.median(ts["plain"])
        lines.append(f"| {name} | {K} | {stat(ts['plain'])} | {stat(ts['coalesce'])} | {ratio:.2f} | {stat(grp)} | "
                     f"{stat(sel)} | {stat(fan)} |")
    return lines + [""]


def host_read(dev, iters: int) -> str:
    k = torch.ones(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(iters, 20)):
        t0 = time.perf_counter()
        k.item()
        ts.append((time.perf_counter() - t0) * 1e6)
    return stat(ts)


def loopback(R: int, M: int, iters: int, dev) -> list[str]:
    n = 1 << 16
    fc = hip().FakeComm(R)
    out, errors = [None] * R, []
    start = threading.Barrier(R)

    def run(r):
        try:
            torch.cuda.set_device(dev)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                ex = ActorExchange(table(n, R, dev), M, chunks=1,
                                   state=torch.zeros(n // R, dtype=torch.int64, device=dev), fake=(fc, r))
                co = CO.Coalescer(dev, M)
                z = gen_zipf_requests(M, n, s=1.1, seed=70 + r, device=dev)
                b = MsgBatch(z.actor, z.a0 & 3, z.a1 & 3, None, METHOD_CALC_MULTIPLY)  # a small argument range
                res = {}
                start.wait(timeout=120)
                for name, fn in (("plain", lambda: ex.send_all(b)), ("coalesce", lambda: co.send(b, ex.send_all))):
                    fn()
                    s.synchronize()
                    c0 = (ex.counters.wire_bytes, ex.counters.resends)
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        fn()
                    s.synchronize()
                    res[name] = ((ex.counters.wire_bytes - c0[0]) / (iters * M), (ex.counters.resends - c0[1]) / iters,
                                 (time.perf_counter() - t0) * 1e6 / iters)
                res["K"] = co.counters["executed"] / max(co.counters["sends"], 1)
                out[r] = res
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append((r, repr(e)))
            start.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    if errors or any(t.is_alive() for t in threads):
        raise RuntimeError(f"coalesce_cost: loopback failed: {errors}")
    lines = [f"### {R} in-process ranks (FakeComm), {M} messages per rank and Send, Zipf(1.1) ids over {n} actors, "
             "arguments in [0, 4)", "",
             "| rank | leaders per Send (K) | plain: wire B / message | re-send rounds / Send | us / Send | coalesced: wire B "
             "/ message | re-send rounds / Send | us / Send |", "|---|---|---|---|---|---|---|---|"]
    for r, res in enumerate(out):
        p, c = res["plain"], res["coalesce"]
        lines.append(f"| {r} | {res['K']:.0f} | {p[0]:.2f} | {p[1]:.2f} | {p[2]:.0f} | {c[0]:.2f} | {c[1]:.2f} | {c[2]:.0f} |")
    return lines + ["", "(wire bytes are per message of the caller's batch, M; the us / Send of in-process ranks share one "
                    "GPU and one interpreter: a ratio, not a Send time)", ""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="*", default=[1 << 20, 8 << 20])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--delay-us", type=int, default=2)
    ap.add_argument("--prime-msgs", type=int, default=1 << 18)
    ap.add_argument("--loopback", type=int, default=8)
    ap.add_argument("--loopback-msgs", type=int, default=1 << 18)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("coalesce_cost: no GPU", file=sys.stderr)
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

    emit([f"world 1, eager `send_all` over {ACTORS} actors; {a.iters} timed calls per variant after 3 warm-up rounds, "
          "plain and coalesced alternating in one process, host clock around the Send + a device synchronise; "
          f"group and fan-out: device events around {a.reps} launches.  Cells: median (min .. max).", ""])
    for M in a.msgs:
        emit([f"### Calculator.Multiply, M = {M}", ""] + world1(M, a.iters, a.reps, dev))
    emit([f"a bare 4-byte device-to-host read of a ready value: {host_read(dev, a.iters)} us", ""])
    if a.delay_us > 0:
        emit([f"### Prime.Check, delay_us = {a.delay_us} per candidate (at most 8 candidates per call), "
              f"M = {a.prime_msgs}", ""] +
             world1(a.prime_msgs, max(3, a.iters // 4), a.reps, dev, METHOD_PRIME_CHECK, a.delay_us, (SHARES[2],)))
    if a.loopback > 1:
        emit(loopback(a.loopback, a.loopback_msgs, max(3, a.iters // 2), dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
