#!/usr/bin/env python3
"""What the reply cache (ops/reply_cache.py, csrc/hip/reply_cache.hip) costs and saves.

Every row compares the plain Send with the cached Send of the same batch, the two
alternating inside one process (the baseline is always the plain Send of this run),
world 1, eager ``send_all``:

1.  ``Calculator.Multiply`` at each ``--msgs`` size, keys that all have a slot of
    their own: the cold Send (the cache cleared before it: all misses), the all-hit
    Send and a 50 % hit Send (cleared, then the hit half warmed, before every timed
    call), with the cold Send's steps timed on their own -- lookup, claim and write
    with device events around ``--reps`` launches, the selection with a host clock
    (it ends in the host read of K).
2.  ``Prime.Check`` with a per-candidate delay (``--delay-us``): the first Send
    against the repeat Send, and ``--zipf-sends`` Sends of Zipf-repeated keys.
3.  Hit rate and time against ``cache_entries`` for a set of ``--keys`` keys.

    python tools/reply_cache_cost.py [--msgs 1048576 8388608] [--iters 20] [--reps 10] [--delay-us 2 50 250] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import coalesce as CO  # noqa: E402
from ptype_amd.ops import hip, raw_stream  # noqa: E402
from ptype_amd.ops import reply_cache as RC  # noqa: E402
from ptype_amd.ops import retry as RT  # noqa: E402
from ptype_amd.ops.batch import MsgBatch, gen_zipf_requests  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_PRIME_CHECK, STATUS_OK  # noqa: E402
from ptype_amd.ops.table import RegistryTable, actor_keys  # noqa: E402
from ptype_amd.parallel.exchange import ActorExchange  # noqa: E402

ACTORS = 1 << 20


def table(n: int, dev) -> RegistryTable:
    tab = RegistryTable(2 * n, device=dev)
    ids = torch.arange(n)
    tab.upsert(actor_keys(ids), torch.zeros(n, dtype=torch.int32), ids.to(torch.int32))
    tab.enable_directory(n, affine_world=1)
    return tab


def key_batch(k: torch.Tensor, method: int) -> MsgBatch:
    """The messages of key numbers ``k`` (int64, on any device): distinct per number."""
    actor = (k % ACTORS).to(torch.int32)
    if method == METHOD_PRIME_CHECK:  # first divisor of n in [2, 10): n = 1009 + 2 k
        return MsgBatch(actor, torch.full_like(k, 2), torch.full_like(k, 10), 1009 + 2 * k, method)
    return MsgBatch(actor, k - 12345, (k * 7 + 3) & 0xFFFF, None, method)


def own_slot_keys(count: int, entries: int, method: int, first: int = 0) -> torch.Tensor:
    """``count`` key numbers from ``first`` on whose keys fall into pairwise different
    slots of a table of ``entries`` (the host mirror of the device hash picks them)."""
    got, lo, taken = [], first, np.zeros(entries, dtype=bool)
    while sum(x.size for x in got) < count:
        k = torch.arange(lo, lo + (1 << 20))
        b = key_batch(k, method)
        z = np.zeros(k.numel(), dtype=np.int64)
        slot = (CO.key_hash(b.actor.numpy(), method, b.a0.numpy(), b.a1.numpy(), z if b.a2 is None else b.a2.numpy())
                & np.uint64(entries - 1)).astype(np.int64)
        idx = np.sort(np.unique(slot, return_index=True)[1])
        idx = idx[~taken[slot[idx]]]
        taken[slot[idx]] = True
        got.append(k.numpy()[idx])
        lo += 1 << 20
    return torch.from_numpy(np.concatenate(got)[:count])


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


def alternate(variants, iters: int, prep=None) -> dict:
    """Host clock around each variant + a device synchronise, the variants alternating;
    ``prep(name)`` runs untimed (and synchronised) before each call."""
    ts = {name: [] for name, _ in variants}
    for it in range(iters + 3):  # 3 warm-up rounds
        for name, fn in variants:
            if prep is not None:
                prep(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 3:
                ts[name].append((time.perf_counter() - t0) * 1e6)
    return ts


def check(out, want, what: str) -> None:
    torch.cuda.synchronize()
    if not torch.equal(out[0], want[0]) or not torch.equal(out[1], want[1]):
        raise RuntimeError(f"reply_cache_cost: {what}: the cached Send's replies differ from the plain Send's")


def multiply(M: int, iters: int, reps: int, dev) -> list[str]:
    entries = 1 << max(22, (4 * M - 1).bit_length())
    ex = ActorExchange(table(ACTORS, dev), M, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev))
    cache = RC.ReplyCache(dev, entries)
    keys = own_slot_keys(M, entries, METHOD_CALC_MULTIPLY)
    g = torch.Generator().manual_seed(1)
    b = key_batch(keys[torch.randperm(M, generator=g)].to(dev), METHOD_CALC_MULTIPLY)
    half = b.slice(0, M // 2)
    want = ex.send_all(b)
    plain = ("plain", lambda: ex.send_all(b))
    cached = ("cached", lambda: cache.send(b, ex.send_all))
    lines = [f"### Calculator.Multiply, M = {M}, {M} distinct keys with a slot of their own in {entries} entries "
             f"({entries * 64 >> 20} MiB)", "",
             "| Send | hits | plain Send us | cached Send us | cached / plain |", "|---|---|---|---|---|"]

    def row(name, prep):
        prep("cached")
        c0 = cache.counters["hits"]
        check(cache.send(b, ex.send_all), want, name)
        hits = cache.counters["hits"] - c0
        ts = alternate([plain, cached], iters, prep)
        ratio = statistics.median(ts["cached"]) / statistics.median(ts["plain"])
        lines.append(f"| {name} | {hits} | {stat(ts['plain'])} | {stat(ts['cached'])} | {ratio:.2f} |")

    def cold(name):
        if name == "cached":
            cache.clear()

    def half_warm(name):
        if name == "cached":
            cache.clear()
            cache.send(half, ex.send_all)

    row("cold (all misses)", cold)
    row("50 % hits", half_warm)
    cache.clear()
    cache.send(b, ex.send_all)
    row("all hits", lambda name: None)
    # the cold Send's steps
    cache.clear()
    _, st = cache.lookup(b)
    sub, _, K = RT.select_mask(b, st, 1 << RC.PENDING)
    v2, s2 = ex.send_all(b)
    args, keep = cache._key_args(b)
    ins = (lambda ph: hip().reply_cache_insert_phase(*args, M, v2.data_ptr(), s2.data_ptr(), cache.table.data_ptr(),
                                                     cache.log2, cache.epoch, cache.seq, ph, raw_stream(dev)))
    look = events(lambda: cache.lookup(b), reps)
    sel = alternate([("select", lambda: RT.select_mask(b, st, 1 << RC.PENDING))], iters)["select"]
    inner = events(lambda: ex.send_all(b), reps)
    claim = events(lambda: ins(1), reps)
    write = events(lambda: ins(2), reps)
    cache.clear()
    cache.send(b, ex.send_all)
    look_hit = events(lambda: cache.lookup(b), reps)
    del keep
    return lines + ["", f"the cold Send's steps (K = {K}): lookup {stat(look)} us, select (with the allocation of the "
                    f"sub-batch and the host read) {stat(sel)} us, inner Send {stat(inner)} us, claim {stat(claim)} us, "
                    f"write {stat(write)} us; the all-hit lookup {stat(look_hit)} us", ""]


def prime(M: int, delay_us: int, iters: int, zipf_sends: int, dev) -> list[str]:
    entries = 1 << 22
    ex = ActorExchange(table(ACTORS, dev), M, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev),
                       delay_us=delay_us)
    cache = RC.ReplyCache(dev, entries)
    K = max(1, M // 10)  # duplicate share 0.9, as profiles/coalesce.md
    keys = own_slot_keys(K, entries, METHOD_PRIME_CHECK)
    g = torch.Generator().manual_seed(2)
    pick = torch.cat([torch.arange(K), torch.randint(0, K, (M - K,), generator=g)])[torch.randperm(M, generator=g)]
    b = key_batch(keys[pick].to(dev), METHOD_PRIME_CHECK)
    want = ex.send_all(b)
    lines = [f"### Prime.Check, delay_us = {delay_us} per candidate (at most 8 candidates per call), M = {M}, "
             f"{K} distinct keys", "", "| Send | hits | plain Send us | cached Send us | cached / plain |",
             "|---|---|---|---|---|"]
    plain = ("plain", lambda: ex.send_all(b))
    cached = ("cached", lambda: cache.send(b, ex.send_all))
    for name, prep in (("first (cold)", lambda n: cache.clear() if n == "cached" else None), ("repeat", lambda n: None)):
        prep("cached")
        c0 = cache.counters["hits"]
        check(cache.send(b, ex.send_all), want, name)
        hits = cache.counters["hits"] - c0
        ts = alternate([plain, cached], iters, prep)
        ratio = statistics.median(ts["cached"]) / statistics.median(ts["plain"])
        lines.append(f"| {name} | {hits} | {stat(ts['plain'])} | {stat(ts['cached'])} | {ratio:.2f} |")
    # Zipf-repeated keys: every Send draws its keys afresh, the popular ones come back
    cache.clear()
    lines += ["", f"{zipf_sends} Sends of keys drawn Zipf(1.1) from {ACTORS}, a cold cache before the first:", "",
              "| Send | hits | plain Send us | cached Send us | cached / plain |", "|---|---|---|---|---|"]
    for s in range(zipf_sends):
        z = gen_zipf_requests(M, ACTORS, s=1.1, seed=90 + s, device=dev)
        zb = key_batch(z.actor.to(torch.int64), METHOD_PRIME_CHECK)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zw = ex.send_all(zb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        c0 = cache.counters["hits"]
        out = cache.send(zb, ex.send_all)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        check(out, zw, f"zipf Send {s}")
        lines.append(f"| {s} | {cache.counters['hits'] - c0} | {(t1 - t0) * 1e6:.1f} | {(t2 - t1) * 1e6:.1f} | "
                     f"{(t2 - t1) / (t1 - t0):.2f} |")
    return lines + [""]


def sizes(nkeys: int, iters: int, dev) -> list[str]:
    ex = ActorExchange(table(ACTORS, dev), nkeys, state=torch.zeros(ACTORS, dtype=torch.int64, device=dev))
    g = torch.Generator().manual_seed(3)
    b = key_batch((torch.randperm(nkeys, generator=g) + (1 << 24)).to(dev), METHOD_CALC_MULTIPLY)
    want = ex.send_all(b)
    lines = [f"### hit rate against cache_entries: {nkeys} distinct Calculator.Multiply keys, one message each, the "
             "same batch again and again", "",
             "| cache_entries | MiB | hit rate of a repeat Send | plain Send us | cached repeat Send us | cached / plain |",
             "|---|---|---|---|---|---|"]
    for log2 in range(16, 27, 2):
        cache = RC.ReplyCache(dev, 1 << log2)
        for _ in range(2):
            check(cache.send(b, ex.send_all), want, f"entries 1 << {log2}")
        c0 = dict(cache.counters)
        ts = alternate([("plain", lambda: ex.send_all(b)), ("cached", lambda: cache.send(b, ex.send_all))], iters)
        rate = (cache.counters["hits"] - c0["hits"]) / (cache.counters["messages"] - c0["messages"])
        ratio = statistics.median(ts["cached"]) / statistics.median(ts["plain"])
        lines.append(f"| 1 << {log2} | {64 << log2 >> 20} | {rate:.3f} | {stat(ts['plain'])} | {stat(ts['cached'])} | "
                     f"{ratio:.2f} |")
        del cache
    return lines + [""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, nargs="*", default=[1 << 20, 8 << 20])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--delay-us", type=int, nargs="*", default=[2, 50, 250])
    ap.add_argument("--prime-msgs", type=int, default=1 << 18)
    ap.add_argument("--zipf-sends", type=int, default=8)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("reply_cache_cost: no GPU", file=sys.stderr)
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
          "plain and cached alternating in one process, host clock around the Send + a device synchronise; lookup, "
          f"claim and write: device events around {a.reps} launches.  Cells: median (min .. max).", ""])
    for M in a.msgs:
        emit(multiply(M, a.iters, a.reps, dev))
    for d in a.delay_us:
        emit(prime(a.prime_msgs, d, max(3, a.iters // 4), a.zipf_sends, dev))
    if a.keys > 0:
        emit(sizes(a.keys, a.iters, dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
