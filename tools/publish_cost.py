#!/usr/bin/env python3
"""What publish/subscribe topics (ops/topics.py, the ``topics`` rule of csrc/hip/scatter.hip) cost.

1.  Expansion alone: ``--rows`` rows from ``--pubs`` publications, one strided segment per
    topic, against the ``members`` rule producing the identical rows from a CSR of one
    int32 per subscriber (the baseline: its kernels are unchanged).  The two expand launches,
    and the count + scan + first launches, by device events, the variants alternating in
    one process; the baseline is in the rotation twice, and the difference between its two
    series is the run-to-run spread the comparison is read against.  The columns are
    compared for exact equality before anything is timed.
2.  The worst case: the same rows from segments of length 1 (one segment per subscriber),
    reported as the ratio to case 1.  No threshold.
3.  End to end through a one-member ``Join``: ``Client.Publish`` against ``Client.Ask`` with a
    hand-built members CSR of the same rows, on a quiet table (``apply()`` is the follower's
    two loads).  Host clock around the call plus a device synchronise, alternating.

    python tools/publish_cost.py [--rows N] [--pubs Q] [--iters 10] [--reps 10] [--md FILE] [--no-join]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import scatter as S  # noqa: E402
from ptype_amd.ops import topics as T  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY  # noqa: E402

ACTORS = 1 << 20


def stat(ts) -> str:
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def alternate_events(variants, iters: int, reps: int) -> dict:
    """us per call by device events around ``reps`` calls, the variants alternating, ``iters``
    groups per variant after two warm-up groups."""
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


def case(rows: int, pubs: int, unit: bool, dev, n_actors: int = ACTORS):
    """``pubs`` topics of ``rows // pubs`` subscribers each: topic g is the progression
    ``g % stride_g + stride_g * k`` below ``n_actors``; ``unit``: as segments of length 1.  Returns
    (topics Scatter, members Scatter, publications)."""
    per = rows // pubs
    gen = torch.Generator().manual_seed(11)
    stride = torch.randint(1, max(n_actors // per, 2), (pubs,), generator=gen)
    start = torch.randint(0, 1 << 30, (pubs,), generator=gen) % stride
    ids = (start[:, None] + stride[:, None] * torch.arange(per)[None, :]).reshape(-1)
    if unit:
        flat = {"seg_off": np.arange(pubs + 1, dtype=np.int64) * per, "row_off": np.arange(pubs * per + 1, dtype=np.int64),
                "seg_start": ids.numpy().astype(np.int32), "seg_stride": np.ones(pubs * per, dtype=np.int32)}
    else:
        flat = {"seg_off": np.arange(pubs + 1, dtype=np.int64), "row_off": np.arange(pubs + 1, dtype=np.int64) * per,
                "seg_start": start.numpy().astype(np.int32), "seg_stride": stride.numpy().astype(np.int32)}
    table = T.TopicTable(dev, max_topics=pubs)
    table.load(flat)
    offsets = (torch.arange(pubs + 1, dtype=torch.int64) * per).to(dev)
    sc_t = S.Scatter.topics(table, capacity=pubs * per, q_capacity=pubs)
    sc_m = S.Scatter.members(offsets, ids.to(torch.int32).to(dev), capacity=pubs * per, q_capacity=pubs)
    qs = MsgBatch(torch.randperm(pubs, generator=gen).to(torch.int32).to(dev),
                  torch.randint(-2**31, 2**31, (pubs,), generator=gen).to(dev),
                  torch.randint(-2**31, 2**31, (pubs,), generator=gen).to(dev), None, METHOD_CALC_MULTIPLY)
    return sc_t, sc_m, qs


def equal_or_die(a: S.Expansion, b: S.Expansion, what: str) -> None:
    torch.cuda.synchronize()
    for name, x, y in (("actor", a.batch.actor, b.batch.actor), ("a0", a.batch.a0, b.batch.a0), ("a1", a.batch.a1, b.batch.a1),
                       ("group", a.group, b.group), ("first", a.first, b.first), ("n", a.n, b.n)):
        if not torch.equal(x, y):
            raise RuntimeError(f"publish_cost: {what}: column {name} differs between the topics and the members rule")


def expansion(rows: int, pubs: int, iters: int, reps: int, dev) -> list[str]:
    lines = ["### expansion alone: the `topics` rule against the `members` rule producing the identical rows", "",
             "| table | Q | rows | segments | topics expand launch us | members expand launch us | members again us | "
             "baseline spread (median - median) us | topics - members us | topics count+scan+first us | "
             "members count+scan+first us |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    medians = {}
    for label, unit in (("one strided segment per topic", False), ("all segments of length 1", True)):
        sc_t, sc_m, qs = case(rows, pubs, unit, dev)
        et, em = sc_t.expand(qs), sc_m.expand(qs)
        equal_or_die(et, em, label)
        Q, total = et.Q, et.total
        cols = (qs.actor, qs.a0, qs.a1, None, None)
        ts = alternate_events([("members", lambda: sc_m._fill(cols, Q, total)), ("topics", lambda: sc_t._fill(cols, Q, total)),
                               ("members again", lambda: sc_m._fill(cols, Q, total))], iters, reps)
        tc = alternate_events([("members", lambda: sc_m._count(cols, Q)), ("topics", lambda: sc_t._count(cols, Q))],
                              iters, reps)
        med = {k: statistics.median(v) for k, v in ts.items()}
        medians[unit] = med["topics"]
        lines.append(f"| {label} | {Q} | {total} | {sc_t.table.host['seg_start'].size} | {stat(ts['topics'])} | "
                     f"{stat(ts['members'])} | {stat(ts['members again'])} | {med['members again'] - med['members']:+.1f} | "
                     f"{med['topics'] - med['members']:+.1f} | {stat(tc['topics'])} | {stat(tc['members'])} |")
        print(lines[-1], flush=True)
        del sc_t, sc_m, et, em
        torch.cuda.empty_cache()
    lines += ["", f"Worst case over case 1 (expand launch, median / median): {medians[True] / medians[False]:.2f}", ""]
    print(lines[-2], flush=True)
    return lines


def end_to_end(rows: int, pubs: int, iters: int) -> list[str]:
    """Client.Publish against Client.Ask(members CSR) through a one-member Join."""
    import socket

    from ptype_amd import cluster as C
    from ptype_amd.models import calculator

    def port():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            return s.getsockname()[1]

    os.environ.setdefault("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    lines = ["### end to end: `Client.Publish` against `Client.Ask` with a hand-built members CSR, quiet table", "",
             "| Q | rows | Ask us | Publish us | Ask again us | baseline spread us | Publish - Ask us |", "|---|---|---|---|---|---|---|"]
    with tempfile.TemporaryDirectory() as tmp:
        pp, pc = port(), port()
        cfg = C.Config()
        cfg.service_name, cfg.node_name, cfg.port = "calculator", "gpu0", port()
        cfg.member = C.member_config(name="m0", dir=os.path.join(tmp, "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                     apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                     acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                     heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
        cfg.has_gpu = True
        cfg.gpu.device, cfg.gpu.actors, cfg.gpu.max_batch, cfg.gpu.topics = 0, ACTORS, rows, max(pubs, 1)
        c = C.Join(C.background(), cfg)
        server = C.Server()
        try:
            calculator.serve_device(c.runtime, server)
            server.Listen(cfg.port, "127.0.0.1")
            client = c.NewClient("calculator", C.ConnConfig())
            dev = c.runtime.device
            sc_t, sc_m, qs = case(rows, pubs, False, dev, n_actors=c.runtime.total_actors)
            h = sc_t.table.host
            per = rows // pubs
            for g in range(pubs):  # the same topics through the store: one record per topic
                client.Subscribe(g, segments=[[int(h["seg_start"][g]), per, int(h["seg_stride"][g])]])
            pub, ask = client.Publish(qs), client.Ask(qs, sc_m)
            torch.cuda.synchronize()
            if not (torch.equal(pub.val, ask.val) and torch.equal(pub.value, ask.value) and torch.equal(pub.count, ask.count)):
                raise RuntimeError("publish_cost: Publish and Ask(members) differ")
            ts = alternate_host([("ask", lambda: client.Ask(qs, sc_m)), ("publish", lambda: client.Publish(qs)),
                                 ("ask again", lambda: client.Ask(qs, sc_m))], iters)
            med = {k: statistics.median(v) for k, v in ts.items()}
            st = c.Stats()["runtime"]["topics"]
            lines.append(f"| {pubs} | {pub.val.numel()} | {stat(ts['ask'])} | {stat(ts['publish'])} | {stat(ts['ask again'])} | "
                         f"{med['ask again'] - med['ask']:+.1f} | {med['publish'] - med['ask']:+.1f} |")
            print(lines[-1], flush=True)
            lines += ["", f"Table uploads during the timed Publishes: {c.runtime.topics().uploads} in all "
                          f"(records {st['records']}, publishes {st['publishes']}).", ""]
            client.Close()
        finally:
            server.Close()
            c.Close()
    return lines


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--pubs", type=int, default=8192)
    ap.add_argument("--e2e-rows", type=int, default=1 << 18)
    ap.add_argument("--e2e-pubs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-join", action="store_true", help="skip the end-to-end section")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("publish_cost: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = []

    def emit(new):  # written section by section: a failure later keeps what was measured
        lines.extend(new)
        if a.md:
            os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
            with open(a.md, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit([f"One MI355X, profiler off.  The launches: device events around {a.reps} calls, {a.iters} groups per variant "
          "after 2 warm-up groups, the variants alternating in one process, the baseline twice in the rotation.  Publish "
          f"and Ask: host clock around the call + a device synchronise, {max(5, a.iters)} rounds after 3 warm-up rounds.  "
          "The columns compared for exact equality first.  Cells: median (min .. max).", ""])
    emit(expansion(a.rows, a.pubs, a.iters, a.reps, dev))
    if not a.no_join:
        emit(end_to_end(a.e2e_rows, a.e2e_pubs, max(5, a.iters)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
