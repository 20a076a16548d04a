#!/usr/bin/env python3
"""What topic queue subscriptions (the QUEUES variant of the ``topics`` rule, csrc/hip/scatter.hip) cost.

The method of ``tools/publish_cost.py`` (whose helpers this uses): the variants alternate in
one process, the baseline is in the rotation twice so that its own spread is the margin the
comparison is read against, and the columns are compared for exact equality before anything
is timed.

a.  A table WITHOUT a queue subscription, at ``publish_cost.py``'s shape (``--rows`` rows from
    ``--pubs`` publications, one strided segment per topic): its expand launch, twice in the
    rotation -- it launches the instantiation the ``topics`` rule always launched (the dispatch
    in ``launch_scatter_expand`` takes the QUEUES kernels only for ``n_queues >= 1``), so this
    number stands next to ``profiles/topics.md``'s -- and the same table with ONE queue
    subscription on a topic nobody publishes to, which produces the identical rows through the
    QUEUES kernel: what the variant costs ordinary rows.
b.  Queue rows: ``--qpubs`` publications to topics with only queue subscriptions (8 per topic,
    1024 members each), as one segment per subscription and as 1024 segments of length 1,
    against the ``members`` rule producing the identical rows from a host-built CSR of one
    group per publication.
c.  Count + scan + first for every table above.

    python tools/queue_cost.py [--rows N] [--pubs Q] [--qpubs Q] [--iters 10] [--reps 10] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from publish_cost import alternate_events, case, equal_or_die, stat  # noqa: E402

from ptype_amd.ops import scatter as S  # noqa: E402
from ptype_amd.ops import topics as T  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY  # noqa: E402

SUBS_PER_TOPIC, MEMBERS = 8, 1024


def without_queues(rows: int, pubs: int, iters: int, reps: int, dev) -> list[str]:
    lines = ["### (a) a table without a queue subscription, and the same rows through the QUEUES kernel", "",
             "| Q | rows | topics expand us | topics expand again us | baseline spread (median - median) us | "
             "same rows, one unused queue subscription (QUEUES kernel) us | QUEUES - topics us | topics count+scan+first us | "
             "QUEUES count+scan+first us |", "|---|---|---|---|---|---|---|---|---|"]
    sc_t, _, qs = case(rows, pubs, False, dev)
    # one more topic, which nobody publishes to, holds the queue subscription
    h = sc_t.table.host
    flat = {"seg_off": np.concatenate([h["seg_off"], h["seg_off"][-1:]]), "row_off": np.concatenate([h["row_off"], h["row_off"][-1:] + 4]),
            "seg_start": np.concatenate([h["seg_start"], [7]]), "seg_stride": np.concatenate([h["seg_stride"], [1]]),
            "q_off": np.concatenate([np.zeros(pubs + 1, dtype=np.int64), [1]]),
            "q_seg": np.asarray([h["seg_start"].size, h["seg_start"].size + 1], dtype=np.int64)}
    tq = T.TopicTable(dev, max_topics=pubs + 1)
    tq.load(flat)
    sc_q = S.Scatter.topics(tq, capacity=sc_t.capacity, q_capacity=pubs)
    assert tq.n_queues == 1 and sc_t.table.n_queues == 0
    et, eq = sc_t.expand(qs), sc_q.expand(qs)
    equal_or_die(et, eq, "no queue subscription against an unused one")
    Q, total = et.Q, et.total
    cols = (qs.actor, qs.a0, qs.a1, None, None)
    cols_q = cols + (qs.a0,)
    ts = alternate_events([("topics", lambda: sc_t._fill(cols, Q, total)), ("queues", lambda: sc_q._fill(cols_q, Q, total)),
                           ("topics again", lambda: sc_t._fill(cols, Q, total))], iters, reps)
    tc = alternate_events([("topics", lambda: sc_t._count(cols, Q)), ("queues", lambda: sc_q._count(cols_q, Q))], iters, reps)
    med = {k: statistics.median(v) for k, v in ts.items()}
    lines.append(f"| {Q} | {total} | {stat(ts['topics'])} | {stat(ts['topics again'])} | {med['topics again'] - med['topics']:+.1f} | "
                 f"{stat(ts['queues'])} | {med['queues'] - med['topics']:+.1f} | {stat(tc['topics'])} | {stat(tc['queues'])} |")
    print(lines[-1], flush=True)
    return lines + [""]


def queue_case(pubs: int, unit: bool, dev):
    """``pubs`` publications over 64 topics of 8 queue subscriptions of 1024 members each (one
    strided segment, or 1024 segments of length 1).  Returns (topics Scatter, members Scatter of
    the identical rows, publications, key column)."""
    topics_n = 64
    gen = torch.Generator().manual_seed(12)
    n_subs = topics_n * SUBS_PER_TOPIC
    start = torch.randint(0, 1 << 20, (n_subs,), generator=gen).numpy()
    stride = torch.randint(1, 1 << 10, (n_subs,), generator=gen).numpy()
    if unit:
        seg_start = (start[:, None] + stride[:, None] * np.arange(MEMBERS)[None, :]).reshape(-1)
        flat = {"row_off": np.arange(n_subs * MEMBERS + 1, dtype=np.int64), "seg_start": seg_start,
                "seg_stride": np.ones(n_subs * MEMBERS, dtype=np.int32), "q_seg": np.arange(n_subs + 1, dtype=np.int64) * MEMBERS}
    else:
        flat = {"row_off": np.arange(n_subs + 1, dtype=np.int64) * MEMBERS, "seg_start": start, "seg_stride": stride,
                "q_seg": np.arange(n_subs + 1, dtype=np.int64)}
    flat["seg_off"] = np.zeros(topics_n + 1, dtype=np.int64)
    flat["q_off"] = np.arange(topics_n + 1, dtype=np.int64) * SUBS_PER_TOPIC
    host = T.TopicTable("cpu", max_topics=topics_n)
    host.load(flat)
    table = T.TopicTable(dev, max_topics=topics_n)
    table.load(flat)
    g = torch.randint(0, topics_n, (pubs,), generator=gen).to(torch.int32)
    key = torch.randint(-2**62, 2**62, (pubs,), generator=gen)
    qs = MsgBatch(g, torch.randint(-2**31, 2**31, (pubs,), generator=gen), torch.randint(-2**31, 2**31, (pubs,), generator=gen),
                  None, METHOD_CALC_MULTIPLY)
    ref = S.scatter_ref(S.Scatter.topics(host, capacity=pubs * SUBS_PER_TOPIC), qs, key=key)  # the rows, on the host
    rows = pubs * SUBS_PER_TOPIC
    assert ref["total"] == rows
    sc_t = S.Scatter.topics(table, capacity=rows, q_capacity=pubs)
    offsets = (torch.arange(pubs + 1, dtype=torch.int64) * SUBS_PER_TOPIC).to(dev)
    sc_m = S.Scatter.members(offsets, ref["actor"].to(dev), capacity=rows, q_capacity=pubs)
    c = (lambda t: t.to(dev))
    qs_t = MsgBatch(c(qs.actor), c(qs.a0), c(qs.a1), None, METHOD_CALC_MULTIPLY)
    qs_m = MsgBatch(torch.arange(pubs, dtype=torch.int32, device=dev), qs_t.a0, qs_t.a1, None, METHOD_CALC_MULTIPLY)
    return sc_t, sc_m, qs_t, qs_m, c(key)


def queue_rows(pubs: int, iters: int, reps: int, dev) -> list[str]:
    lines = ["### (b), (c) queue rows against the `members` rule producing the identical rows", "",
             "| table | Q | rows | queue subscriptions | segments | queue expand launch us | members expand launch us | members again us | "
             "baseline spread (median - median) us | queue / members | queue count+scan+first us | members count+scan+first us |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, unit in (("8 queue subscriptions per topic, 1024 members in one segment", False),
                        ("the same, 1024 segments of length 1 per subscription", True)):
        sc_t, sc_m, qs_t, qs_m, key = queue_case(pubs, unit, dev)
        et, em = sc_t.expand(qs_t, key=key), sc_m.expand(qs_m)
        equal_or_die(et, em, label)
        Q, total = et.Q, et.total
        cols_t = (qs_t.actor, qs_t.a0, qs_t.a1, None, None, key)
        cols_m = (qs_m.actor, qs_m.a0, qs_m.a1, None, None)
        ts = alternate_events([("members", lambda: sc_m._fill(cols_m, Q, total)), ("queues", lambda: sc_t._fill(cols_t, Q, total)),
                               ("members again", lambda: sc_m._fill(cols_m, Q, total))], iters, reps)
        tc = alternate_events([("members", lambda: sc_m._count(cols_m, Q)), ("queues", lambda: sc_t._count(cols_t, Q))], iters, reps)
        med = {k: statistics.median(v) for k, v in ts.items()}
        lines.append(f"| {label} | {Q} | {total} | {sc_t.table.n_queues} | {sc_t.table.host['seg_start'].size} | {stat(ts['queues'])} | "
                     f"{stat(ts['members'])} | {stat(ts['members again'])} | {med['members again'] - med['members']:+.1f} | "
                     f"{med['queues'] / med['members']:.2f} | {stat(tc['queues'])} | {stat(tc['members'])} |")
        print(lines[-1], flush=True)
        del sc_t, sc_m, et, em
        torch.cuda.empty_cache()
    return lines + [""]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--pubs", type=int, default=8192)
    ap.add_argument("--qpubs", type=int, default=1 << 18)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("queue_cost: no GPU", file=sys.stderr)
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
          "after 2 warm-up groups, the variants alternating in one process, the baseline twice in the rotation.  The "
          "columns compared for exact equality first.  Cells: median (min .. max).", ""])
    emit(without_queues(a.rows, a.pubs, a.iters, a.reps, dev))
    emit(queue_rows(a.qpubs, a.iters, a.reps, dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
