"""Pub/sub topics: subscriptions kept in the replicated store, expanded on the device.

A subscription is one record of the store (cluster-wide truth, so every client of a
cluster agrees on who is subscribed to what):

``store/_ptype/topics/<service>/<topic>/<name>`` -> ``{"segments": [[start, count, stride], ...], "queue": true}``

``topic`` is a decimal integer in ``[0, max_topics)`` (``gpu.topics``, default 1024), ``name``
the subscription's name (by default the node's).  Logical actor ids are arithmetic here
(actor ``rank + world * k``), so a subscription is a list of **strided segments**: segment
``[start, count, stride]`` stands for the ids ``start + stride * k``, ``0 <= k < count``, valid
when ``count >= 1``, ``stride >= 1``, ``start >= 0`` and its last id is at most ``2**31 - 2``.  A
record holds 1 to 1024 segments.  A topic's subscribers are its records in key order,
segments in record order, and **nothing is de-duplicated across records**: two
subscriptions that both name actor 5 deliver to it twice.  A record is persistent unless it
was put under a lease (``Client.Subscribe(ephemeral=True)``): actors are re-homed when a
rank fails, so by default a subscription outlives the node that made it.

``queue`` is optional.  Absent or ``false`` is an *ordinary* subscription: every one of its ids
gets every publication (Akka's ``DistributedPubSub.Publish``).  ``true`` makes the record a
**queue subscription** (competing consumers: Akka's ``sendOneMessageToEachGroup``, a NATS queue
group, a Kafka consumer group): a publication reaches exactly ONE of its members, the ids of
its segments in record order, ``1 <= c <= 2**31 - 1`` of them.  Which one is ``ops/scatter.py``'s
business (by a key's hash, so one key always reaches one member while the membership stands,
or round robin by index).  Any other value of ``queue`` makes the record invalid.  A
publication's rows are those of the topic's ordinary subscriptions, then one row per queue
subscription of the topic, in key order.

``TopicTable`` is the device side: the four arrays the scatter's ``topics`` rule reads
(``ops/scatter.py``) -- ``seg_off`` int64[max_topics + 1], ``row_off`` int64[S + 1],
``seg_start`` / ``seg_stride`` int32[S]; no per-subscriber list exists on the host or in HBM.
The segments of the queue subscriptions follow the ordinary ones in ``row_off`` / ``seg_start``
/ ``seg_stride`` (``seg_off[max_topics]`` keeps bounding the ordinary ones); ``q_off``
int64[max_topics + 1] maps a topic to its queue subscriptions and ``q_seg`` int64[NQ + 1] a
queue subscription to its first segment (1 to 1024 segments each).  Ordinary plus queue
segments, and the queue subscriptions, number at most ``2**24`` each.
The compiled follower (``_core.TopicFollower``, csrc/core/topic_follower.hpp) keeps the
records current with a watch and a periodic re-list and flattens them; a record that is
not valid is skipped and counted (``bad_records``), never an error.  ``apply()`` -- at the
start of every Publish, on the caller's stream -- uploads the arrays when the follower's
version moved and is two atomic loads otherwise.  ``wait(rev)`` blocks until the applied
table reflects store revision ``rev``: read-your-writes for ``Subscribe``.
"""
from __future__ import annotations

import time

import numpy as np
import torch

TOPICS_PREFIX = "_ptype/topics"
STORE_PREFIX = "store/"
LEASE_TTL_S = 2                  # an ephemeral subscription's lease (the service registry's)
MAX_TOPICS = 1 << 20             # topic_follower.hpp kTopicMaxTopics
MAX_RECORD_SEGMENTS = 1024       # topic_follower.hpp kTopicMaxSegmentsPerRecord
MAX_ACTOR = (1 << 31) - 2        # topic_follower.hpp kTopicMaxActor
MAX_SEGMENTS = 1 << 24           # topic_follower.hpp kTopicMaxSegments (ordinary plus queue)
MAX_QUEUES = 1 << 24             # topic_follower.hpp kTopicMaxQueues
MAX_QUEUE_MEMBERS = (1 << 31) - 1  # topic_follower.hpp kTopicMaxQueueMembers


def topic_key(service: str, topic: int, name: str) -> str:
    """The store key of a subscription (with the store's own prefix)."""
    return f"{STORE_PREFIX}{TOPICS_PREFIX}/{service}/{int(topic)}/{name}"


def check_segments(segments) -> list[list[int]]:
    """``segments`` as a validated list of ``[start, count, stride]``; raises ``ValueError``."""
    out = []
    for seg in segments:
        if len(seg) != 3:
            raise ValueError("a segment is [start, count, stride]")
        start, count, stride = (int(x) for x in seg)
        if start < 0 or count < 1 or stride < 1 or start + stride * (count - 1) > MAX_ACTOR:
            raise ValueError(f"segment {[start, count, stride]}: need start >= 0, count >= 1, stride >= 1 and a last "
                             f"id of at most {MAX_ACTOR}")
        out.append([start, count, stride])
    if not 1 <= len(out) <= MAX_RECORD_SEGMENTS:
        raise ValueError(f"a subscription holds 1 to {MAX_RECORD_SEGMENTS} segments, not {len(out)}")
    return out


def segments_of(ids) -> list[list[int]]:
    """The ids (any iterable or tensor of ints) as strided segments: sorted, de-duplicated,
    then cut greedily from the left -- a run opens at ``ids[i]`` with the stride ``ids[i + 1]
    - ids[i]`` (1 for a last lone id) and extends while the difference repeats.
    Deterministic; an arithmetic progression becomes one segment."""
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().numpy()
    u = np.unique(np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids, dtype=np.int64))
    out, i, n = [], 0, int(u.size)
    if n == 0:
        return out
    d = np.diff(u)
    # change: the indices j >= 1 with d[j] != d[j - 1], where a run of equal differences ends
    change = np.flatnonzero(d[1:] != d[:-1]) + 1 if n > 2 else np.zeros(0, dtype=np.int64)
    while i < n:
        if i == n - 1:
            out.append([int(u[i]), 1, 1])
            break
        at = int(np.searchsorted(change, i, side="right"))
        e = int(change[at]) if at < change.size else n - 1  # d[i .. e - 1] are equal
        out.append([int(u[i]), e - i + 1, int(d[i])])
        i = e + 1
    return out


def flatten_segments(segments) -> np.ndarray:
    """The ids a list of segments stands for, in order (int64; for tests and ``Topics()``)."""
    parts = [s + st * np.arange(c, dtype=np.int64) for s, c, st in segments]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def flatten_records(records: dict, max_topics: int) -> dict:
    """``{"<topic>/<name>": value}`` through the compiled flatten (``_core.topics_flatten``)."""
    from .._core import topics_flatten

    return topics_flatten({str(k): str(v) for k, v in records.items()}, int(max_topics))


class TopicTable:
    """The topic table of one service (module docstring).  ``kv``: the cluster's KvClient; None
    builds a table without a follower, filled with ``load`` (tests, tools)."""

    def __init__(self, device, max_topics: int = 1024, kv=None, service: str = "", relist_s: float = 0.5,
                 watch: bool = True):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_topics = int(max_topics)
        if not 1 <= self.max_topics <= MAX_TOPICS:
            raise ValueError(f"TopicTable: max_topics must be in [1, {MAX_TOPICS}]")
        self.service = service
        self.prefix = f"{STORE_PREFIX}{TOPICS_PREFIX}/{service}/"
        self.relist_s = float(relist_s)
        self.applied_rev = 0
        self.uploads = 0
        self.counters = {"records": 0, "bad_records": 0, "events": 0, "relists": 0}
        self.subs: list = []
        self.queues: list = []
        self._dev = self._args = None
        self.load({"seg_off": np.zeros(self.max_topics + 1, dtype=np.int64), "row_off": np.zeros(1, dtype=np.int64),
                   "seg_start": np.zeros(0, dtype=np.int32), "seg_stride": np.zeros(0, dtype=np.int32)})
        self._f = None
        if kv is not None:
            from .._core import TopicFollower

            self._f = TopicFollower(kv, self.prefix, self.max_topics, self.relist_s, bool(watch))
            self.apply()

    @classmethod
    def from_topics(cls, device, topics: dict, max_topics: int = 1024, queues: dict | None = None) -> "TopicTable":
        """A table without a follower from ``{topic: [[start, count, stride], ...]}`` (any number
        of segments per topic: no records are involved; ``load`` validates) and, with
        ``queues={topic: [[[start, count, stride], ...], ...]}``, the topics' queue subscriptions
        (a list of segment lists per topic, 1 to 1024 segments each)."""
        t = cls(device, max_topics)
        queues = queues or {}
        for g in queues:
            if not 0 <= int(g) < t.max_topics:
                raise ValueError(f"TopicTable.from_topics: topic {g} outside [0, {t.max_topics})")
        per = np.zeros(t.max_topics + 1, dtype=np.int64)
        rows = []
        for g in sorted(topics):
            if not 0 <= int(g) < t.max_topics:
                raise ValueError(f"TopicTable.from_topics: topic {g} outside [0, {t.max_topics})")
            segs = np.asarray(topics[g], dtype=np.int64).reshape(-1, 3)
            per[int(g) + 1] = segs.shape[0]
            rows.append(segs)
        S = int(sum(r.shape[0] for r in rows))
        q_per = np.zeros(t.max_topics + 1, dtype=np.int64)
        q_seg, qlist = [S], []
        for g in sorted(queues, key=int):
            q_per[int(g) + 1] = len(queues[g])
            for sub in queues[g]:
                segs = np.asarray(sub, dtype=np.int64).reshape(-1, 3)
                qlist.append((int(g), "", q_seg[-1], int(segs.shape[0])))
                q_seg.append(q_seg[-1] + int(segs.shape[0]))
                rows.append(segs)
        segs = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int64)
        if segs.size and (segs[:, 0].max() > MAX_ACTOR or segs[:, 2].max() > MAX_ACTOR):
            raise ValueError("TopicTable.from_topics: a segment leaves [0, 2**31 - 2]")
        t.load({"seg_off": np.cumsum(per), "row_off": np.concatenate([[0], np.cumsum(segs[:, 1])]),
                "seg_start": segs[:, 0], "seg_stride": segs[:, 2],
                "subs": [(int(g), "", int(np.cumsum(per)[int(g)]), int(per[int(g) + 1])) for g in sorted(topics)],
                "q_off": np.cumsum(q_per), "q_seg": np.asarray(q_seg, dtype=np.int64), "queues": qlist})
        return t

    # ------------------------------------------------------------------ the arrays
    def load(self, flat: dict) -> None:
        """Replace the table with flattened arrays (validated: a table the kernels may trust).
        Without ``q_off`` / ``q_seg`` the table has no queue subscriptions."""
        a = {k: np.ascontiguousarray(flat[k], dtype=dt) for k, dt in
             (("seg_off", np.int64), ("row_off", np.int64), ("seg_start", np.int32), ("seg_stride", np.int32))}
        if ("q_off" in flat) != ("q_seg" in flat):
            raise ValueError("TopicTable.load: q_off and q_seg come together")
        S = int(a["seg_start"].size)  # ordinary plus queue segments
        if a["seg_off"].size != self.max_topics + 1 or a["row_off"].size != S + 1 or a["seg_stride"].size != S or \
                S > MAX_SEGMENTS:
            raise ValueError("TopicTable.load: the arrays' lengths do not fit a table of max_topics topics")
        if "q_off" in flat:
            a["q_off"] = np.ascontiguousarray(flat["q_off"], dtype=np.int64)
            a["q_seg"] = np.ascontiguousarray(flat["q_seg"], dtype=np.int64)
        else:
            a["q_off"] = np.zeros(self.max_topics + 1, dtype=np.int64)
            a["q_seg"] = np.full(1, S, dtype=np.int64)
        NQ = int(a["q_seg"].size) - 1
        if a["q_off"].ndim != 1 or a["q_seg"].ndim != 1 or a["q_off"].size != self.max_topics + 1 or \
                not 0 <= NQ <= MAX_QUEUES:
            raise ValueError("TopicTable.load: the queue arrays' lengths do not fit a table of max_topics topics")
        So = int(a["q_seg"][0])  # the ordinary segments
        if int(a["seg_off"][0]) != 0 or int(a["seg_off"][-1]) != So or bool((np.diff(a["seg_off"]) < 0).any()) or \
                int(a["row_off"][0]) != 0 or bool((np.diff(a["row_off"]) < 1).any()):
            raise ValueError("TopicTable.load: seg_off must run from 0 to S and row_off increase strictly from 0")
        if int(a["q_off"][0]) != 0 or int(a["q_off"][-1]) != NQ or bool((np.diff(a["q_off"]) < 0).any()) or \
                int(a["q_seg"][-1]) != S or bool((np.diff(a["q_seg"]) < 1).any()) or \
                bool((np.diff(a["q_seg"]) > MAX_RECORD_SEGMENTS).any()):
            raise ValueError("TopicTable.load: q_off must run from 0 to the queue subscriptions, q_seg from the "
                             "ordinary segments to all of them in steps of 1 to 1024")
        if NQ and int(np.diff(a["row_off"][a["q_seg"]]).max()) > MAX_QUEUE_MEMBERS:
            raise ValueError(f"TopicTable.load: a queue subscription has more than {MAX_QUEUE_MEMBERS} members")
        if S:
            last = a["seg_start"].astype(np.int64) + a["seg_stride"].astype(np.int64) * (np.diff(a["row_off"]) - 1)
            if int(a["seg_start"].min()) < 0 or int(a["seg_stride"].min()) < 1 or int(last.max()) > MAX_ACTOR:
                raise ValueError("TopicTable.load: a segment leaves [0, 2**31 - 2]")
        self.host = a
        self.subs = list(flat.get("subs", []))
        self.queues = list(flat.get("queues", []))
        self._dev = None
        self.uploads += 1

    @property
    def n_queues(self) -> int:
        """The queue subscriptions of the table."""
        return int(self.host["q_seg"].size) - 1

    def device_arrays(self, device=None, queues: bool = False):
        """``(seg_off, row_off, seg_start, seg_stride)`` on the table's device -- with
        ``queues=True`` followed by ``(q_off, q_seg)``: new tensors per upload, so kernels
        already enqueued keep reading the arrays they were given."""
        device = self.device if device is None else torch.device(device)
        if device != self.device:
            raise ValueError("TopicTable: the questions live on another device than the table")
        if self._dev is None:
            self._args = None
            names = ("seg_off", "row_off", "seg_start", "seg_stride", "q_off", "q_seg")
            if device.type == "cuda":
                up = (lambda a: (a.pin_memory() if a.numel() else a).to(device, non_blocking=True))
                self._dev = tuple(up(torch.from_numpy(self.host[k])) for k in names)
            else:
                self._dev = tuple(torch.from_numpy(self.host[k]) for k in names)
        return self._dev if queues else self._dev[:4]

    def launch_args(self, device):
        """What the scatter launchers take of the table: ``(seg_off, topics, row_off, ordinary
        segments, seg_start, seg_stride, q_off, q_seg, queue subscriptions, all segments)`` as
        pointers and counts, kept until the next upload."""
        if self._dev is None or self._args is None or device != self.device:
            d = self.device_arrays(device, queues=True)
            self._args = (d[0].data_ptr(), int(d[0].numel()) - 1, d[1].data_ptr(), int(self.host["q_seg"][0]),
                          d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                          int(d[5].numel()) - 1, int(d[2].numel()))
        return self._args

    # ------------------------------------------------------------------ following the store
    def apply(self) -> bool:
        """Take the follower's table when its version moved (True); two loads otherwise."""
        f = self._f
        if f is None or f.quiet():
            return False
        flat = f.take()
        self.load(flat)
        self.applied_rev = max(self.applied_rev, int(flat["rev"]))
        self.counters = {k: int(flat[k]) for k in ("records", "bad_records", "events", "relists")}
        return True

    def wait(self, rev: int, timeout: float = 10.0) -> None:
        """Block until the applied table reflects store revision ``rev``."""
        if self._f is None:
            raise RuntimeError("TopicTable.wait: the table follows no store")
        deadline = time.monotonic() + float(timeout)
        while True:
            seen = int(self._f.rev)  # (read before quiet(): topic_follower.hpp)
            self.apply()
            if self._f.quiet():
                self.applied_rev = max(self.applied_rev, seen)
            if self.applied_rev >= int(rev):
                return
            left = deadline - time.monotonic()
            if left <= 0:
                raise TimeoutError(f"topics of {self.service!r}: applied revision {self.applied_rev}, waiting for {rev}")
            self._f.wait_change(int(min(left, 0.05) * 1000) + 1)

    # ------------------------------------------------------------------ views
    def view(self, queues: bool = False) -> dict:
        """The applied ordinary subscriptions: ``{topic: [(name, [[start, count, stride], ...])]}``.
        ``queues=True``: every subscription as ``(name, segments, queue)``, a topic's ordinary ones
        (``queue`` False) before its queue subscriptions (True), each in key order."""
        h, out = self.host, {}
        cnt = np.diff(h["row_off"])
        for is_q, subs in ((False, self.subs), (True, self.queues if queues else [])):
            for topic, name, seg, n in subs:
                segs = [[int(h["seg_start"][s]), int(cnt[s]), int(h["seg_stride"][s])] for s in range(seg, seg + n)]
                out.setdefault(int(topic), []).append((name, segs, is_q) if queues else (name, segs))
        return dict(sorted(out.items())) if queues else out

    def stats(self) -> dict:
        h = self.host
        c = self.counters
        So = int(h["q_seg"][0])  # (the ordinary subscriptions' segments; queue_stats has the others)
        return {"topics": int((np.diff(h["seg_off"]) > 0).sum()), "segments": So,
                "subscribers": int(h["row_off"][So]), "records": c["records"], "bad_records": c["bad_records"],
                "applied_rev": int(self.applied_rev)}

    def queue_stats(self) -> dict:
        """The queue subscriptions of the applied table, their members and their segments."""
        h = self.host
        So = int(h["q_seg"][0])
        return {"queues": self.n_queues, "members": int(h["row_off"][-1] - h["row_off"][So]),
                "segments": int(h["seg_start"].size) - So}

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
