"""Topic queue subscriptions without a GPU: ``scatter_ref`` against a sequential loop over
records that shares no code with it (member lists, Python ints), the pinned pick values, the
compiled flatten on queue records, the ``seq`` counter of ``by="index"``, and Subscribe(queue=True)
/ Publish(key=, by=) through a real one-member ``Join`` on the CPU runtime."""
import json
import time

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import scatter as S
from ptype_amd.ops import topics as T
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_CALC_MULTIPLY, STATUS_OK
from ptype_amd.ops.table import mix64

from test_scatter import same_expansion
from test_topics import cpu_join

M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_ACTOR = (1 << 31) - 2


def rec(*segments, queue=None):
    d = {"segments": [list(s) for s in segments]}
    if queue is not None:
        d["queue"] = queue
    return json.dumps(d)


# ---------------------------------------------------------------- the second oracle: Python ints only
def py_mix64(x: int) -> int:
    x &= M64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return x


def py_pick(c: int, key: int | None = None, index: int | None = None) -> int:
    if index is not None:
        return (index & M64) % c
    return ((py_mix64(key) >> 32) * c) >> 32


def loop_oracle(records, max_topics, qs, by="key", key=None, seq=0):
    """Publication by publication: the ordinary records' ids, then one member of every queue
    record, both in key order.  Rows are (actor, a0, a1, method, q)."""
    rows, first, n, oob = [], [], [], 0
    for q in range(qs.M):
        first.append(len(rows))
        g = int(qs.actor[q])
        m = qs.method if isinstance(qs.method, int) else int(qs.method[q])
        if not 0 <= g < max_topics:
            oob += 1
            n.append(0)
            continue
        before = len(rows)
        payload = (int(qs.a0[q]), None if qs.a1 is None else int(qs.a1[q]), m, q)
        for want_queue in (False, True):
            for k in sorted(records):
                topic, _name = k.split("/", 1)
                r = json.loads(records[k])
                if int(topic) != g or bool(r.get("queue", False)) != want_queue:
                    continue
                members = [start + stride * j for start, count, stride in r["segments"] for j in range(count)]
                if want_queue:
                    kq = int(qs.a0[q]) if key is None else int(key[q])
                    at = py_pick(len(members), key=kq) if by == "key" else py_pick(len(members), index=seq + q)
                    members = [members[at]]
                rows += [(a,) + payload for a in members]
        n.append(len(rows) - before)
    return rows, first, n, oob


RECORDS = {
    "3/b": rec([0, 4, 2], [100, 1, 1]), "3/a": rec([7, 3, 5]), "3/q1": rec([50, 5, 3], [9, 2, 1], queue=True),
    "3/a0": rec([1000, 7, 1], queue=True), "3/plain": rec([8, 1, 1], queue=False),
    "0/x": rec([MAX_ACTOR - 6, 3, 3]), "0/y": rec([MAX_ACTOR - 12, 5, 3], queue=True),
    "10/n1": rec([5, 2, 1]), "10/n0": rec([5, 1, 1], [5, 1, 1]),
    "2/solo": rec([9, 1, 1], queue=True),                                        # a topic with only a queue subscription, one member
    "7/w0": rec(*[[3 * k, 1, 1] for k in range(40)], queue=True), "7/w1": rec([500, 40, 2], queue=True),  # only queues
    "6/z": rec([77, 3, 1]),
}
QUEUE_KEYS = [k for k in RECORDS if json.loads(RECORDS[k]).get("queue")]


def the_table(records=RECORDS, max_topics=11):
    flat = T.flatten_records(records, max_topics)
    table = T.TopicTable("cpu", max_topics=max_topics)
    table.load(flat)
    return flat, table


def the_questions(method_col=False):
    g = [3, 10, 0, 1, 11, -1, 3, 2, 1 << 20, 7, 7, -(1 << 31), (1 << 31) - 1, 7, 6, 2, 0, 3]
    Q = len(g)
    method = ([METHOD_CALC_MULTIPLY, METHOD_ECHO] * Q)[:Q] if method_col else METHOD_ECHO
    a0 = torch.arange(Q, dtype=torch.int64) * 3 - 7
    a0[2], a0[9] = I64_MIN, I64_MAX
    return MsgBatch(torch.tensor(g, dtype=torch.int32), a0, torch.arange(Q, dtype=torch.int64) + (1 << 40), None,
                    torch.tensor(method, dtype=torch.int16) if method_col else method)


def same_rows(ref, rows, first, n, oob, qs):
    assert ref["total"] == len(rows) and ref["oob"] == oob
    assert ref["first"].tolist() == first and ref["n"].tolist() == n
    assert ref["actor"].tolist() == [r[0] for r in rows]
    assert ref["a0"].tolist() == [r[1] for r in rows] and ref["a1"].tolist() == [r[2] for r in rows] and ref["a2"] is None
    assert ref["group"].tolist() == [r[4] for r in rows]
    if not isinstance(qs.method, int):
        assert ref["method"].tolist() == [r[3] for r in rows]


@pytest.mark.parametrize("by", ["key", "index"])
@pytest.mark.parametrize("method_col", [False, True])
def test_queue_reference_against_the_loop(by, method_col):
    qs = the_questions(method_col)
    flat, table = the_table()
    assert flat["bad_records"] == 0 and flat["records"] == len(RECORDS)
    for key in (None, torch.arange(qs.M, dtype=torch.int64) * 0x9e3779b97f4a7c15 % (1 << 62) - (1 << 61)):
        sc = S.Scatter.topics(table, capacity=256, by=by)
        sc.seq = 12345
        ref = S.scatter_ref(sc, qs, key=key)
        rows, first, n, oob = loop_oracle(RECORDS, 11, qs, by=by, key=key, seq=12345)
        same_rows(ref, rows, first, n, oob, qs)
        assert oob == 5 and sc.seq == 12345  # (the reference leaves the counter alone)
        exp = sc.expand(qs, key=key)         # the CPU expand is the reference
        same_expansion(exp, ref)
        assert sc.seq == (12345 + qs.M if by == "index" else 12345)
    # topic 3: 4 + 1 + 3 + 1 ordinary rows (a, b, plain), then a0 and q1; topic 7: two queue rows only
    assert n[0] == 9 + 2 and n[9] == 2 and n[7] == 1 and n[3] == 0 and n[14] == 3 and n[2] == 3 + 1
    assert [r[0] for r in rows[first[0]:first[0] + 9]] == [7, 12, 17, 0, 2, 4, 6, 100, 8]
    assert 1000 <= rows[first[0] + 9][0] < 1007 and rows[first[0] + 10][0] in (50, 53, 56, 59, 62, 9, 10)
    assert rows[first[7]][0] == 9  # one member


def test_the_key_column_differs_from_a0_and_is_what_picks():
    qs = the_questions()
    _, table = the_table()
    sc = S.Scatter.topics(table, capacity=256)
    key = torch.full((qs.M,), 99, dtype=torch.int64)
    a, b = S.scatter_ref(sc, qs), S.scatter_ref(sc, qs, key=key)
    assert not torch.equal(a["actor"], b["actor"]) and torch.equal(a["a0"], b["a0"]) and torch.equal(a["group"], b["group"])
    # one key, one member: every publication to topic 7 reaches the same two actors
    at = [int(b["first"][q]) for q in (9, 10, 13)]
    assert len({(int(b["actor"][i]), int(b["actor"][i + 1])) for i in at}) == 1
    assert torch.equal(S.scatter_ref(sc, qs, key=qs.a0)["actor"], a["actor"])  # the default key is a0


# ---------------------------------------------------------------- the pinned pick values
def test_pinned_pick_values():
    assert int(mix64(np.array([0], dtype=np.uint64))[0]) == 0 == py_mix64(0)
    assert int(mix64(np.array([1], dtype=np.uint64))[0]) == 0x5692161d100b05e5 == py_mix64(1)
    keys = np.array([0, 1, -1, I64_MAX, I64_MIN], dtype=np.int64)
    assert S.queue_pick(7, key=keys).tolist() == [0, 2, 4, 2, 1] == [py_pick(7, key=int(k)) for k in keys]
    assert int(S.queue_pick((1 << 31) - 1, key=np.array([-1], dtype=np.int64))[0]) == 1516776189 == py_pick((1 << 31) - 1, key=-1)
    assert S.queue_pick(1, key=keys).tolist() == [0] * 5
    assert S.queue_pick(1, index=np.array([0, 5, M64], dtype=np.uint64)).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        S.queue_pick(3)
    edge = np.array([0, -1, I64_MIN, I64_MAX, 1, 2, 12345, -98765], dtype=np.int64)
    for c in (1, 2, 3, 1024, (1 << 31) - 1):
        m = S.queue_pick(c, key=edge)
        assert m.dtype == np.uint64 and int(m.max()) < c
        assert m.tolist() == [py_pick(c, key=int(k)) for k in edge]
        ix = np.array([0, 1, c - 1, c, M64 - 2, M64], dtype=np.uint64)
        assert S.queue_pick(c, index=ix).tolist() == [int(i) % c for i in ix]
    counts = np.bincount(S.queue_pick(8, key=np.arange(4096, dtype=np.int64)).astype(np.int64), minlength=8)
    assert counts.sum() == 4096 and 477 <= counts.min() and counts.max() <= 565  # no member unpicked


def test_the_pick_reaches_both_ends_of_the_largest_subscription():
    c = (1 << 31) - 1
    table = T.TopicTable.from_topics("cpu", {}, max_topics=2, queues={1: [[[0, c, 1]]]})
    keys = np.arange(200000, dtype=np.int64)
    m = S.queue_pick(c, key=keys).astype(np.int64)
    lo, hi = int(keys[m.argmin()]), int(keys[m.argmax()])
    assert m.min() < 1 << 16 and m.max() > c - (1 << 16)
    qs = MsgBatch(torch.ones(3, dtype=torch.int32), torch.tensor([lo, hi, -1]), None, None, METHOD_ECHO)
    ref = S.scatter_ref(S.Scatter.topics(table, capacity=8), qs)
    assert ref["actor"].tolist() == [py_pick(c, key=lo), py_pick(c, key=hi), 1516776189] and ref["n"].tolist() == [1, 1, 1]


# ---------------------------------------------------------------- the compiled flatten
def test_flatten_keeps_the_ordinary_arrays_and_lists_queues_in_key_order():
    flat = T.flatten_records(RECORDS, 11)
    plain = T.flatten_records({k: v for k, v in RECORDS.items() if k not in QUEUE_KEYS}, 11)
    S_ord = int(plain["seg_start"].size)
    assert flat["seg_off"].tolist() == plain["seg_off"].tolist() and flat["subs"] == plain["subs"]
    assert all(len(s) == 4 for s in flat["subs"])
    assert flat["row_off"][:S_ord + 1].tolist() == plain["row_off"].tolist()
    assert flat["seg_start"][:S_ord].tolist() == plain["seg_start"].tolist()
    assert flat["seg_stride"][:S_ord].tolist() == plain["seg_stride"].tolist()
    assert (flat["topics"], flat["segments"], flat["subscribers"]) == (plain["topics"], plain["segments"], plain["subscribers"])
    assert plain["q_off"].tolist() == [0] * 12 and plain["q_seg"].tolist() == [S_ord] and plain["queues"] == []
    # the queue subscriptions: by topic, then key order, their segments after the ordinary ones
    assert [(q[0], q[1]) for q in flat["queues"]] == [(0, "y"), (2, "solo"), (3, "a0"), (3, "q1"), (7, "w0"), (7, "w1")]
    assert [q[3] for q in flat["queues"]] == [1, 1, 1, 2, 40, 1]
    assert flat["q_seg"].tolist() == [S_ord, S_ord + 1, S_ord + 2, S_ord + 3, S_ord + 5, S_ord + 45, S_ord + 46]
    assert [q[2] for q in flat["queues"]] == flat["q_seg"].tolist()[:-1]
    assert flat["q_off"].tolist() == [0, 1, 1, 2, 4, 4, 4, 4, 6, 6, 6, 6]
    assert flat["queue_segments"] == 46 and flat["queue_members"] == 5 + 1 + 7 + 7 + 40 + 40
    assert flat["row_off"].size == S_ord + 46 + 1 and bool((np.diff(flat["row_off"]) >= 1).all())
    _, table = the_table()
    assert table.view() == T.TopicTable("cpu", max_topics=11).view() | the_table(
        {k: v for k, v in RECORDS.items() if k not in QUEUE_KEYS})[1].view()
    v = table.view(queues=True)
    assert list(v) == [0, 2, 3, 6, 7, 10]
    assert v[3] == [("a", [[7, 3, 5]], False), ("b", [[0, 4, 2], [100, 1, 1]], False), ("plain", [[8, 1, 1]], False),
                    ("a0", [[1000, 7, 1]], True), ("q1", [[50, 5, 3], [9, 2, 1]], True)]
    assert v[2] == [("solo", [[9, 1, 1]], True)] and v[6] == [("z", [[77, 3, 1]], False)]
    assert table.queue_stats() == {"queues": 6, "members": 100, "segments": 46}
    assert table.stats()["segments"] == S_ord and table.stats()["subscribers"] == plain["subscribers"]


HOSTILE_QUEUE = {"a number": "1", "zero": "0", "a string": '"true"', "null": "null", "a list": "[true]", "an object": "{}",
                 "a float": "1.0", "an empty string": '""'}


@pytest.mark.parametrize("what", sorted(HOSTILE_QUEUE))
def test_flatten_skips_and_counts_a_hostile_queue_value(what):
    good = {"3/z": rec([10, 2, 5]), "4/0": rec([1, 1, 1], queue=True), "4/z": rec([7, 3, 1]), "5/a": rec([0, 2, 2])}
    bad = '{"segments": [[1, 2, 3]], "queue": ' + HOSTILE_QUEUE[what] + "}"
    want = T.flatten_records(good, 8)
    for key in ("4/a", "4/00"):
        flat = T.flatten_records(dict(good, **{key: bad}), 8)
        assert flat["records"] == 5 and flat["bad_records"] == 1 and want["bad_records"] == 0
        for k in ("seg_off", "row_off", "seg_start", "seg_stride", "q_off", "q_seg"):
            assert flat[k].dtype == want[k].dtype and flat[k].tolist() == want[k].tolist(), k
        assert flat["subs"] == want["subs"] and flat["queues"] == want["queues"] == [(4, "0", 3, 1)]


def test_flatten_limits_of_a_queue_record():
    big = (1 << 31) - 1
    ok = {"1/a": rec([0, big, 1], queue=True), "1/b": rec([0, big - 1, 1], [5, 1, 1], queue=True),
          "1/c": rec(*[[k, 1, 1] for k in range(1024)], queue=True), "1/d": rec([0, big, 1], [0, big, 1])}
    flat = T.flatten_records(ok, 2)
    assert flat["bad_records"] == 0 and len(flat["queues"]) == 3 and flat["queue_members"] == 2 * big + 1024
    bad = {"1/e": rec([0, big, 1], [0, 1, 1], queue=True),          # 2^31 members
           "1/f": rec(*[[k, 1, 1] for k in range(1025)], queue=True),
           "1/g": rec([0, 0, 1], queue=True), "1/h": '{"queue": true}', "1/i": '{"segments": [], "queue": true}'}
    flat = T.flatten_records(dict(ok, **bad), 2)
    assert flat["bad_records"] == 5 and len(flat["queues"]) == 3 and len(flat["subs"]) == 1
    lim = __import__("ptype_amd")._core.topic_limits()
    assert (lim["max_queues"], lim["max_queue_members"]) == (T.MAX_QUEUES, T.MAX_QUEUE_MEMBERS) == (1 << 24, big)
    assert T.MAX_QUEUES == S.MAX_QUEUES


def test_table_load_refuses_queue_arrays_a_kernel_could_not_trust():
    t = T.TopicTable("cpu", max_topics=2)
    ok = {"seg_off": [0, 1, 1], "row_off": [0, 3, 4, 9], "seg_start": [0, 5, 6], "seg_stride": [1, 1, 1],
          "q_off": [0, 1, 2], "q_seg": [1, 2, 3]}
    t.load(ok)
    assert t.n_queues == 2 and t.stats()["subscribers"] == 3 and t.queue_stats() == {"queues": 2, "members": 6, "segments": 2}
    for bad in ({"q_off": [0, 1, 3]}, {"q_off": [1, 1, 2]}, {"q_off": [0, 2, 1]}, {"q_off": [0, 2]}, {"q_seg": [1, 2, 4]},
                {"q_seg": [0, 2, 3]}, {"q_seg": [1, 1, 3]}, {"q_seg": [1, 3, 2]}, {"q_seg": [2, 3]}, {"q_seg": []},
                {"seg_off": [0, 1, 3]}, {"row_off": [0, 3, 4, 4]}, {"seg_start": [0, 5, MAX_ACTOR]},
                {"row_off": [0, 3, 4, 4 + (1 << 31)]}):
        with pytest.raises(ValueError):
            t.load(dict(ok, **bad))
    with pytest.raises(ValueError):
        t.load({k: v for k, v in ok.items() if k != "q_seg"})
    assert t.host["q_seg"].tolist() == [1, 2, 3]  # a refused load leaves the table as it was
    t.load({"seg_off": [0, 1, 2], "row_off": [0, 3, 4], "seg_start": [0, 5], "seg_stride": [1, 1]})
    assert t.n_queues == 0 and t.host["q_seg"].tolist() == [2] and t.host["q_off"].tolist() == [0, 0, 0]
    assert len(t.device_arrays()) == 4 and len(t.device_arrays(queues=True)) == 6 and len(t.launch_args(t.device)) == 10
    with pytest.raises(ValueError):
        T.TopicTable.from_topics("cpu", {}, max_topics=2, queues={2: [[[0, 1, 1]]]})
    with pytest.raises(ValueError):
        T.TopicTable.from_topics("cpu", {}, max_topics=2, queues={1: [[[0, 1, 1]] * 1025]})


# ---------------------------------------------------------------- by="index": the seq counter
def test_seq_advances_by_q_and_wraps():
    table = T.TopicTable.from_topics("cpu", {0: [[0, 2, 1]]}, max_topics=3, queues={0: [[[10, 5, 1]]], 1: [[[20, 3, 1], [40, 4, 2]]]})
    sc = S.Scatter.topics(table, capacity=64, by="index")
    qs = MsgBatch(torch.tensor([1, 0, 1, 2, 1], dtype=torch.int32), torch.zeros(5, dtype=torch.int64), None, None, METHOD_ECHO)
    members1 = [20, 21, 22, 40, 42, 44, 46]
    assert sc.seq == 0
    e = sc.expand(qs)
    assert e.batch.actor.tolist() == [members1[0], 0, 1, 10 + 1, members1[2], members1[4]] and sc.seq == 5
    e = sc.expand(qs)
    assert e.batch.actor.tolist() == [members1[5], 0, 1, 10 + (6 % 5), members1[7 % 7], members1[9 % 7]] and sc.seq == 10
    sc.seq = (1 << 64) - 3  # q = 0 .. 4 gives 2^64 - 3, - 2, - 1, 0, 1
    e = sc.expand(qs)
    want = [members1[((1 << 64) - 3) % 7], 0, 1, 10 + ((1 << 64) - 2) % 5, members1[((1 << 64) - 1) % 7], members1[1]]
    assert e.batch.actor.tolist() == want and sc.seq == 2
    # a refused expansion and a table without a queue subscription leave the counter alone
    with pytest.raises(ValueError, match="capacity"):
        small = S.Scatter.topics(table, capacity=2, by="index")
        small.expand(qs)
    assert small.seq == 0
    plain = S.Scatter.topics(T.TopicTable.from_topics("cpu", {0: [[0, 2, 1]]}, max_topics=3), by="index")
    plain.expand(qs)
    assert plain.seq == 0
    # by="key" never touches it
    k = S.Scatter.topics(table, capacity=64)
    k.expand(qs)
    assert k.seq == 0 and k.by == "key"


def test_argument_errors_of_the_scatter():
    table = T.TopicTable.from_topics("cpu", {}, max_topics=2, queues={0: [[[0, 4, 1]]]})
    with pytest.raises(ValueError, match="by must be"):
        S.Scatter.topics(table, by="hash")
    sc = S.Scatter.topics(table, capacity=16)
    qs = MsgBatch(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), None, None, METHOD_ECHO)
    for key in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 1, dtype=torch.int64), [0, 0, 0]):
        with pytest.raises(ValueError, match="key must be"):
            sc.expand(qs, key=key)
    off, mem = torch.tensor([0, 2]), torch.tensor([1, 2], dtype=torch.int32)
    for other in (S.Scatter.members(off, mem), S.Scatter.ranges(1, 4)):
        with pytest.raises(ValueError, match="topics rule"):
            other.expand(qs, key=torch.zeros(3, dtype=torch.int64))
    assert S.RULES == ("ranges", "members", "topics")


# ---------------------------------------------------------------- through Join on the CPU runtime
@pytest.fixture
def joined(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, c = cpu_join(tmp_path, ports, topics=16)
    server = C.Server()
    server.RegisterFunc("Calculator.Multiply", lambda args: 0)
    server.Listen(cfg.port, "127.0.0.1")
    clients = [c.NewClient("calculator", C.ConnConfig()), c.NewClient("calculator", C.ConnConfig())]
    try:
        yield c, clients[0], clients[1]
    finally:
        for cl in clients:
            cl.Close()
        server.Close()
        c.Close()


TOPICS_KEYS = {"topics", "segments", "subscribers", "records", "bad_records", "applied_rev", "publishes", "publications",
               "rows", "oob"}


def states(c, n=64):
    """The counter actors' totals: ``METHOD_COUNTER_ADD`` of 0 answers the state."""
    rt = c.runtime
    val, st = rt.send("calculator", MsgBatch(torch.arange(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int64), None,
                                             None, METHOD_COUNTER_ADD))
    assert bool((st == STATUS_OK).all())
    return val.tolist()


def test_queue_subscribe_publish_through_join_cpu(joined):
    c, a, b = joined
    assert c.Stats()["runtime"]["queues"] == {"queues": 0, "members": 0, "segments": 0, "rows": 0}
    a.Subscribe(3, actors=[1, 2, 3], name="all")
    a.Subscribe(3, actors=range(8, 24, 2), name="pool", queue=True)           # 8 workers
    b.Subscribe(3, segments=[[40, 3, 1], [50, 2, 5]], name="pool2", queue=True)  # 5 workers, two segments
    b.Subscribe(5, actors=[60], name="only", queue=True)
    assert a.Topics() == {3: [("all", [[1, 3, 1]])]} == b.Topics()
    want = {3: [("all", [[1, 3, 1]], False), ("pool", [[8, 8, 2]], True), ("pool2", [[40, 3, 1], [50, 2, 5]], True)],
            5: [("only", [[60, 1, 1]], True)]}
    assert a.Topics(queues=True) == want == b.Topics(queues=True)
    st = c.Stats()["runtime"]
    assert set(st["topics"]) == TOPICS_KEYS
    assert (st["topics"]["topics"], st["topics"]["segments"], st["topics"]["subscribers"], st["topics"]["records"]) == (1, 1, 3, 4)
    assert st["queues"] == {"queues": 3, "members": 14, "segments": 4, "rows": 0}

    g = torch.tensor([3, 5, 3, 4, 16, 3, 5, 3], dtype=torch.int32)
    add = torch.tensor([1, 10, 100, 7, 7, 1000, 10000, 100000], dtype=torch.int64)
    key = torch.tensor([11, 22, 33, 44, 55, 11, 22, -9], dtype=torch.int64)
    pubs = MsgBatch(g, add, None, None, METHOD_COUNTER_ADD)
    pool, pool2 = list(range(8, 24, 2)), [40, 41, 42, 50, 55]
    want_state = [0] * 64
    for q in range(8):
        if int(g[q]) == 3:
            for actor in (1, 2, 3, pool[py_pick(8, key=int(key[q]))], pool2[py_pick(5, key=int(key[q]))]):
                want_state[actor] += int(add[q])
        elif int(g[q]) == 5:
            want_state[60] += int(add[q])
    before = states(c)
    assert before == [0] * 64
    ans = b.Publish(pubs, key=key)
    assert ans.count.tolist() == [5, 1, 5, 0, 0, 5, 1, 5] == ans.n_ok.tolist() and ans.oob == 1
    assert ans.n.tolist() == ans.count.tolist()
    assert states(c) == want_state
    # the same key reaches the same member across two Publishes (publications 0 and 5 share key 11)
    ans2 = a.Publish(pubs, key=key)
    assert states(c) == [2 * x for x in want_state]
    assert ans2.count.tolist() == ans.count.tolist()
    # the default key is a0; by="index" walks the members from the scatter's seq
    sc = c.runtime.topics().scatter
    assert sc.seq == 0
    a.Publish(pubs, by="index")
    want_index = [2 * x for x in want_state]
    for q in range(8):
        if int(g[q]) == 3:
            for actor in (1, 2, 3, pool[q % 8], pool2[q % 5]):
                want_index[actor] += int(add[q])
        elif int(g[q]) == 5:
            want_index[60] += int(add[q])
    assert states(c) == want_index and sc.seq == 8
    a.Publish(pubs)  # by key again, the key column a0
    for q in range(8):
        if int(g[q]) == 3:
            for actor in (1, 2, 3, pool[py_pick(8, key=int(add[q]))], pool2[py_pick(5, key=int(add[q]))]):
                want_index[actor] += int(add[q])
        elif int(g[q]) == 5:
            want_index[60] += int(add[q])
    assert states(c) == want_index and sc.seq == 8
    st = c.Stats()["runtime"]
    assert st["queues"] == {"queues": 3, "members": 14, "segments": 4, "rows": 4 * (4 * 2 + 2)}
    assert set(st["topics"]) == TOPICS_KEYS and st["topics"]["rows"] == 4 * 22 and st["topics"]["publishes"] == 4

    # re-subscribing under the same name replaces the subscription: queue -> ordinary -> queue
    a.Subscribe(3, actors=range(8, 24, 2), name="pool")
    assert a.Topics()[3] == [("all", [[1, 3, 1]]), ("pool", [[8, 8, 2]])]
    assert [s[2] for s in a.Topics(queues=True)[3]] == [False, False, True]
    assert b.Publish(pubs).count.tolist() == [12, 1, 12, 0, 0, 12, 1, 12]
    a.Subscribe(3, actors=range(8, 24, 2), name="pool", queue=True)
    assert a.Topics(queues=True) == want and b.Publish(pubs).count.tolist() == [5, 1, 5, 0, 0, 5, 1, 5]
    # Unsubscribe
    b.Unsubscribe(3, name="pool2")
    a.Unsubscribe(5, name="only")
    assert a.Topics(queues=True) == {3: want[3][:2]} and b.Publish(pubs).count.tolist() == [4, 0, 4, 0, 0, 4, 0, 4]
    a.Unsubscribe(3, name="pool")
    assert c.Stats()["runtime"]["queues"]["queues"] == 0
    assert b.Publish(pubs, key=key, by="index").count.tolist() == [3, 0, 3, 0, 0, 3, 0, 3]  # no queue left: key and by change nothing

    # arguments
    with pytest.raises(ValueError, match="by must be"):
        a.Publish(pubs, by="hash")
    for k in (key[:3], key.to(torch.int32), [1] * 8):
        with pytest.raises(ValueError, match="key must be"):
            a.Publish(pubs, key=k)
    with pytest.raises(ValueError, match="topics rule"):
        a.Ask(pubs, S.Scatter.ranges(1, 4), key=key)
    with pytest.raises(ValueError, match="queue"):
        a.Subscribe(1, actors=[1], queue=1)
    # a garbage queue value put by somebody else is counted and breaks nothing
    c.Store.Put(C.background(), "_ptype/topics/calculator/3/odd", '{"segments": [[1, 2, 3]], "queue": "yes"}')
    a.Subscribe(9, actors=[1], name="after")
    st = c.Stats()["runtime"]["topics"]
    assert st["bad_records"] == 1 and st["records"] == 3


def test_an_ephemeral_queue_subscription_lapses_cpu(joined):
    c, a, b = joined
    a.Subscribe(5, actors=[1, 2, 3], name="kept", queue=True)
    a.Subscribe(5, actors=[7, 9], name="gone", queue=True, ephemeral=True)
    assert b.Topics() == {} and [s[0] for s in b.Topics(queues=True)[5]] == ["gone", "kept"]
    pubs = MsgBatch(torch.tensor([5], dtype=torch.int32), torch.tensor([3]), torch.tensor([4]), None, METHOD_CALC_MULTIPLY)
    assert a.Publish(pubs).count.tolist() == [2]
    a._topic_leases[(5, "gone")].stop_keepalive()
    table = c.runtime.topics()
    deadline = time.monotonic() + T.LEASE_TTL_S + 1.0 + 2 * table.relist_s + 2.0
    while len(a.Topics(queues=True)[5]) == 2 and time.monotonic() < deadline:
        table._f.wait_change(50)
    assert a.Topics(queues=True) == {5: [("kept", [[1, 3, 1]], True)]}
    ans = a.Publish(pubs)
    assert ans.count.tolist() == [1] and ans.value.tolist() == [12]
