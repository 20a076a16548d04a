"""Pub/sub topics without a GPU: the ``topics`` rule of ``scatter_ref`` against a sequential
loop over records, ``segments_of``, the compiled flatten on hostile records, and Subscribe /
Publish / Unsubscribe through a real one-member ``Join`` on the CPU runtime."""
import json
import time

import numpy as np
import pytest
import torch

from ptype_amd import _core
from ptype_amd import cluster as C
from ptype_amd.ops import gather as G
from ptype_amd.ops import scatter as S
from ptype_amd.ops import topics as T
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_ECHO, STATUS_NO_ACTOR, STATUS_OK

from test_scatter import FIELDS, same_expansion

MAX_ACTOR = (1 << 31) - 2


def rec(*segments):
    return json.dumps({"segments": [list(s) for s in segments]})


# ---------------------------------------------------------------- scatter_ref against the loop
def loop_oracle(records, max_topics, qs):
    """Publication by publication, record by record (key order), segment by segment, id by id."""
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
        for key in sorted(records):
            topic, _name = key.split("/", 1)
            if int(topic) != g:
                continue
            for start, count, stride in json.loads(records[key])["segments"]:
                for k in range(count):
                    rows.append((start + stride * k, int(qs.a0[q]), None if qs.a1 is None else int(qs.a1[q]), m, q))
        n.append(len(rows) - before)
    return rows, first, n, oob


RECORDS = {"3/b": rec([0, 4, 2], [100, 1, 1]), "3/a": rec([7, 3, 5]), "0/x": rec([MAX_ACTOR - 6, 3, 3]),
           "10/n1": rec([5, 2, 1]), "10/n0": rec([5, 1, 1], [5, 1, 1]), "2/solo": rec([9, 1, 1])}


@pytest.mark.parametrize("method_col", [False, True])
def test_topics_reference_against_the_loop(method_col):
    g = [3, 10, 0, 1, 11, -1, 3, 2, 1 << 20, 10, -(1 << 31), (1 << 31) - 1]
    method = [METHOD_CALC_MULTIPLY, METHOD_ECHO] * (len(g) // 2) if method_col else METHOD_ECHO
    qs = MsgBatch(torch.tensor(g, dtype=torch.int32), torch.arange(len(g), dtype=torch.int64) * 3 - 7,
                  torch.arange(len(g), dtype=torch.int64) + (1 << 40), None,
                  torch.tensor(method, dtype=torch.int16) if method_col else method)
    flat = T.flatten_records(RECORDS, 11)
    assert flat["bad_records"] == 0 and flat["records"] == 6 and flat["topics"] == 4
    table = T.TopicTable("cpu", max_topics=11)
    table.load(flat)
    sc = S.Scatter.topics(table, capacity=64)
    ref = S.scatter_ref(sc, qs)
    rows, first, n, oob = loop_oracle(RECORDS, 11, qs)
    assert ref["total"] == len(rows) and ref["oob"] == oob == 5
    assert ref["first"].tolist() == first and ref["n"].tolist() == n
    assert ref["actor"].tolist() == [r[0] for r in rows] and ref["a0"].tolist() == [r[1] for r in rows]
    assert ref["a1"].tolist() == [r[2] for r in rows] and ref["a2"] is None
    assert ref["group"].tolist() == [r[4] for r in rows]
    if method_col:
        assert ref["method"].tolist() == [r[3] for r in rows]
    # key order within a topic, duplicates kept: topic 10 is n0's 5, 5 then n1's 5, 6
    at = first[1]
    assert ref["actor"].tolist()[at:at + 4] == [5, 5, 5, 6]
    assert int(ref["actor"].max()) == MAX_ACTOR
    same_expansion(sc.expand(qs), ref)  # the CPU expand is the reference
    assert table.view() == {0: [("x", [[MAX_ACTOR - 6, 3, 3]])], 2: [("solo", [[9, 1, 1]])],
                            3: [("a", [[7, 3, 5]]), ("b", [[0, 4, 2], [100, 1, 1]])],
                            10: [("n0", [[5, 1, 1], [5, 1, 1]]), ("n1", [[5, 2, 1]])]}
    with pytest.raises(ValueError, match="capacity"):
        S.Scatter.topics(table, capacity=3).expand(qs)


def test_rules_and_limits():
    assert S.RULES == ("ranges", "members", "topics")
    lim = _core.topic_limits()
    assert (lim["max_segments_per_record"], lim["max_actor"], lim["max_segments"], lim["max_topics"]) == \
        (T.MAX_RECORD_SEGMENTS, T.MAX_ACTOR, T.MAX_SEGMENTS, T.MAX_TOPICS)
    assert T.MAX_SEGMENTS == S.MAX_SEGMENTS
    with pytest.raises(ValueError):
        S.Scatter.topics(object())
    with pytest.raises(ValueError):
        S.Scatter.ranges(1, 1).set_table(T.TopicTable("cpu"))


# ---------------------------------------------------------------- segments_of
def test_segments_of_round_trip():
    gen = torch.Generator().manual_seed(5)
    for k in range(40):
        ids = torch.randint(0, 50 + 40 * k, (k * 7,), generator=gen)
        segs = T.segments_of(ids)
        assert T.flatten_segments(segs).tolist() == sorted(set(ids.tolist()))
        assert segs == T.segments_of(ids.flip(0).tolist()) and (not segs or segs == T.check_segments(segs))
    assert T.segments_of([]) == [] and T.segments_of(torch.zeros(0, dtype=torch.int64)) == []


def test_segments_of_cuts_greedily_from_the_left():
    assert T.segments_of(range(3, 3000, 7)) == [[3, len(range(3, 3000, 7)), 7]]  # a progression: one segment
    assert T.segments_of(np.arange(0, 1 << 20)) == [[0, 1 << 20, 1]]
    assert T.segments_of([9]) == [[9, 1, 1]] and T.segments_of([9, 9, 9]) == [[9, 1, 1]]
    assert T.segments_of([4, 10]) == [[4, 2, 6]]
    assert T.segments_of([0, 1, 5, 6]) == [[0, 2, 1], [5, 2, 1]]  # two-element runs
    assert T.segments_of([0, 1, 3, 5]) == [[0, 2, 1], [3, 2, 2]]  # the left run takes what repeats its stride
    assert T.segments_of([0, 2, 4, 5, 6, 7, 20]) == [[0, 3, 2], [5, 3, 1], [20, 1, 1]]  # a last lone id
    assert T.segments_of([5, 1, 3, 7, 7, 20, 21, 40]) == [[1, 4, 2], [20, 2, 1], [40, 1, 1]]
    assert T.segments_of([0, MAX_ACTOR]) == [[0, 2, MAX_ACTOR]]
    with pytest.raises(ValueError):
        T.check_segments(T.segments_of([0, MAX_ACTOR + 1]))
    with pytest.raises(ValueError):
        T.check_segments([])
    with pytest.raises(ValueError):
        T.check_segments([[0, 1, 1]] * 1025)


# ---------------------------------------------------------------- the compiled flatten on hostile records
HOSTILE = {
    "bad json": ("4/a", '{"segments": [[1, 2, 3]'),
    "not an object": ("4/a", "[[1, 2, 3]]"),
    "no segments": ("4/a", '{"segment": [[1, 2, 3]]}'),
    "empty": ("4/a", '{"segments": []}'),
    "count 0": ("4/a", rec([1, 0, 1])),
    "stride 0": ("4/a", rec([1, 2, 0])),
    "negative start": ("4/a", rec([-1, 2, 1])),
    "negative count": ("4/a", rec([1, -2, 1])),
    "end past 2^31 - 2": ("4/a", rec([MAX_ACTOR, 2, 1])),
    "end past 2^31 - 2 by the stride": ("4/a", rec([1, 3, 1 << 30])),
    "a product past int64": ("4/a", rec([0, 1 << 31, 1 << 31])),
    "a number past int64": ("4/a", '{"segments": [[1, 99999999999999999999999, 1]]}'),
    "a float": ("4/a", '{"segments": [[1, 2.5, 1]]}'),
    "a string field": ("4/a", '{"segments": [["1", 2, 1]]}'),
    "two fields": ("4/a", '{"segments": [[1, 2]]}'),
    "four fields": ("4/a", '{"segments": [[1, 2, 1, 1]]}'),
    "1025 segments": ("4/a", rec(*[[k, 1, 1] for k in range(1025)])),
    "nested deep": ("4/a", "[" * 100000),
    "nested deep in segments": ("4/a", '{"segments": ' + "[" * 50000 + "]" * 50000 + "}"),
    "huge": ("4/a", '{"segments": [[1, 2, 3]], "pad": "' + "x" * (1 << 18) + '"}'),
    "topic max_topics": ("8/a", rec([1, 2, 3])),
    "topic far out": ("99999999999999999999/a", rec([1, 2, 3])),
    "non-numeric topic": ("four/a", rec([1, 2, 3])),
    "negative topic": ("-1/a", rec([1, 2, 3])),
    "topic with a sign": ("+4/a", rec([1, 2, 3])),
    "topic with a leading zero": ("04/a", rec([1, 2, 3])),
    "no name": ("4/", rec([1, 2, 3])),
    "no topic": ("/a", rec([1, 2, 3])),
    "no slash": ("4", rec([1, 2, 3])),
    "empty key": ("", rec([1, 2, 3])),
}


@pytest.mark.parametrize("what", sorted(HOSTILE))
def test_flatten_skips_and_counts_a_hostile_record(what):
    key, value = HOSTILE[what]
    good = {"3/z": rec([10, 2, 5]), "4/0": rec([1, 1, 1]), "4/z": rec([7, 3, 1]), "5/a": rec([0, 2, 2])}
    flat = T.flatten_records(dict(good, **{key: value}), 8)
    want = T.flatten_records(good, 8)
    assert flat["records"] == 5 and flat["bad_records"] == 1 and want["bad_records"] == 0
    for k in ("seg_off", "row_off", "seg_start", "seg_stride"):
        assert flat[k].dtype == want[k].dtype and flat[k].tolist() == want[k].tolist(), k
    assert flat["subs"] == want["subs"] == [(3, "z", 0, 1), (4, "0", 1, 1), (4, "z", 2, 1), (5, "a", 3, 1)]
    assert flat["row_off"].tolist() == [0, 2, 3, 6, 8] and flat["seg_off"].tolist() == [0, 0, 0, 0, 1, 3, 4, 4, 4]
    assert (flat["topics"], flat["segments"], flat["subscribers"]) == (3, 4, 8)


def test_flatten_accepts_the_edges():
    flat = T.flatten_records({"0/a": rec(*[[k, 1, 1] for k in range(1024)]), "7/b": rec([MAX_ACTOR, 1, 1 << 30]),
                              "7/c": rec([0, 2, MAX_ACTOR]), "7/d": ' {"other": {"x": [1]}, "segments" : [ [ 0 , 1 , 1 ] ] } '},
                             8)
    assert flat["bad_records"] == 0 and flat["segments"] == 1027 and flat["subscribers"] == 1024 + 1 + 2 + 1
    assert flat["seg_off"].tolist() == [0] + [1024] * 7 + [1027]
    with pytest.raises(ValueError):
        T.flatten_records({}, 0)
    with pytest.raises(ValueError):
        T.flatten_records({}, (1 << 20) + 1)
    assert T.flatten_records({}, 1 << 20)["seg_off"].size == (1 << 20) + 1


def test_table_load_refuses_arrays_a_kernel_could_not_trust():
    t = T.TopicTable("cpu", max_topics=2)
    ok = {"seg_off": [0, 1, 2], "row_off": [0, 3, 4], "seg_start": [0, 5], "seg_stride": [1, 1]}
    t.load(ok)
    for bad in ({"seg_off": [0, 1, 3]}, {"seg_off": [0, 2, 1]}, {"row_off": [0, 3, 3]}, {"row_off": [1, 3, 4]},
                {"seg_start": [-1, 5]}, {"seg_stride": [0, 1]}, {"seg_start": [MAX_ACTOR - 1, 5]}, {"seg_off": [0, 2]},
                {"row_off": [0, 3]}):
        with pytest.raises(ValueError):
            t.load(dict(ok, **bad))
    assert t.host["row_off"].tolist() == [0, 3, 4]  # a refused load leaves the table as it was


# ---------------------------------------------------------------- through Join on the CPU runtime
def cpu_join(tmp_path, ports, topics=None):
    pp, pc = ports(), ports()
    cfg = C.Config()
    cfg.service_name, cfg.node_name, cfg.port = "calculator", "node0", ports()
    cfg.member = C.member_config(name="m0", dir=str(tmp_path / "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                 apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                 acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                 heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
    cfg.has_gpu = True
    cfg.gpu.cpu, cfg.gpu.actors, cfg.gpu.max_batch = True, 64, 1 << 12
    if topics is not None:
        cfg.gpu.topics = topics
    return cfg, C.Join(C.background(), cfg)


@pytest.fixture
def joined(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, c = cpu_join(tmp_path, ports, topics=16)
    server = C.Server()  # NewClient dials the registered node, as the reference does
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


def pubs_batch():
    return MsgBatch(torch.tensor([3, 4, 3, 16, -1, 9], dtype=torch.int32), torch.arange(6, dtype=torch.int64) + 2,
                    torch.full((6,), 7, dtype=torch.int64), None, METHOD_CALC_MULTIPLY)


def test_subscribe_publish_unsubscribe_through_join_cpu(joined):
    c, a, b = joined
    zero = {"topics": 0, "segments": 0, "subscribers": 0, "records": 0, "bad_records": 0, "applied_rev": 0,
            "publishes": 0, "publications": 0, "rows": 0, "oob": 0}
    assert c.Stats()["runtime"]["topics"] == zero and not c.runtime._topics  # nothing is created or watched yet
    assert c.runtime.max_topics == 16
    r1 = a.Subscribe(3, actors=range(0, 64, 2))
    r2 = b.Subscribe(3, segments=[[1, 5, 1], [5, 1, 1]], name="other")
    r3 = b.Subscribe(9, actors=[60, 61, 62, 63, 64, 65])  # two ids past the service's actors
    assert r1 < r2 < r3 and c.runtime.topics().applied_rev >= r3
    want = {3: [("node0", [[0, 32, 2]]), ("other", [[1, 5, 1], [5, 1, 1]])], 9: [("node0", [[60, 6, 1]])]}
    assert a.Topics() == want and b.Topics() == want  # two clients of one cluster agree
    pubs = pubs_batch()
    sc = S.Scatter.topics(T.TopicTable.from_topics("cpu", {g: sum((s for _, s in subs), []) for g, subs in want.items()},
                                                   max_topics=16))
    ref = S.scatter_ref(sc, pubs)
    assert ref["n"].tolist() == [38, 0, 38, 0, 0, 6] and ref["oob"] == 2
    plain = a.Send(MsgBatch(ref["actor"], ref["a0"], ref["a1"], None, METHOD_CALC_MULTIPLY))
    for op in ("sum", "max"):
        ans = b.Publish(pubs, op=op)
        assert torch.equal(ans.val, plain[0]) and torch.equal(ans.st, plain[1])
        g = G.gather_ref(plain[0], plain[1], ref["group"], pubs.M, op)
        for f in FIELDS:
            assert torch.equal(getattr(ans, f), g[f]), (op, f)
        assert torch.equal(ans.first, ref["first"]) and torch.equal(ans.n, ref["n"]) and ans.oob == 2
    assert ans.count.tolist() == [38, 0, 38, 0, 0, 6] and ans.n_ok.tolist() == [38, 0, 38, 0, 0, 4]
    assert ans.status.tolist() == [STATUS_OK] * 5 + [STATUS_NO_ACTOR]
    st = c.Stats()["runtime"]["topics"]
    assert st == {"topics": 2, "segments": 4, "subscribers": 44, "records": 3, "bad_records": 0, "applied_rev": st["applied_rev"],
                  "publishes": 2, "publications": 12, "rows": 164, "oob": 4} and st["applied_rev"] >= r3
    # the same name replaces the subscription
    r4 = a.Subscribe(3, segments=[[2, 2, 1]])
    assert r4 > r3 and a.Topics()[3] == [("node0", [[2, 2, 1]]), ("other", [[1, 5, 1], [5, 1, 1]])]
    assert b.Publish(pubs).count.tolist() == [8, 0, 8, 0, 0, 6]
    # Unsubscribe
    r5, r6, r7 = a.Unsubscribe(3), b.Unsubscribe(3, name="other"), a.Unsubscribe(9)
    assert r4 < r5 < r6 < r7 and a.Topics() == {}
    a.Unsubscribe(3)  # one that does not exist is not an error
    ans = a.Publish(pubs)
    assert ans.count.tolist() == [0] * 6 and ans.oob == 2 and ans.val.numel() == 0
    st = c.Stats()["runtime"]["topics"]
    assert (st["topics"], st["segments"], st["subscribers"], st["records"], st["oob"]) == (0, 0, 0, 0, 8)
    # arguments
    for kw in ({}, {"actors": [1], "segments": [[1, 1, 1]]}):
        with pytest.raises(ValueError, match="exactly one"):
            a.Subscribe(1, **kw)
    for topic in (-1, 16):
        with pytest.raises(ValueError, match="topic must be in"):
            a.Subscribe(topic, actors=[1])
    for segs in ([[0, 0, 1]], [[0, 1, 0]], [[-1, 1, 1]], [[MAX_ACTOR, 2, 1]], [], [[0, 1, 1]] * 1025):
        with pytest.raises(ValueError):
            a.Subscribe(1, segments=segs)
    with pytest.raises(ValueError, match="name"):
        a.Subscribe(1, actors=[1], name="a/b")
    assert a.Topics() == {}


def test_a_garbage_record_raises_bad_records_and_breaks_nothing_cpu(joined):
    c, a, b = joined
    a.Subscribe(3, actors=[1, 2, 3])
    ctx = C.background()
    c.Store.Put(ctx, "_ptype/topics/calculator/3/garbage", "\x00not json {{{")
    c.Store.Put(ctx, "_ptype/topics/calculator/nonsense", "{}")
    c.Store.Put(ctx, "_ptype/topics/calculator/16/far", rec([1, 2, 3]))
    c.Store.Put(ctx, "_ptype/topics/calculator/3/zero", rec([1, 0, 1]))
    rev = a.Subscribe(4, actors=[9], name="after")  # (its own mirror is waited for: the puts above are applied)
    st = c.Stats()["runtime"]["topics"]
    assert (st["records"], st["bad_records"], st["topics"], st["subscribers"]) == (6, 4, 2, 4) and st["applied_rev"] >= rev
    assert a.Topics() == {3: [("node0", [[1, 3, 1]])], 4: [("after", [[9, 1, 1]])]}
    ans = b.Publish(pubs_batch())
    assert ans.count.tolist() == [3, 1, 3, 0, 0, 0] and ans.n_ok.tolist() == [3, 1, 3, 0, 0, 0]
    val, st = a.Send(MsgBatch(torch.arange(64, dtype=torch.int32), torch.arange(64), torch.arange(64), None,
                              METHOD_CALC_MULTIPLY))
    assert torch.equal(val, torch.arange(64) ** 2) and bool((st == STATUS_OK).all())


def test_an_ephemeral_subscription_lapses_with_its_owner_cpu(joined):
    c, a, b = joined
    a.Subscribe(5, actors=[1, 2, 3], name="kept")
    a.Subscribe(5, actors=[7], name="gone", ephemeral=True)
    b.Subscribe(6, actors=[8], ephemeral=True)
    assert b.Topics() == {5: [("gone", [[7, 1, 1]]), ("kept", [[1, 3, 1]])], 6: [("node0", [[8, 1, 1]])]}
    # closed by Unsubscribe: at once
    b.Unsubscribe(6)
    assert 6 not in a.Topics() and not b._topic_leases
    # closed by Client.Close: the lease is revoked, the watch brings the delete
    d = c.NewClient("calculator", C.ConnConfig())
    d.Subscribe(7, actors=[1], name="closing", ephemeral=True)
    assert a.Topics()[7] == [("closing", [[1, 1, 1]])]
    d.Close()
    deadline = time.monotonic() + 5.0
    while 7 in a.Topics() and time.monotonic() < deadline:
        c.runtime.topics()._f.wait_change(50)
    assert 7 not in a.Topics() and not d._topic_leases
    # its owner stops refreshing: the lease lapses, the store deletes the record
    a._topic_leases[(5, "gone")].stop_keepalive()
    table = c.runtime.topics()
    deadline = time.monotonic() + T.LEASE_TTL_S + 1.0 + 2 * table.relist_s + 2.0  # TTL + grace + the re-list period (+ slack)
    while len(a.Topics()[5]) == 2 and time.monotonic() < deadline:
        table._f.wait_change(50)
    assert a.Topics() == {5: [("kept", [[1, 3, 1]])]}
    assert a.Publish(pubs_batch()).count.tolist() == [0] * 6
    pubs = MsgBatch(torch.tensor([5], dtype=torch.int32), torch.tensor([3]), torch.tensor([4]), None, METHOD_CALC_MULTIPLY)
    ans = a.Publish(pubs)
    assert ans.count.tolist() == [3] and ans.value.tolist() == [36]


def test_topics_need_a_control_plane_and_the_config_key(tmp_path):
    from ptype_amd.runtime import DeviceRuntime

    rt = DeviceRuntime(torch.device("cpu"), actors=8, service="calculator")
    rt.place_local()
    try:
        with pytest.raises(RuntimeError, match="control plane"):
            rt.topics()
        with pytest.raises(RuntimeError, match="control plane"):
            rt.publish("calculator", pubs_batch())
        assert rt.stats()["topics"]["publishes"] == 0
        # a table that follows no store, installed by hand
        rt.topics("calculator", table=T.TopicTable.from_topics("cpu", {3: [[0, 8, 1]]}, max_topics=16))
        ans = rt.publish("calculator", pubs_batch())
        assert ans.count.tolist() == [8, 0, 8, 0, 0, 0] and ans.value.tolist() == [8 * 14, 0, 8 * 28, 0, 0, 0]
        with pytest.raises(RuntimeError, match="follows no store"):
            rt.topics().wait(1)
    finally:
        rt.close()
    with pytest.raises(ValueError):
        DeviceRuntime(torch.device("cpu"), actors=8, max_topics=0)
    # gpu.topics
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    assert C.Config().gpu.topics == 1024
    for text, want in (("gpu: {cpu: true}", 1024), ("gpu: {topics: 1}", 1), ("gpu: {topics: 1048576}", 1 << 20)):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\n{text}\n")
        assert C.ConfigFromFile(str(p)).gpu.topics == want
    for bad in ("0", "-3", "1048577", "many", "true"):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\ngpu:\n  topics: {bad}\n")
        with pytest.raises(C.ConfigError):
            C.ConfigFromFile(str(p))
