"""Topic queue subscriptions on the GPU: the QUEUES variant of the scatter's ``topics`` rule
(csrc/hip/scatter.hip) against the numpy reference by exact equality, on a table built so that
the ordinary/queue boundary of a publication falls on every place the kernel treats apart, and
``publish`` through the runtime, a captured graph, in-process ranks and Join."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import gather as G
from ptype_amd.ops import hip
from ptype_amd.ops import scatter as S
from ptype_amd.ops import topics as T
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, STATUS_NO_ACTOR,
                                   STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange, SendGraph

from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_ledger_gpu import _join
from test_scatter import FIELDS, same_expansion
from test_scatter_gpu import TE, TQ

pytestmark = pytest.mark.gpu

CAP, QCAP = 1 << 15, 2048
MAX_ACTOR = (1 << 31) - 2
BIG = (1 << 31) - 1
M64 = (1 << 64) - 1
GIANT_ORD, GIANT_QUEUES = 3 * TE + 100, 2 * TE


def the_layout():
    """Topics, queue subscriptions and the topic column.  With the 2048-row tile and the 4-row
    quad, the publications' rows fall as the comments say (asserted by the test)."""
    gen = torch.Generator().manual_seed(41)
    cuts = torch.sort(torch.randperm(GIANT_ORD - 1, generator=gen)[:499] + 1).values.tolist()
    giant = [[int(torch.randint(0, 1 << 20, (1,), generator=gen)), b - a, 1 + (i % 3)]
             for i, (a, b) in enumerate(zip([0] + cuts, cuts + [GIANT_ORD]))]
    topics = {0: [[0, 5, 1], [100, TE - 5, 3]],       # rows 0 .. 2047 ordinary, the queue rows from 2048
              1: [[7, 3, 2]], 2: [[9, 1, 1]], 3: [[20, 2, 1], [30, 1, 1]], 6: [[40, 2, 5]], 8: giant,
              10: [[1, 2, 1], [50, 3, 7]]}
    unit = [[3 * k + 1, 1, 1] for k in range(1024)]    # 1024 length-1 segments: the full bisection depth
    queues = {0: [[[0, 9, 1]], [[5, 2, 1], [90, 4, 2]], [[77, 1, 1]]],
              1: [[[1, 3, 1]], [[100, 5, 5], [3, 2, 1]]],
              2: [[[11, 4, 1]], [[12, 1, 1]], [[13, 2, 9]]],
              3: [[[200, 6, 1]]],
              4: [unit, [[123456, 1, 1]], [[MAX_ACTOR - 6 * 11, 7, 11]], [[8, 3, 1], [800, 3, 2], [8000, 3, 3]]],
              5: [[[60, 2, 1]], [[70, 5, 1]]],
              8: [[[k, 1 + k % 5, 1 + k % 2]] if k % 3 else [[k, 2, 1], [9 * k, 1 + k % 4, 3]] for k in range(GIANT_QUEUES)],
              9: [[[0, BIG, 1]]],                       # start 0, stride 1, count 2^31 - 1
              10: [[[1000, 3, 1], [2000, 2, 1], [3000, 2, 1]]]}
    head = [0,      # 2048 ordinary rows, then 3 queue rows: the boundary at rows 2047 / 2048
            1,      # rows 2051 .. 2055: the quad 2052 .. 2055 is 2 ordinary + 2 queue rows
            2,      # rows 2056 .. 2059: 1 + 3
            3,      # rows 2060 .. 2063: 3 + 1
            4,      # rows 2064 .. 2067: four queue rows of four subscriptions
            5, 6,   # rows 2068 .. 2071: a quad of two publications, the first ends in queue rows
            7, 12,  # a topic without a row, a topic out of range
            8,      # the giant: tiles inside one publication, with its boundary and with queue rows only
            9, 9, 9, -1, 10]
    fill = [10, 4, 7, 1, 2, 3, 5, 6, 9, 12, -1, (1 << 31) - 1, 11]
    g = head + [fill[i % len(fill)] for i in range(TQ + 70 - len(head))]  # Q straddles a count tile
    return topics, queues, g


@pytest.fixture(scope="module")
def layout():
    return build_layout("cuda")


def build_layout(device):
    topics, queues, g = the_layout()
    table = T.TopicTable.from_topics(device, topics, max_topics=12, queues=queues)
    Q = len(g)
    gen = torch.Generator().manual_seed(42)
    # keys that pick near both ends of the 2^31 - 1 members, found on the host
    cand = np.arange(200000, dtype=np.int64)
    m = S.queue_pick(BIG, key=cand).astype(np.int64)
    lo, hi = int(cand[m.argmin()]), int(cand[m.argmax()])
    assert m.min() < 1 << 16 and m.max() > BIG - (1 << 16)
    cols = []
    for _ in range(4):  # a0, a1, a2 and a key column of its own
        c = torch.randint(-2**62, 2**62, (Q,), generator=gen)
        c[10], c[11], c[12], c[14], c[15], c[16], c[17] = lo, hi, -1, 0, -(1 << 63), (1 << 63) - 1, 1
        cols.append(c)
    method = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO], dtype=torch.int16)[torch.randint(0, 2, (Q,), generator=gen)]
    return {"table": table, "g": torch.tensor(g, dtype=torch.int32), "cols": cols, "method": method, "lo": lo, "hi": hi,
            "sc": S.Scatter.topics(table, capacity=CAP, q_capacity=QCAP)}


def check(sc, qs, key=None, qs_gpu=None, key_gpu=None):
    """Expand on the device and compare with the reference (computed before: by="index" reads seq)."""
    ref = S.scatter_ref(sc, qs, key=key)
    seq = sc.seq
    exp = sc.expand(_cuda(qs) if qs_gpu is None else qs_gpu,
                    key=key_gpu if key_gpu is not None else None if key is None else key.cuda())
    assert exp.batch.M == exp.total == exp.group.numel() and exp.first.numel() == exp.n.numel() == qs.M
    same_expansion(exp, ref)
    if sc.by == "index" and sc.table.n_queues and qs.M:
        assert sc.seq == (seq + qs.M) & M64
    else:
        assert sc.seq == seq
    return exp, ref


def test_constants_match_the_module():
    assert hip().scatter_limits()["max_queues"] == S.MAX_QUEUES == T.MAX_QUEUES
    assert tuple(hip().scatter_limits()["rules"]) == S.RULES == ("ranges", "members", "topics")
    assert hip().scatter_expand_tile() == TE == 2048 and hip().scatter_question_tile() == TQ == 1024


VARIANTS = {"a0 as the key": dict(cols=3, method_col=False, own_key=False, unaligned=False),
            "a key column": dict(cols=2, method_col=True, own_key=True, unaligned=False),
            "a0 only": dict(cols=1, method_col=False, own_key=True, unaligned=False),
            "unaligned views": dict(cols=3, method_col=True, own_key=True, unaligned=True)}


@pytest.mark.parametrize("by", ["key", "index"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_queue_kernels_against_reference(layout, variant, by):
    v = VARIANTS[variant]
    a0, a1, a2, kcol = layout["cols"]
    qs = MsgBatch(layout["g"], a0, a1 if v["cols"] > 1 else None, a2 if v["cols"] > 2 else None,
                  layout["method"] if v["method_col"] else METHOD_ECHO)
    key = kcol if v["own_key"] else None
    sc = layout["sc"]
    sc.by, sc.seq = by, (1 << 64) - 3
    qg = kg = None
    if v["unaligned"]:
        off1 = (lambda t: torch.cat([t[:1], t]).cuda()[1:])
        qg = MsgBatch(off1(qs.actor), off1(qs.a0), off1(qs.a1), off1(qs.a2), off1(qs.method))
        kg = off1(key)
        assert qg.actor.data_ptr() % 16 == 4 and qg.a0.data_ptr() % 16 == 8 and kg.data_ptr() % 16 == 8
    exp, ref = check(sc, qs, key=key, qs_gpu=qg, key_gpu=kg)
    # the layout the cases rest on
    first, n = ref["first"].tolist(), ref["n"].tolist()
    assert first[:7] == [0, TE + 3, TE + 8, TE + 12, TE + 16, TE + 20, TE + 22] and n[:9] == [TE + 3, 5, 4, 4, 4, 2, 2, 0, 0]
    assert n[9] == GIANT_ORD + GIANT_QUEUES and first[9] == TE + 24 and n[10:15] == [1, 1, 1, 0, 6]
    boundary = first[9] + GIANT_ORD
    tile = boundary // TE  # a tile inside the giant publication that holds its ordinary / queue boundary
    assert first[9] < tile * TE and (tile + 1) * TE <= first[10] and tile * TE < boundary < (tile + 1) * TE
    assert (tile + 2) * TE <= first[10] and first[9] + GIANT_ORD <= (tile + 1) * TE  # and a tile of queue rows only
    assert first[9] // TE + 3 <= tile  # tiles of ordinary rows only before it
    assert ref["oob"] == sum(1 for x in layout["g"].tolist() if not 0 <= x < 12) > 0 and qs.M > TQ
    actor = ref["actor"].tolist()
    if by == "key":
        k = a0 if key is None else key
        assert actor[first[10]] == int(S.queue_pick(BIG, key=np.int64(layout["lo"]))) < 1 << 16
        assert actor[first[11]] == int(S.queue_pick(BIG, key=np.int64(layout["hi"]))) > BIG - (1 << 16)
        assert actor[first[12]] == 1516776189 and int(k[12]) == -1
    else:
        seq = (1 << 64) - 3  # publication q takes (seq + q) mod 2^64: 7 for q = 10, 1 for q = 4
        assert actor[first[10]] == ((seq + 10) & M64) % BIG == 7 and actor[first[4]] == 3 * (((seq + 4) & M64) % 1024) + 1 == 4
    assert actor[first[4] + 1] == 123456                                         # a single member
    assert max(actor[first[q] + 2] for q in range(qs.M) if layout["g"][q] == 4) == MAX_ACTOR  # a member with the last id 2^31 - 2
    assert min(actor) >= 0 and max(actor) <= MAX_ACTOR


def test_tables_replaced_queue_none_queue(layout):
    topics, queues, _ = the_layout()
    del topics[8], queues[8]
    g = torch.tensor([0, 4, 7, 10, 12, 1, 9, 5], dtype=torch.int32)
    qs = MsgBatch(g, torch.arange(8, dtype=torch.int64) * 77 - 5, torch.arange(8, dtype=torch.int64), None, METHOD_ECHO)
    with_q = T.TopicTable.from_topics("cuda", topics, max_topics=12, queues=queues)
    plain = T.TopicTable.from_topics("cuda", topics, max_topics=12)
    sc = S.Scatter.topics(with_q, capacity=CAP, q_capacity=QCAP)
    e1, r1 = check(sc, qs)
    a1 = e1.batch.actor.clone()
    sc.set_table(plain)
    e2, r2 = check(sc, qs)
    # the middle table gives exactly what a plain topics scatter gives
    other = S.Scatter.topics(plain, capacity=CAP, q_capacity=QCAP).expand(_cuda(qs))
    assert e2.total == other.total == r2["total"] < r1["total"] and torch.equal(e2.batch.actor, other.batch.actor)
    assert torch.equal(e2.first, other.first) and torch.equal(e2.n, other.n) and torch.equal(e2.group, other.group)
    assert r2["n"].tolist() == [TE, 0, 0, 5, 0, 3, 0, 0]
    sc.set_table(with_q)
    e3, r3 = check(sc, qs)
    assert torch.equal(e3.batch.actor, a1) and r3["n"].tolist() == [TE + 3, 4, 0, 6, 0, 5, 1, 2]
    # one TopicTable whose arrays are replaced in place (what a follower's apply does)
    with_q.load(plain.host)
    check(sc, qs)
    with_q.load(T.TopicTable.from_topics("cpu", {}, max_topics=12, queues={4: [[[5, 1, 1]]]}).host)  # no ordinary segment at all
    e, r = check(sc, qs)
    assert r["n"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and e.batch.actor.cpu().tolist() == [5]


def test_capacity_is_exact_and_refused_before_a_row_is_written():
    cap = TE + 5
    table = T.TopicTable.from_topics("cuda", {0: [[0, TE, 1]], 1: [[7, 2, 3]]}, max_topics=4,
                                     queues={0: [[[3, 9, 1]]], 1: [[[1, 3, 1]], [[4, 4, 4]]], 2: [[[0, 6, 1]]]})
    sc = S.Scatter.topics(table, capacity=cap, q_capacity=8)
    mk = (lambda g: MsgBatch(torch.tensor(g, dtype=torch.int32), torch.arange(len(g), dtype=torch.int64), None, None,
                             METHOD_ECHO))
    exp, ref = check(sc, mk([0, 3, 1]))
    assert exp.total == cap
    with pytest.raises(ValueError, match=f"{cap + 1} rows, the capacity is {cap}"):
        sc.expand(_cuda(mk([0, 2, 1])))
    torch.cuda.synchronize()
    for name in ("actor", "a0", "group"):  # the buffers still hold the previous expansion
        assert torch.equal(getattr(sc, name).cpu(), ref[name]), name


def test_launchers_validate_the_queue_arguments():
    table = T.TopicTable.from_topics("cuda", {0: [[0, 4, 1]]}, max_topics=4, queues={0: [[[9, 2, 1]]]})
    sc = S.Scatter.topics(table, capacity=64, q_capacity=8)
    qs = _cuda(MsgBatch(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), None, None, METHOD_ECHO))
    sc.expand(qs)
    seg_off, row_off, seg_start, seg_stride, q_off, q_seg = table.device_arrays(queues=True)
    p = (lambda t: t.data_ptr())
    count = (lambda **kw: hip().scatter_count(2, p(qs.actor), p(qs.a0), 2, 1, p(seg_off), 4, p(sc.n), p(sc.first),
                                              p(sc.tsum), p(sc.toob), sc.tile_cap, p(sc.ctr), 0, row_off=p(row_off),
                                              n_segs=1, **kw))
    with pytest.raises(ValueError, match="q_off"):
        count(n_queues=1)
    with pytest.raises(ValueError, match="q_off"):
        count(q_off=p(q_off) + 4, n_queues=1)
    with pytest.raises(ValueError, match="n_queues"):
        count(q_off=p(q_off), n_queues=(1 << 24) + 1)
    expand = (lambda **kw: hip().scatter_expand(2, p(qs.actor), p(qs.a0), 0, 0, 0, 2, 1, 1, 0, False, 0, p(seg_off), 0, 4, 0,
                                                p(sc.first), p(sc.n), 10, 64, p(sc.actor), p(sc.a0), 0, 0, 0, p(sc.group),
                                                0, row_off=p(row_off), seg_start=p(seg_start), seg_stride=p(seg_stride),
                                                n_segs=1, q_off=p(q_off), n_queues=1, **kw))
    with pytest.raises(ValueError, match="q_seg"):
        expand(n_all=2, key=p(qs.a0))
    with pytest.raises(ValueError, match="n_all"):
        expand(q_seg=p(q_seg), n_all=(1 << 24) + 1, key=p(qs.a0))
    with pytest.raises(ValueError, match="key"):
        expand(q_seg=p(q_seg), n_all=2)
    with pytest.raises(ValueError, match="topics rule"):
        hip().scatter_count(1, p(qs.actor), p(qs.a0), 2, 1, p(seg_off), 4, p(sc.n), p(sc.first), p(sc.tsum), p(sc.toob),
                            sc.tile_cap, p(sc.ctr), 0, q_off=p(q_off), n_queues=1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the runtime
def small_case(n_actors=64):
    """Ordinary and queue subscriptions over ``n_actors`` actors (one queue member is nobody)."""
    topics = {0: [[0, 10, 1]], 2: [[1, 5, 3], [5, 1, 1]], 3: [[n_actors - 2, 2, 1]]}
    queues = {0: [[[10, 8, 2]], [[30, 3, 1], [40, 4, 5]]], 1: [[[20, 5, 1]]], 3: [[[n_actors - 1, 2, 1]]],
              5: [[[k % n_actors, 1, 1] for k in range(0, 900, 7)]]}
    g = torch.tensor([0, 5, 3, 1, 2, 9, 6, 8, -1, 3, 4, 0, 1, 5, 0, 3], dtype=torch.int32)
    a0 = torch.arange(3, 3 + g.numel(), dtype=torch.int64) * 1000003
    key = torch.tensor([5, 6, 7, 8, 5, 6, 7, 8, 1, 2, 3, 4, 8, 6, 5, -7], dtype=torch.int64)
    return topics, queues, g, a0, key


def predicted_states(ref, n_actors):
    """The counter actors after a ``METHOD_COUNTER_ADD`` of the reference's rows."""
    st = np.zeros(n_actors, dtype=np.int64)
    actor, a0 = ref["actor"].numpy().astype(np.int64), ref["a0"].numpy()
    ok = actor < n_actors
    np.add.at(st, actor[ok], a0[ok])
    return st.tolist()


def read_states(send, n_actors):
    val, st = send(MsgBatch(torch.arange(n_actors, dtype=torch.int32, device="cuda"),
                            torch.zeros(n_actors, dtype=torch.int64, device="cuda"), None, None, METHOD_COUNTER_ADD))
    assert bool((st == STATUS_OK).all())
    return val.cpu().tolist()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_publish_counter_add_states_and_retries_dead_letters_gpu(delivery):
    rt = gpu_runtime(delivery, actors=64)
    rt_dl, rt_dl_plain = gpu_runtime(delivery, actors=64, dead_letters=True), gpu_runtime(delivery, actors=64, dead_letters=True)
    try:
        topics, queues, g, a0, key = small_case(64)
        pubs = MsgBatch(g, a0, None, None, METHOD_COUNTER_ADD)
        table = T.TopicTable.from_topics("cuda", topics, max_topics=8, queues=queues)
        tt = rt.topics("calculator", table=table)
        sc = S.Scatter.topics(table)
        ref = S.scatter_ref(sc, pubs, key=key)
        ans = rt.publish("calculator", _cuda(pubs), key=key.cuda())
        assert torch.equal(ans.n.cpu(), ref["n"]) and torch.equal(ans.first.cpu(), ref["first"]) and ans.oob == ref["oob"] == 3
        assert ans.count.cpu().tolist() == ref["n"].tolist() == [12, 1, 3, 1, 6, 0, 0, 0, 0, 3, 0, 12, 1, 1, 12, 3]
        missing = ref["actor"] >= 64
        assert torch.equal(ans.st.cpu(), torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32))
        want = predicted_states(ref, 64)
        assert read_states(lambda b: rt.send("calculator", b), 64) == want
        # by index: seq 0, then Q further
        sc.by = "index"
        for seq in (0, pubs.M):
            sc.seq = seq
            r = S.scatter_ref(sc, pubs)
            rt.publish("calculator", _cuda(pubs), by="index")
            want = [x + y for x, y in zip(want, predicted_states(r, 64))]
            assert read_states(lambda b: rt.send("calculator", b), 64) == want and tt.scatter.seq == seq + pubs.M
        q = rt.stats()["queues"]
        per = int((ref["n"].sum() - S.scatter_ref(S.Scatter.topics(T.TopicTable.from_topics("cpu", topics, max_topics=8)), pubs)["n"].sum()))
        assert q == {"queues": 5, "members": 8 + 7 + 5 + 2 + len(range(0, 900, 7)), "segments": 5 + len(range(0, 900, 7)),
                     "rows": 3 * per} and per == 13
        assert set(rt.stats()["topics"]) == {"topics", "segments", "subscribers", "records", "bad_records", "applied_rev",
                                             "publishes", "publications", "rows", "oob"}
        assert rt.stats()["topics"]["subscribers"] == 10 + 6 + 2
        # with retries and dead letters: what a plain Send of the reference's rows does
        rows = MsgBatch(ref["actor"].cuda(), ref["a0"].cuda(), None, None, METHOD_COUNTER_ADD)
        plain = rt_dl_plain.send("calculator", rows, retries=2, dead_letter=True)
        rt_dl.topics("calculator", table=T.TopicTable.from_topics("cuda", topics, max_topics=8, queues=queues))
        ans = rt_dl.publish("calculator", _cuda(pubs), key=key.cuda(), retries=2, dead_letter=True)
        assert torch.equal(ans.val, plain[0]) and torch.equal(ans.st, plain[1])
        gref = G.gather_ref(plain[0], plain[1], ref["group"], pubs.M, "sum")
        for f in FIELDS:
            assert torch.equal(getattr(ans, f).cpu(), gref[f]), f
        got, pl = rt_dl.stats()["dead_letters"], rt_dl_plain.stats()["dead_letters"]
        assert got["appended"] == pl["appended"] == int(missing.sum()) > 0
        la, lb = rt_dl.dead_letters(), rt_dl_plain.dead_letters()
        assert la.n == lb.n > 0 and torch.equal(la.actor.cpu(), lb.actor.cpu()) and torch.equal(la.row.cpu(), lb.row.cpu())
        assert read_states(lambda b: rt_dl.send("calculator", b), 64) == predicted_states(ref, 64)
    finally:
        for r in (rt, rt_dl, rt_dl_plain):
            r.close()


def test_a_prepared_queue_expansion_is_captured_and_replayed():
    rt = gpu_runtime("direct", actors=64)
    try:
        topics, queues, g, a0, key = small_case(64)
        table = T.TopicTable.from_topics("cuda", topics, max_topics=8, queues=queues)
        sc = rt.topics("calculator", table=table).scatter
        pubs = _cuda(MsgBatch(g, a0 % 1000, a0 % 77, None, METHOD_CALC_MULTIPLY))
        key = key.cuda()  # (before the capture: a copy is no part of it)
        eager = rt.publish("calculator", pubs, op="sum", key=key)
        want = {f: getattr(eager, f).clone() for f in FIELDS}
        assert want["count"].cpu().tolist() == [12, 1, 3, 1, 6, 0, 0, 0, 0, 3, 0, 12, 1, 1, 12, 3]
        s = torch.cuda.Stream()
        scratch = torch.zeros(8, device="cuda")
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            scratch.add_(1)
            with pytest.raises(ValueError, match="captured Send: the total of the expansion is read on the host"):
                sc.expand(pubs, key=key)
        exp = sc.expand(pubs, key=key)
        gq = exp.gather("sum")
        out_val = torch.empty(exp.total, dtype=torch.int64, device="cuda")
        out_status = torch.empty(exp.total, dtype=torch.int32, device="cuda")
        sg = SendGraph(rt.exchange, exp.batch, out_val, out_status, gather=gq)
        for _ in range(2):
            gq.value.zero_(), gq.status.fill_(-1)
            sg.replay()
            torch.cuda.synchronize()
            for f in FIELDS:
                assert torch.equal(getattr(gq, f), want[f]), f
            assert torch.equal(out_val, eager.val) and torch.equal(out_status, eager.st)
        rt.exchange._capturing = True  # as inside ActorExchange.capture
        with pytest.raises(ValueError, match="captured Send"):
            rt.publish("calculator", pubs, key=key)
        rt.exchange._capturing = False
    finally:
        rt.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_queue_publish_multirank_fakecomm():
    """Two in-process ranks, each publishes its own batch with its own keys."""
    from ptype_amd.runtime import DeviceRuntime

    R_, n, M = 2, 2000, 1 << 12
    fc = hip().FakeComm(R_)
    topics, queues, g, a0, key = small_case(n)
    results, errors = [None] * R_, []
    start = threading.Barrier(R_)

    def batches(r):
        if r == 0:
            return [(MsgBatch(g, a0 % 1000, a0 % 77, None, METHOD_CALC_MULTIPLY), key, "key", "sum")]
        return [(MsgBatch(g.flip(0), a0 % 999, a0 % 78, None, METHOD_CALC_MULTIPLY), key * 3 + 1, "key", "max"),
                (MsgBatch(g, a0 % 998, a0 % 79, None, METHOD_CALC_MULTIPLY), None, "index", "min")]

    def run(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tab = RegistryTable(2 * n, device="cuda")
                ids = torch.arange(n)
                tab.upsert(actor_keys(ids), (ids % R_).to(torch.int32), (ids // R_).to(torch.int32))
                tab.enable_directory(n, affine_world=R_)
                st = torch.zeros(n // R_, dtype=torch.int64, device="cuda")
                ex = ActorExchange(tab, M, chunks=1, state=st, fake=(fc, r), delivery="direct")
                rt = DeviceRuntime(torch.device("cuda", 0), actors=n // R_, service="calculator", shm=False, max_batch=M)
                rt.rank, rt.world, rt.world0, rt.table, rt._exchange = r, R_, R_, tab, ex
                try:
                    rt.topics("calculator", table=T.TopicTable.from_topics("cuda", topics, max_topics=8, queues=queues))
                    start.wait(timeout=60)
                    out = []
                    todo = batches(r)
                    for i in range(2):  # (the Send is collective: rank 0 joins the second with nothing to publish)
                        if i < len(todo):
                            q, k, by, op = todo[i]
                            ans = rt.publish("calculator", _cuda(q), op=op, key=None if k is None else k.cuda(), by=by)
                        else:
                            nothing = MsgBatch(torch.tensor([7, -3], dtype=torch.int32), a0[:2], a0[:2], None, METHOD_CALC_MULTIPLY)
                            ans = rt.publish("calculator", _cuda(nothing))
                        s.synchronize()
                        out.append({f: getattr(ans, f).cpu().clone() for f in FIELDS + ("val", "st", "first", "n")})
                    results[r] = out
                finally:
                    rt.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))
            start.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R_)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank hung"
    assert not errors, errors
    table = T.TopicTable.from_topics("cpu", topics, max_topics=8, queues=queues)
    for r in range(R_):
        for (q, k, by, op), got in zip(batches(r), results[r]):
            sc = S.Scatter.topics(table, by=by)  # (seq 0: each rank's table scatter used it once at most)
            ref = S.scatter_ref(sc, q, key=k)
            missing = ref["actor"] >= n
            assert torch.equal(got["st"], torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), (r, op)
            assert torch.equal(got["val"][~missing], (ref["a0"] * ref["a1"])[~missing]), (r, op)
            want = G.gather_ref(got["val"], got["st"], ref["group"], q.M, op)
            for f in FIELDS:
                assert torch.equal(got[f], want[f]), (r, op, f)
            assert torch.equal(got["first"], ref["first"]) and torch.equal(got["n"], ref["n"])
    assert results[0][1]["count"].tolist() == [0, 0]


# ---------------------------------------------------------------- Client.Publish through Join
def test_client_queue_subscribe_publish_through_join_gpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    cfg, c = _join(tmp_path, ports, True)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        n = c.runtime.total_actors
        a, b = c.NewClient("calculator", C.ConnConfig()), c.NewClient("calculator", C.ConnConfig())
        a.Subscribe(3, actors=[1, 2, 3], name="all")
        a.Subscribe(3, actors=torch.arange(100, 100 + 2 * 1000, 2), name="pool", queue=True)   # 1000 workers, one segment
        b.Subscribe(3, segments=[[k * 5, 1, 1] for k in range(600, 1624)], name="pool2", queue=True)  # 1024 segments
        b.Subscribe(5, actors=[n - 1, n + 5], name="edge", queue=True)
        want = {3: [("all", [[1, 3, 1]], False), ("pool", [[100, 1000, 2]], True),
                    ("pool2", [[k * 5, 1, 1] for k in range(600, 1624)], True)],
                5: [("edge", [[n - 1, 2, 6]], True)]}
        assert a.Topics(queues=True) == want == b.Topics(queues=True) and a.Topics() == {3: [("all", [[1, 3, 1]])]}
        Q = 300
        gen = torch.Generator().manual_seed(9)
        g = torch.tensor([3, 5, 3, 4, 1024, 3], dtype=torch.int32).repeat(Q // 6)
        add = torch.randint(1, 1 << 40, (Q,), generator=gen)
        key = torch.randint(0, 40, (Q,), generator=gen)  # 40 users
        pubs = MsgBatch(g, add, None, None, METHOD_COUNTER_ADD)
        table = T.TopicTable.from_topics("cpu", {3: [[1, 3, 1]]}, queues={3: [want[3][1][1], want[3][2][1]], 5: [[[n - 1, 2, 6]]]})
        ref = S.scatter_ref(S.Scatter.topics(table), pubs, key=key)
        send = (lambda bt: a.Send(bt))
        before = read_states(send, n)
        ans = b.Publish(_cuda(pubs), key=key.cuda())
        assert torch.equal(ans.n.cpu(), ref["n"]) and ans.count.cpu().tolist()[:6] == [5, 1, 5, 0, 0, 5] and ans.oob == Q // 6
        missing = ref["actor"] >= n
        assert torch.equal(ans.st.cpu(), torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32))
        after = read_states(send, n)
        assert [y - x for x, y in zip(before, after)] == predicted_states(ref, n)
        # one key, one member: the 40 users reach at most 40 workers of each pool
        rows = ref["actor"].numpy()
        assert len(set(rows[(rows >= 100) & (rows < 2100) & (rows % 2 == 0)].tolist())) <= 40
        st = c.Stats()["runtime"]
        assert st["queues"] == {"queues": 3, "members": 1000 + 1024 + 2, "segments": 1 + 1024 + 1,
                                "rows": int(ref["total"]) - 3 * (Q // 2)}
        assert (st["topics"]["topics"], st["topics"]["segments"], st["topics"]["subscribers"], st["topics"]["records"]) == (1, 1, 3, 4)
        a.Unsubscribe(3, name="pool")
        b.Unsubscribe(3, name="pool2")
        assert b.Publish(_cuda(pubs), key=key.cuda()).count.cpu().tolist()[:6] == [3, 1, 3, 0, 0, 3]
        a.Close()
        b.Close()
    finally:
        server.Close()
        c.Close()
