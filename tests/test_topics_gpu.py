"""Pub/sub topics on the GPU: the ``topics`` rule of the scatter kernels
(csrc/hip/scatter.hip) against the numpy reference, by exact equality, and ``publish``
through the runtime, a captured graph, in-process ranks and Join."""
import threading

import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import gather as G
from ptype_amd.ops import hip
from ptype_amd.ops import scatter as S
from ptype_amd.ops import topics as T
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, STATUS_FAILED,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange, SendGraph

from test_coalesce import retry_mix
from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_ledger_gpu import _join
from test_scatter import FIELDS, same_expansion
from test_scatter_gpu import LAYOUTS, QS, TE, TQ, counts

pytestmark = pytest.mark.gpu

CAP, QCAP = 1 << 15, 4096
MAX_ACTOR = (1 << 31) - 2


def cut(n, shape, gen, k):
    """The segment lengths of a topic of ``n`` rows (k: the topic's index, for variety)."""
    if n == 0:
        return []
    if shape == "one" or (shape == "giant1"):
        return [n]
    if shape == "unit":
        return [1] * n
    if shape == "giant500" and n > 2 * TE:
        cuts = torch.sort(torch.randperm(n - 1, generator=gen)[:499] + 1).values.tolist()
        return [b - a for a, b in zip([0] + cuts, cuts + [n])]
    # ragged: ends at every residue mod 4, and at rows TE - 1, TE, TE + 1 of a tile where the topic reaches them
    ends = sorted({e for e in (1, 2, 3, 5, 6, 7, 8, 12, 13, TE - 1, TE, TE + 1, 2 * TE - 1, 2 * TE + 3) if e < n}
                  | {e for e in range(17 + k % 5, n, 61 + k % 7)} | {n})
    return [b - a for a, b in zip([0] + ends[:-1], ends)]


def topics_case(n, shape, gen, oob=False, method_col=False, cols=2, max_topics=None):
    """One topic per publication, in another order; strides 1, 3 and one whose last id is
    exactly 2**31 - 2.  Returns the table (CUDA) and the publications (CPU)."""
    Q = n.numel()
    G_ = max(Q, 1) if max_topics is None else max_topics
    perm = torch.randperm(Q, generator=gen)
    topics = {}
    for q in range(Q):
        segs = []
        for j, c in enumerate(cut(int(n[q]), shape, gen, q)):
            kind = (q + j) % 3
            if kind == 0:
                segs.append([int(torch.randint(0, 1 << 20, (1,), generator=gen)), c, 1])
            elif kind == 1:
                segs.append([int(torch.randint(0, 1 << 20, (1,), generator=gen)), c, 3])
            else:
                stride = MAX_ACTOR // c if c > 1 else 1
                segs.append([MAX_ACTOR - stride * (c - 1), c, stride])  # the last id is exactly 2**31 - 2
        if segs:
            topics[int(perm[q])] = segs
    table = T.TopicTable.from_topics("cuda", topics, max_topics=G_)
    g = perm.to(torch.int32)
    if oob and Q:
        where = torch.rand(Q, generator=gen) < 0.25
        bad = torch.tensor([G_, G_ + 7, -1, -(1 << 31), (1 << 31) - 1])[torch.randint(0, 5, (Q,), generator=gen)]
        g = torch.where(where, bad, g.to(torch.int64)).to(torch.int32)
    col = (lambda: torch.randint(-2**62, 2**62, (Q,), generator=gen))
    m = METHOD_CALC_MULTIPLY
    if method_col:
        m = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO], dtype=torch.int16)[torch.randint(0, 2, (Q,), generator=gen)]
    return table, MsgBatch(g, col(), col() if cols > 1 else None, col() if cols > 2 else None, m)


def check(sc, qs, qs_gpu=None):
    exp = sc.expand(_cuda(qs) if qs_gpu is None else qs_gpu)
    ref = S.scatter_ref(sc, qs)
    assert exp.batch.M == exp.total == exp.group.numel() and exp.first.numel() == exp.n.numel() == qs.M
    same_expansion(exp, ref)
    return exp, ref


def test_constants_match_the_module():
    lim = hip().scatter_limits()
    assert tuple(lim["rules"]) == S.RULES == ("ranges", "members", "topics")
    assert lim["max_segments"] == S.MAX_SEGMENTS == T.MAX_SEGMENTS
    assert hip().scatter_expand_tile() == TE and hip().scatter_question_tile() == TQ


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("shape", ["one", "unit", "ragged", "giant"])
def test_topics_kernels_against_reference(shape, kind):
    gen = torch.Generator().manual_seed(700 + LAYOUTS.index(kind))
    shapes = ["giant1", "giant500"] if shape == "giant" else [shape]
    sc = None
    for sh in shapes:
        for i, Q in enumerate(QS):
            n = counts(kind, Q, gen)
            table, qs = topics_case(n, sh, gen, oob=i % 2 == 0, method_col=i % 2 == 1, cols=1 + i % 3)
            if sc is None:
                sc = S.Scatter.topics(table, capacity=CAP, q_capacity=QCAP)
            else:
                sc.set_table(table)
            exp, ref = check(sc, qs)
            if i % 2 == 1:
                assert ref["n"].tolist() == n.tolist() and exp.oob == 0
            if ref["total"]:
                assert int(ref["actor"].max()) <= MAX_ACTOR and int(ref["actor"].min()) >= 0
    if kind in ("edges", "giant"):
        assert int(ref["actor"].max()) == MAX_ACTOR  # the large stride's last id was reached


def test_out_of_range_topics_and_empty_topics():
    gen = torch.Generator().manual_seed(71)
    table = T.TopicTable.from_topics("cuda", {0: [[5, 3, 2]], 2: [[0, 1, 1], [9, 2, 4]], 7: [[1, 70, 1]]}, max_topics=8)
    sc = S.Scatter.topics(table, capacity=CAP, q_capacity=QCAP)
    g = torch.tensor([8, -1, -(1 << 31), (1 << 31) - 1, 0, 1, 2, 7, 3, 15, 2], dtype=torch.int32)
    qs = MsgBatch(g, torch.randint(-9, 9, (g.numel(),), generator=gen), None, None, METHOD_ECHO)
    exp, ref = check(sc, qs)
    assert exp.oob == 5 and exp.n.cpu().tolist() == [0, 0, 0, 0, 3, 0, 3, 70, 0, 0, 3]
    assert exp.batch.actor.cpu().tolist()[:6] == [5, 7, 9, 0, 9, 13]
    # a table without a subscriber: nothing is launched past the count
    sc.set_table(T.TopicTable("cuda", max_topics=8))
    exp, ref = check(sc, qs)
    assert exp.total == 0 and exp.oob == 5


def test_unaligned_publication_views_and_method_column():
    gen = torch.Generator().manual_seed(72)
    Q = TQ + 66
    table, qs = topics_case(counts("giant", Q, gen), "ragged", gen, oob=True, method_col=True, cols=3)
    off1 = (lambda t: torch.cat([t[:1], t]).cuda()[1:])
    qg = MsgBatch(off1(qs.actor), off1(qs.a0), off1(qs.a1), off1(qs.a2), off1(qs.method))
    assert qg.actor.data_ptr() % 16 == 4 and qg.a0.data_ptr() % 16 == 8 and qg.method.data_ptr() % 16 == 2
    sc = S.Scatter.topics(table, capacity=CAP, q_capacity=QCAP)
    exp, ref = check(sc, qs, qg)
    assert exp.batch.method.dtype == torch.int16 and exp.oob > 0


def test_repeated_expand_and_a_table_replaced_between_expands():
    gen = torch.Generator().manual_seed(73)
    sc = None
    for Q, kind, shape in ((3 * TQ + 17, "giant", "giant500"), (65, "random", "unit"), (1, "ones", "one"),
                           (5, "zeros", "one"), (0, "ones", "one"), (TQ + 1, "edges", "ragged"),
                           (3 * TQ + 17, "random", "ragged")):
        table, qs = topics_case(counts(kind, Q, gen), shape, gen, cols=2)
        if sc is None:
            sc = S.Scatter.topics(table, capacity=CAP, q_capacity=QCAP)
        sc.set_table(table)  # the table of the previous expand is gone: every expand reads the current one
        exp, ref = check(sc, qs)
        assert exp.batch.a0.numel() == ref["total"] and exp.group.numel() == ref["total"]
    # one TopicTable whose arrays are replaced in place (what a follower's apply does)
    table.load(T.TopicTable.from_topics("cuda", {0: [[3, 4, 5]]}, max_topics=table.max_topics).host)
    qs = MsgBatch(torch.tensor([0, 1, 0], dtype=torch.int32), torch.tensor([1, 2, 3]), None, None, METHOD_ECHO)
    exp, ref = check(sc, qs)
    assert exp.batch.actor.cpu().tolist() == [3, 8, 13, 18] * 2 and exp.n.cpu().tolist() == [4, 0, 4]


def test_capacity_is_exact_and_the_total_is_refused_before_a_row_is_written():
    cap = TE + 5
    table = T.TopicTable.from_topics("cuda", {0: [[0, TE, 1]], 1: [[7, 2, 3], [1, 3, 1]], 2: [[0, 6, 1]]}, max_topics=4)
    sc = S.Scatter.topics(table, capacity=cap, q_capacity=8)
    mk = (lambda g: MsgBatch(torch.tensor(g, dtype=torch.int32), torch.arange(len(g), dtype=torch.int64), None, None,
                             METHOD_ECHO))
    exp, ref = check(sc, mk([0, 3, 1]))
    assert exp.total == cap
    with pytest.raises(ValueError, match=f"{cap + 1} rows, the capacity is {cap}"):
        sc.expand(_cuda(mk([0, 2])))
    with pytest.raises(ValueError, match="q_capacity"):
        sc.expand(_cuda(mk([3] * 9)))
    torch.cuda.synchronize()
    for name in ("actor", "a0", "group"):  # the buffers still hold the previous expansion
        assert torch.equal(getattr(sc, name).cpu(), ref[name]), name


def test_launchers_validate_the_table():
    table = T.TopicTable.from_topics("cuda", {0: [[0, 4, 1]]}, max_topics=4)
    sc = S.Scatter.topics(table, capacity=64, q_capacity=8)
    qs = _cuda(MsgBatch(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), None, None, METHOD_ECHO))
    sc.expand(qs)
    seg_off, row_off, seg_start, seg_stride = table.device_arrays()
    p = (lambda t: t.data_ptr())
    count = (lambda **kw: hip().scatter_count(2, p(qs.actor), p(qs.a0), 2, 1, p(seg_off), 4, p(sc.n), p(sc.first),
                                              p(sc.tsum), p(sc.toob), sc.tile_cap, p(sc.ctr), 0, **kw))
    with pytest.raises(ValueError, match="row_off"):
        count()
    with pytest.raises(ValueError, match="row_off"):
        count(row_off=p(row_off) + 4, n_segs=1)
    with pytest.raises(ValueError, match="n_segs"):
        count(row_off=p(row_off), n_segs=(1 << 24) + 1)
    expand = (lambda **kw: hip().scatter_expand(2, p(qs.actor), p(qs.a0), 0, 0, 0, 2, 1, 1, 0, False, 0, p(seg_off), 0, 4, 0,
                                                p(sc.first), p(sc.n), 8, 64, p(sc.actor), p(sc.a0), 0, 0, 0, p(sc.group),
                                                0, **kw))
    with pytest.raises(ValueError, match="segment table"):
        expand(row_off=p(row_off), n_segs=1)
    with pytest.raises(ValueError, match="segment table"):
        expand(row_off=p(row_off), seg_start=p(seg_start), seg_stride=p(seg_stride), n_segs=0)
    with pytest.raises(ValueError, match="misaligned"):
        expand(row_off=p(row_off), seg_start=p(seg_start) + 2, seg_stride=p(seg_stride), n_segs=1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- capture
def test_expand_is_refused_under_capture_and_a_prepared_expansion_is_captured():
    rt = gpu_runtime("direct", actors=64)
    try:
        table = T.TopicTable.from_topics("cuda", {0: [[0, 64, 1]], 1: [[1, 20, 3], [5, 1, 1]], 3: [[2, 7, 9]]}, max_topics=4)
        tt = rt.topics("calculator", table=table)
        sc = tt.scatter
        pubs = _cuda(MsgBatch(torch.tensor([1, 0, 2, 3, 1], dtype=torch.int32), torch.arange(2, 7, dtype=torch.int64),
                              torch.arange(5, dtype=torch.int64) - 2, None, METHOD_CALC_MULTIPLY))
        eager = rt.publish("calculator", pubs, op="sum")
        want = {f: getattr(eager, f).clone() for f in FIELDS}
        assert want["count"].cpu().tolist() == [21, 64, 0, 7, 21]
        s = torch.cuda.Stream()
        scratch = torch.zeros(8, device="cuda")
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            scratch.add_(1)
            with pytest.raises(ValueError, match="captured Send: the total of the expansion is read on the host"):
                sc.expand(pubs)
        exp = sc.expand(pubs)
        g = exp.gather("sum")
        out_val = torch.empty(exp.total, dtype=torch.int64, device="cuda")
        out_status = torch.empty(exp.total, dtype=torch.int32, device="cuda")
        sg = SendGraph(rt.exchange, exp.batch, out_val, out_status, gather=g)
        for _ in range(2):
            g.value.zero_(), g.status.fill_(-1)
            sg.replay()
            torch.cuda.synchronize()
            for f in FIELDS:
                assert torch.equal(getattr(g, f), want[f]), f
            assert torch.equal(out_val, eager.val) and torch.equal(out_status, eager.st)
        rt.exchange._capturing = True  # as inside ActorExchange.capture
        with pytest.raises(ValueError, match="captured Send"):
            rt.publish("calculator", pubs)
        rt.exchange._capturing = False
    finally:
        rt.close()


# ---------------------------------------------------------------- runtime.publish at world 1
def publish_case(n_actors):
    """Topics over Calculator actors (one names an unregistered actor, two name actor 5) and
    the publications."""
    topics = {0: [[0, n_actors, 1]], 2: [[1, 20, 3], [5, 1, 1], [5, 3, 2]], 3: [[n_actors - 3, 4, 1]],
              5: [[k % n_actors, 1, 1] for k in range(2100)], 6: [[0, 300, 1]]}
    g = torch.tensor([5, 0, 3, 1, 2, 9, 6, 8, -1, 3, 4, 0], dtype=torch.int32)
    a0 = torch.arange(3, 3 + g.numel(), dtype=torch.int64)
    a1 = torch.arange(-5, -5 + g.numel(), dtype=torch.int64)
    return topics, MsgBatch(g, a0, a1, None, METHOD_CALC_MULTIPLY)


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_publish_equals_a_plain_send_of_the_reference_rows_gpu(delivery):
    rt, rt_plain = gpu_runtime(delivery, actors=64), gpu_runtime(delivery, actors=64)
    try:
        topics, pubs = publish_case(rt.total_actors)
        topics[6] = [[0, 60, 1]]
        table = T.TopicTable.from_topics("cuda", topics, max_topics=8)
        rt.topics("calculator", table=table)
        ref = S.scatter_ref(S.Scatter.topics(table), pubs)
        plain = rt_plain.send("calculator", MsgBatch(ref["actor"].cuda(), ref["a0"].cuda(), ref["a1"].cuda(), None,
                                                     METHOD_CALC_MULTIPLY))
        for op in ("sum", "max"):
            ans = rt.publish("calculator", _cuda(pubs), op=op)
            assert torch.equal(ans.val, plain[0]) and torch.equal(ans.st, plain[1])
            want = G.gather_ref(plain[0], plain[1], ref["group"], pubs.M, op)
            for f in FIELDS:
                assert torch.equal(getattr(ans, f).cpu(), want[f]), (op, f)
            assert torch.equal(ans.first.cpu(), ref["first"]) and torch.equal(ans.n.cpu(), ref["n"]) and ans.oob == 3
        assert int((ans.status == STATUS_NO_ACTOR).sum()) == 2  # topic 3 reaches one id past the actors
        assert ans.count.cpu().tolist()[4] == 24 and ans.n_ok.cpu().tolist()[4] == 24  # actor 5 twice: no de-duplication
        st = rt.stats()["topics"]
        assert (st["publishes"], st["publications"], st["rows"], st["oob"]) == (2, 2 * pubs.M, 2 * ref["total"], 6)
        assert (st["topics"], st["segments"], st["subscribers"]) == (5, 2106, int(table.host["row_off"][-1]))
        # the Send's wrappers apply to the expanded calls
        for kw in ({"coalesce": True, "cache": True, "retries": 2}, {"coalesce": True}):
            again = rt.publish("calculator", _cuda(pubs), op="max", **kw)
            assert torch.equal(again.val, plain[0]) and torch.equal(again.st, plain[1])
            for f in FIELDS:
                assert torch.equal(getattr(again, f).cpu(), want[f]), (kw, f)
    finally:
        rt.close()
        rt_plain.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_publish_with_retries_and_dead_letters_over_a_retry_mix_gpu(delivery):
    """Every publication is one row of ``retry_mix`` (a topic of one subscriber), so the
    Publish's per-call replies are the retried Send's."""
    b, where = retry_mix()
    topics = {q: [[int(b.actor[q]), 1, 1]] for q in range(b.M)}
    pubs = MsgBatch(torch.arange(b.M, dtype=torch.int32), b.a0, b.a1, None, b.method)
    rt, rt_plain = gpu_runtime(delivery), gpu_runtime(delivery)
    rt_dl, rt_dl_plain = gpu_runtime(delivery, dead_letters=True), gpu_runtime(delivery, dead_letters=True)
    try:
        table = T.TopicTable.from_topics("cuda", topics, max_topics=1024)
        want = rt_plain.send("calculator", _cuda(b), retries=2)
        rt.topics("calculator", table=table)
        ans = rt.publish("calculator", _cuda(pubs), op="max", retries=2, coalesce=True)
        assert torch.equal(ans.val, want[0]) and torch.equal(ans.st, want[1])
        assert int((ans.st.cpu()[where] == STATUS_FAILED).sum()) == 16
        ref = G.gather_ref(want[0], want[1], torch.arange(b.M, dtype=torch.int32), b.M, "max")
        for f in FIELDS:
            assert torch.equal(getattr(ans, f).cpu(), ref[f]), f
        # dead letters: the failed deliveries are filed as a plain Send's are
        want = rt_dl_plain.send("calculator", _cuda(b), dead_letter=True)
        rt_dl.topics("calculator", table=T.TopicTable.from_topics("cuda", topics, max_topics=1024))
        ans = rt_dl.publish("calculator", _cuda(pubs), op="sum", dead_letter=True)
        assert torch.equal(ans.val, want[0]) and torch.equal(ans.st, want[1])
        got, plain = rt_dl.stats()["dead_letters"], rt_dl_plain.stats()["dead_letters"]
        assert got["appended"] == plain["appended"] == int((want[1] != STATUS_OK).sum()) > 0
        la, lb = rt_dl.dead_letters(), rt_dl_plain.dead_letters()
        assert la.n == lb.n > 0 and torch.equal(la.actor.cpu(), lb.actor.cpu()) and torch.equal(la.row.cpu(), lb.row.cpu())
        assert torch.equal(la.status.cpu(), lb.status.cpu())
    finally:
        for r in (rt, rt_plain, rt_dl, rt_dl_plain):
            r.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_publish_multirank_fakecomm():
    """Two in-process ranks, each publishes its own batch; rank 1's second Publish expands
    into nothing and joins the collective Send with an empty batch."""
    from ptype_amd.runtime import DeviceRuntime

    R_, n, M = 2, 6000, 1 << 13
    fc = hip().FakeComm(R_)
    topics, pubs = publish_case(n)
    topics[0] = [[0, 2000, 3]]
    results, inner, errors = [None] * R_, [None] * R_, []
    start = threading.Barrier(R_)

    def batches(r):
        if r == 0:
            return [(pubs, "sum"), (MsgBatch(pubs.actor.flip(0), pubs.a0, pubs.a1, None, METHOD_CALC_MULTIPLY), "min")]
        nothing = MsgBatch(torch.tensor([1, 7, -3, 40], dtype=torch.int32), pubs.a0[:4], pubs.a1[:4], None,
                           METHOD_CALC_MULTIPLY)
        return [(MsgBatch(pubs.actor, pubs.a1, pubs.a0 * 3, None, METHOD_CALC_MULTIPLY), "max"), (nothing, "sum")]

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
                calls = []
                inner_send = rt._send

                def counted(service, sub, *a, **kw):
                    calls.append(sub.M)
                    return inner_send(service, sub, *a, **kw)

                rt._send = counted
                try:
                    rt.topics("calculator", table=T.TopicTable.from_topics("cuda", topics, max_topics=8))
                    start.wait(timeout=60)
                    out = []
                    for q, op in batches(r):
                        ans = rt.publish("calculator", _cuda(q), op=op)
                        s.synchronize()
                        out.append({f: getattr(ans, f).cpu().clone() for f in FIELDS + ("val", "st", "first", "n")})
                    results[r], inner[r] = out, calls
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
    sc = S.Scatter.topics(T.TopicTable.from_topics("cpu", topics, max_topics=8))
    for r in range(R_):
        for (q, op), got in zip(batches(r), results[r]):
            ref = S.scatter_ref(sc, q)
            missing = ref["actor"] >= n
            assert torch.equal(got["st"], torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), (r, op)
            assert torch.equal(got["val"][~missing], (ref["a0"] * ref["a1"])[~missing]), (r, op)
            want = G.gather_ref(got["val"], got["st"], ref["group"], q.M, op)
            for f in FIELDS:
                assert torch.equal(got[f], want[f]), (r, op, f)
            assert torch.equal(got["first"], ref["first"]) and torch.equal(got["n"], ref["n"])
    assert inner[1][1] == 0 and inner[0][1] > 0 and results[1][1]["count"].tolist() == [0] * 4


# ---------------------------------------------------------------- Client.Publish through Join
def test_client_subscribe_publish_unsubscribe_through_join_gpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    cfg, c = _join(tmp_path, ports, True)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        n = c.runtime.total_actors
        zero = {"topics": 0, "segments": 0, "subscribers": 0, "records": 0, "bad_records": 0, "applied_rev": 0,
                "publishes": 0, "publications": 0, "rows": 0, "oob": 0}
        assert c.Stats()["runtime"]["topics"] == zero and not c.runtime._topics  # nothing is watched yet
        a, b = c.NewClient("calculator", C.ConnConfig()), c.NewClient("calculator", C.ConnConfig())
        x = torch.arange(n, dtype=torch.int64, device="cuda") - 100
        every = MsgBatch(torch.arange(n, dtype=torch.int32, device="cuda"), x, x + 7, None, METHOD_CALC_MULTIPLY)
        r1 = a.Subscribe(3, actors=torch.arange(1, n, 2))          # one strided segment
        r2 = b.Subscribe(3, segments=[[5, 3, 1], [5, 1, 1]], name="again")
        r3 = b.Subscribe(900, actors=[0, 1, 2, 3, 10, 4000, n + 5], name="mixed")
        assert r1 < r2 < r3
        want = {3: [("again", [[5, 3, 1], [5, 1, 1]]), ("gpu0", [[1, n // 2, 2]])],
                900: [("mixed", [[0, 4, 1], [10, 2, 3990], [n + 5, 1, 1]])]}
        assert a.Topics() == want and b.Topics() == want
        val, st = a.Send(every)  # the registry's own Sends in between are unaffected
        assert torch.equal(val, x * (x + 7)) and bool((st == STATUS_OK).all())
        pubs = MsgBatch(torch.tensor([3, 900, 4, 1024, 3], dtype=torch.int32), torch.tensor([2, 3, 4, 5, -6]),
                        torch.tensor([7, 7, 7, 7, 7]), None, METHOD_CALC_MULTIPLY)
        sc = S.Scatter.topics(T.TopicTable.from_topics("cpu", {g: sum((s for _, s in subs), []) for g, subs in want.items()}))
        ref = S.scatter_ref(sc, pubs)
        plain = a.Send(MsgBatch(ref["actor"].cuda(), ref["a0"].cuda(), ref["a1"].cuda(), None, METHOD_CALC_MULTIPLY))
        for op in ("sum", "min"):
            ans = b.Publish(_cuda(pubs), op=op)
            assert torch.equal(ans.val, plain[0]) and torch.equal(ans.st, plain[1])
            g = G.gather_ref(plain[0], plain[1], ref["group"], pubs.M, op)
            for f in FIELDS:
                assert torch.equal(getattr(ans, f).cpu(), g[f]), (op, f)
        assert ans.count.cpu().tolist() == [n // 2 + 4, 7, 0, 0, n // 2 + 4] and ans.oob == 1
        assert ans.n_ok.cpu().tolist() == [n // 2 + 4, 6, 0, 0, n // 2 + 4]  # actor n + 5 is nobody
        val, st = a.Send(every)
        assert torch.equal(val, x * (x + 7)) and bool((st == STATUS_OK).all())
        st = c.Stats()["runtime"]["topics"]
        assert st == {"topics": 2, "segments": 6, "subscribers": n // 2 + 4 + 7, "records": 3, "bad_records": 0,
                      "applied_rev": r3, "publishes": 2, "publications": 10, "rows": 2 * ref["total"], "oob": 2}
        r4 = a.Unsubscribe(3)
        r5 = b.Unsubscribe(3, name="again")
        assert r3 < r4 < r5 and set(a.Topics()) == {900}
        ans = a.Publish(_cuda(pubs))
        assert ans.count.cpu().tolist() == [0, 7, 0, 0, 0] and ans.oob == 1
        a.Close()
        b.Close()
    finally:
        server.Close()
        c.Close()
