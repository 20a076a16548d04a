"""Call scatter on the GPU: the kernels (csrc/hip/scatter.hip) against the numpy
reference, by exact equality, and ``ask`` through the runtime, a captured graph, in-process
ranks and Join."""
import threading

import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.models import optimus
from ptype_amd.ops import gather as G
from ptype_amd.ops import hip
from ptype_amd.ops import scatter as S
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK, STATUS_FAILED,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange, SendGraph

from test_coalesce import retry_mix
from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_ledger_gpu import _join
from test_scatter import FIELDS, same_expansion
from test_send_retries import retry_scenario

pytestmark = pytest.mark.gpu

TQ = 1024  # questions per tile of the count pass (checked below against the module)
TE = 2048  # output rows per tile of the expand pass
QS = [0, 1, 63, 64, 65, TQ - 1, TQ, TQ + 1, 3 * TQ + 17]
LAYOUTS = ["ones", "zeros", "random", "edges", "giant"]
CAP, QCAP = 1 << 15, 4096


def constants():
    assert hip().scatter_question_tile() == TQ == S.QUESTION_TILE and hip().scatter_expand_tile() == TE == S.TILE
    lim = hip().scatter_limits()
    assert lim["max_rows"] == S.MAX_ROWS and lim["max_questions"] == S.MAX_QUESTIONS and lim["max_step"] == S.MAX_STEP
    assert tuple(lim["rules"]) == S.RULES and lim["ctr_words"] == 2


def counts(kind, Q, gen):
    """Rows per question."""
    if kind == "ones":
        return torch.ones(Q, dtype=torch.int64)
    if kind == "zeros":
        return torch.zeros(Q, dtype=torch.int64)
    small = torch.tensor([0, 0, 0, 1, 2, 5])[torch.randint(0, 6, (Q,), generator=gen)]
    if kind == "random":
        return small
    if kind == "edges":  # runs that end exactly at TE - 1, TE, TE + 1 and at 2 * TE; then a head at every row
        n = torch.cat([torch.tensor([TE - 1, 1, 1, TE - 1]), torch.ones(Q, dtype=torch.int64)])[:Q]
        if Q > 8:
            n[6] = 0
        return n
    # giant: one question of 3 * TE + 7 rows between one-row and zero-row neighbours; a run of
    # zero-row questions longer than a block's stride further on
    n = small.clone()
    if Q == 0:
        return n
    at = Q // 2
    n[at] = 3 * TE + 7
    for d, v in ((-2, 0), (-1, 1), (1, 0), (2, 0), (3, 1)):
        if 0 <= at + d < Q:
            n[at + d] = v
    if Q >= TQ:
        n[at + 10:at + 400] = 0
    return n


def ranges_case(n, step, gen):
    """Targets whose question q has n[q] ranges: n * step - r with r in [0, step); none: t <= 0."""
    r = torch.randint(0, step, (n.numel(),), generator=gen)
    t = torch.where(n > 0, n * step - r, -torch.randint(0, 3, (n.numel(),), generator=gen) * 1000)
    return MsgBatch(torch.zeros(n.numel(), dtype=torch.int32), t, None, None, METHOD_PRIME_CHECK)


def members_case(n, gen, oob=False, method_col=False, cols=2):
    """A CSR with one group per question, in another order, and the questions that name them."""
    Q = n.numel()
    perm = torch.randperm(Q, generator=gen)  # question q names group perm[q]
    sizes = torch.zeros(Q, dtype=torch.int64)
    sizes[perm] = n
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    members = torch.randint(0, 1 << 20, (int(sizes.sum()),), generator=gen).to(torch.int32)
    g = perm.to(torch.int32)
    if oob and Q:
        where = torch.rand(Q, generator=gen) < 0.25
        bad = torch.tensor([Q, Q + 7, -1, -(1 << 31), (1 << 31) - 1])[torch.randint(0, 5, (Q,), generator=gen)]
        g = torch.where(where, bad, g.to(torch.int64)).to(torch.int32)
    col = (lambda: torch.randint(-2**62, 2**62, (Q,), generator=gen))
    m = METHOD_CALC_MULTIPLY
    if method_col:
        m = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO], dtype=torch.int16)[torch.randint(0, 2, (Q,), generator=gen)]
    return offsets, members, MsgBatch(g, col(), col() if cols > 1 else None, col() if cols > 2 else None, m)


def check(sc, qs, qs_gpu=None):
    """expand on the GPU equals scatter_ref, field for field."""
    exp = sc.expand(_cuda(qs) if qs_gpu is None else qs_gpu)
    ref = S.scatter_ref(sc, qs)
    assert exp.batch.M == exp.total == exp.group.numel() and exp.first.numel() == exp.n.numel() == qs.M
    assert exp.batch.actor.is_cuda and (exp.total == 0 or exp.batch.actor.data_ptr() == sc.actor.data_ptr())
    same_expansion(exp, ref)
    return exp, ref


def test_constants_match_the_module():
    constants()


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("step,first_lo", [(10, 2), (1, None), ((1 << 31) - 1, -5)])
def test_ranges_kernels_against_reference(step, first_lo, kind):
    constants()
    gen = torch.Generator().manual_seed(200 + LAYOUTS.index(kind))
    sc = S.Scatter.ranges(step, 1000 if step == 10 else 3, first_lo=first_lo, actor_base=5, capacity=CAP, q_capacity=QCAP)
    for Q in QS:
        n = counts(kind, Q, gen)
        exp, ref = check(sc, ranges_case(n, step, gen))
        assert ref["n"].tolist() == n.tolist()


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("oob", [False, True])
def test_members_kernels_against_reference(oob, kind):
    constants()
    gen = torch.Generator().manual_seed(300 + LAYOUTS.index(kind))
    sc = None
    for i, Q in enumerate(QS):
        offsets, members, qs = members_case(counts(kind, Q, gen), gen, oob=oob, method_col=i % 2 == 1, cols=1 + i % 3)
        if sc is None:
            sc = S.Scatter.members(offsets.cuda(), members.cuda(), capacity=CAP, q_capacity=QCAP)
        else:
            sc.set_members(offsets.cuda(), members.cuda())
        exp, ref = check(sc, qs)
        assert exp.oob == 0 if not oob else (exp.oob > 0 or Q < 63)


def test_total_past_int32_is_refused_before_a_row_is_written():
    """Counts that do not fit int32, and a total that saturates: the host read refuses them."""
    sc = S.Scatter.ranges(1, 4, capacity=64)
    exp, _ = check(sc, MsgBatch(torch.zeros(2, dtype=torch.int32), torch.tensor([30, 34]), None, None, METHOD_ECHO))
    before = (sc.actor.clone(), sc.a0.clone(), sc.a1.clone(), sc.a2.clone(), sc.group.clone())
    big = (1 << 63) - 1
    for t, total in (([big, 5, 1 << 40], big + 5 + (1 << 40)), ([big] * 3, (1 << 64) - 1), ([60, 5], 65)):
        qs = MsgBatch(torch.zeros(len(t), dtype=torch.int32).cuda(), torch.tensor(t).cuda(), None, None, METHOD_ECHO)
        with pytest.raises(ValueError, match=f"{total} rows, the capacity is 64"):
            sc.expand(qs)
    torch.cuda.synchronize()
    for got, want in zip((sc.actor, sc.a0, sc.a1, sc.a2, sc.group), before):
        assert torch.equal(got, want)


# ---------------------------------------------------------------- buffer handling
def test_repeated_expand_shrinking_and_growing():
    constants()
    gen = torch.Generator().manual_seed(31)
    sc = S.Scatter.ranges(10, 77, first_lo=2, capacity=CAP, q_capacity=QCAP)
    for Q, kind in ((3 * TQ + 17, "giant"), (65, "random"), (1, "ones"), (5, "zeros"), (0, "ones"), (TQ + 1, "edges"),
                    (3 * TQ + 17, "random")):
        exp, ref = check(sc, ranges_case(counts(kind, Q, gen), 10, gen))
        assert exp.batch.a0.numel() == ref["total"] and exp.group.numel() == ref["total"]  # no stale row is exposed


def test_unaligned_question_views_and_method_column():
    constants()
    gen = torch.Generator().manual_seed(32)
    Q = TQ + 66
    # ranges: a0 (and a method column) as views at an odd element offset
    qs = ranges_case(counts("random", Q, gen), 10, gen)
    qs.method = torch.randint(0, 9, (Q,), generator=gen).to(torch.int16)
    a0, m = torch.cat([qs.a0[:1], qs.a0]).cuda()[1:], torch.cat([qs.method[:1], qs.method]).cuda()[1:]
    assert a0.data_ptr() % 16 == 8 and m.data_ptr() % 4 == 2
    sc = S.Scatter.ranges(10, 9, capacity=CAP, q_capacity=QCAP)
    check(sc, qs, MsgBatch(qs.actor.cuda(), a0, None, None, m))
    # members: every column off by one element, an int16 method column
    offsets, members, qs = members_case(counts("giant", Q, gen), gen, oob=True, method_col=True, cols=3)
    off1 = (lambda t: torch.cat([t[:1], t]).cuda()[1:])
    qg = MsgBatch(off1(qs.actor), off1(qs.a0), off1(qs.a1), off1(qs.a2), off1(qs.method))
    assert qg.actor.data_ptr() % 16 == 4 and qg.a0.data_ptr() % 16 == 8 and qg.method.data_ptr() % 16 == 2
    sc = S.Scatter.members(offsets.cuda(), members.cuda(), capacity=CAP, q_capacity=QCAP)
    exp, ref = check(sc, qs, qg)
    assert exp.batch.method.dtype == torch.int16 and exp.oob > 0


def test_capacity_is_exact():
    constants()
    cap = TE + 5
    sc = S.Scatter.ranges(10, 7, first_lo=2, capacity=cap, q_capacity=8)
    full = MsgBatch(torch.zeros(3, dtype=torch.int32), torch.tensor([10 * TE, 0, 41]), None, None, METHOD_PRIME_CHECK)
    exp, ref = check(sc, full)
    assert exp.total == cap
    over = MsgBatch(full.actor, torch.tensor([10 * TE, 1, 41]), None, None, METHOD_PRIME_CHECK)
    with pytest.raises(ValueError, match=f"{cap + 1} rows, the capacity is {cap}"):
        sc.expand(_cuda(over))
    with pytest.raises(ValueError, match="q_capacity"):
        sc.expand(_cuda(ranges_case(torch.ones(9, dtype=torch.int64), 10, torch.Generator().manual_seed(1))))
    torch.cuda.synchronize()
    for name in ("actor", "a0", "a1", "a2", "group"):  # the buffers still hold the previous expansion
        assert torch.equal(getattr(sc, name).cpu(), ref[name]), name


# ---------------------------------------------------------------- capture
def test_expand_is_refused_under_capture_and_a_prepared_expansion_is_captured():
    constants()
    rt = gpu_runtime("direct", actors=64)
    try:
        rt.host(optimus.SERVICE)
        gen = torch.Generator().manual_seed(41)
        targets = torch.cat([torch.tensor([2, 3, 4, 91, 97, 7919, 7921]), torch.randint(2, 400, (150,), generator=gen)])
        qs = MsgBatch(torch.zeros(targets.numel(), dtype=torch.int32).cuda(), targets.cuda(), None, None,
                      METHOD_PRIME_CHECK)
        sc = S.Scatter.ranges(10, rt.total_actors, first_lo=2, capacity=rt.max_batch)
        eager = rt.ask(optimus.SERVICE, qs, sc, op="first_ne", sentinel=qs.a0)
        want = {f: getattr(eager, f).clone() for f in FIELDS}
        assert want["value"].cpu().tolist()[:7] == [2, 3, 2, 7, 97, 7919, 89]
        # expand under capture: the documented error, before anything is launched
        s = torch.cuda.Stream()
        scratch = torch.zeros(8, device="cuda")
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            scratch.add_(1)
            with pytest.raises(ValueError, match="captured Send: the total of the expansion is read on the host"):
                sc.expand(qs)
        # the prepared expansion through the existing captured Send
        exp = sc.expand(qs)
        g = exp.gather("first_ne", qs.a0)
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
            rt.ask(optimus.SERVICE, qs, sc, op="first_ne", sentinel=qs.a0)
        rt.exchange._capturing = False
    finally:
        rt.close()


# ---------------------------------------------------------------- runtime.ask at world 1
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_ask_ranges_prime_check_gpu(delivery):
    gen = torch.Generator().manual_seed(51)
    targets = torch.cat([torch.tensor([2, 3, 4, 5, 9, 97, 121, 1009, 1024, 0, -4]),
                         torch.randint(2, 500, (189,), generator=gen)])
    rt = gpu_runtime(delivery, actors=64)
    try:
        rt.host(optimus.SERVICE)
        qs = MsgBatch(torch.zeros(targets.numel(), dtype=torch.int32).cuda(), targets.cuda(), None, None,
                      METHOD_PRIME_CHECK)
        sc = S.Scatter.ranges(10, rt.total_actors, first_lo=2, capacity=rt.max_batch)
        for _ in range(2):
            ans = rt.ask(optimus.SERVICE, qs, sc, op="first_ne", sentinel=qs.a0)
            f = optimus.FanOut(targets.clamp(min=0), rt.total_actors, "cpu")  # (its n: (t + 9) // 10)
            want, status = optimus.gather_ref(ans.val.cpu(), ans.st.cpu(), f.first, f.n, targets)
            assert torch.equal(ans.value.cpu(), want) and torch.equal(ans.status.cpu(), status)
            assert torch.equal(ans.first.cpu(), f.first) and torch.equal(ans.n.cpu().to(torch.int64), f.n)
            assert bool((ans.status == STATUS_OK).all()) and ans.val.numel() == f.M and ans.oob == 0
        divisors = [next((d for d in range(2, t) if t % d == 0), t) for t in targets.tolist()]
        assert ans.value.cpu().tolist() == divisors
        # ask_device: the same answers without a FanOut
        a2, s2 = optimus.ask_device(rt, targets)
        assert a2.cpu().tolist() == divisors and bool((s2 == STATUS_OK).all())
        assert rt.stats()["scatter"] == {"asks": 3, "questions": 3 * targets.numel(), "rows": 3 * f.M, "oob": 0}
    finally:
        rt.close()


def broadcast_case(n_actors):
    """Groups of Calculator actors (one with an unregistered member) and the questions."""
    sizes = torch.tensor([5, 0, 64, 1, 300, 17, 0, 2100])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    members = (torch.arange(int(sizes.sum())) * 7 % n_actors).to(torch.int32)
    bad_at = int(offsets[4]) + 123
    members[bad_at] = n_actors + 9  # group 4, its row 123: nobody
    g = torch.tensor([7, 0, 4, 1, 3, 9, 2, 5, -1, 4, 6, 0], dtype=torch.int32)
    a0 = torch.arange(3, 3 + g.numel(), dtype=torch.int64)
    a1 = torch.arange(-5, -5 + g.numel(), dtype=torch.int64)
    return sizes, offsets, members, MsgBatch(g, a0, a1, None, METHOD_CALC_MULTIPLY)


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_ask_members_multiply_sum_gpu(delivery):
    rt, rt_led = gpu_runtime(delivery, actors=64), gpu_runtime(delivery, actors=64, ledger=True)
    try:
        sizes, offsets, members, qs = broadcast_case(rt.total_actors)
        sc = S.Scatter.members(offsets.cuda(), members.cuda(), capacity=rt.max_batch)
        g = qs.actor.to(torch.int64)
        inside = (g >= 0) & (g < sizes.numel())
        n = torch.where(inside, sizes[g.clamp(0, sizes.numel() - 1)], 0)
        ans = rt.ask("calculator", _cuda(qs), sc, op="sum")
        assert torch.equal(ans.count.cpu().to(torch.int64), n) and torch.equal(ans.n.cpu().to(torch.int64), n)
        assert ans.oob == 2 and ans.val.numel() == int(n.sum())
        ok = g != 4
        assert torch.equal(ans.value.cpu()[ok], (n * qs.a0 * qs.a1)[ok])
        assert torch.equal(ans.value.cpu()[~ok], ((n - 1) * qs.a0 * qs.a1)[~ok])  # the OK rows still fold
        assert torch.equal(ans.status.cpu(), torch.where(ok, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
        first = ans.first.cpu()
        assert torch.equal(ans.bad_row.cpu().to(torch.int64), torch.where(ok, -1, first + 123))
        assert torch.equal(ans.n_ok.cpu().to(torch.int64), torch.where(ok, n, n - 1))
        want = {f: getattr(ans, f).clone() for f in FIELDS}
        val, st = ans.val.clone(), ans.st.clone()
        # the Send's wrappers apply to the expanded calls; the ledger counts T messages
        for kw in ({"coalesce": True, "cache": True, "retries": 2}, {"coalesce": True}, {"cache": True}):
            ans = rt_led.ask("calculator", _cuda(qs), sc, op="sum", **kw)
            assert torch.equal(ans.val, val) and torch.equal(ans.st, st)
            for f in FIELDS:
                assert torch.equal(getattr(ans, f), want[f]), (kw, f)
        led = rt_led.stats()["ledger"]
        assert led["sends"] == 3 and led["messages"] == 3 * int(n.sum())
        assert rt_led.stats()["coalesce"]["messages"] == 2 * int(n.sum())
        # nothing to send: no Send, the identities
        sent = rt.exchange.counters.sent
        ans = rt.ask("calculator", _cuda(MsgBatch(qs.actor[[3, 5, 8]], qs.a0[:3], qs.a1[:3], None, METHOD_CALC_MULTIPLY)),
                     sc, op="min")
        assert rt.exchange.counters.sent == sent and ans.value.cpu().tolist() == [G.INT64_MAX] * 3
        assert ans.count.cpu().tolist() == [0] * 3 and ans.status.cpu().tolist() == [STATUS_OK] * 3
        too_many = S.Scatter.members(torch.tensor([0, rt.max_batch + 2]).cuda(),
                                     torch.zeros(rt.max_batch + 2, dtype=torch.int32).cuda(), capacity=rt.max_batch + 2)
        with pytest.raises(ValueError, match="exceeds max_batch"):
            rt.ask("calculator", _cuda(MsgBatch(qs.actor[:1] * 0, qs.a0[:1], qs.a1[:1], None, METHOD_CALC_MULTIPLY)),
                   too_many)
        assert rt.exchange.counters.sent == sent
    finally:
        rt.close()
        rt_led.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_ask_with_retries_over_a_retry_mix_gpu(delivery):
    """Questions whose calls fail at first: every question is one row of ``retry_mix`` (a group
    of one member), so the Ask's per-call replies are the retried Send's."""
    b, where = retry_mix()
    offsets = torch.arange(b.M + 1, dtype=torch.int64)
    qs = MsgBatch(torch.arange(b.M, dtype=torch.int32), b.a0, b.a1, None, b.method)
    rt, rt_plain = gpu_runtime(delivery), gpu_runtime(delivery)
    try:
        want = rt_plain.send("calculator", _cuda(b), retries=2)
        sc = S.Scatter.members(offsets.cuda(), b.actor.cuda(), capacity=rt.max_batch)
        ans = rt.ask("calculator", _cuda(qs), sc, op="max", retries=2, coalesce=True)
        assert torch.equal(ans.val, want[0]) and torch.equal(ans.st, want[1])
        assert int((ans.st.cpu()[where] == STATUS_FAILED).sum()) == 16
        ref = G.gather_ref(want[0], want[1], torch.arange(b.M, dtype=torch.int32), b.M, "max")
        for f in FIELDS:
            assert torch.equal(getattr(ans, f).cpu(), ref[f]), f
        # retry_scenario: RetryTest and CounterAdd rows under a method column
        M, n_c = 600, 48
        sc2 = retry_scenario(M, n_c, seed=11)
        n = M + n_c
    finally:
        rt.close()
        rt_plain.close()
    from ptype_amd.runtime import DeviceRuntime

    rt = DeviceRuntime(torch.device("cuda", 0), actors=n, service="calculator", shm=False, max_batch=1 << 13,
                       delivery=delivery, ledger=True)
    rt.place_local()
    try:
        # a question's calls share its a0 and method: group the scenario's rows by (method, a0) first
        order = torch.argsort(sc2["method"].to(torch.int64) * 16 + sc2["a0"], stable=True)
        actor, a0, method = sc2["actor"][order], sc2["a0"][order], sc2["method"][order]
        keys = method.to(torch.int64) * 16 + a0
        starts = torch.cat([torch.tensor([0]), torch.nonzero(keys[1:] != keys[:-1]).flatten() + 1, torch.tensor([n])])
        offsets = starts.to(torch.int64)
        Q = offsets.numel() - 1
        qs = MsgBatch(torch.arange(Q, dtype=torch.int32), a0[starts[:-1]], None, None, method[starts[:-1]].contiguous())
        sc = S.Scatter.members(offsets.cuda(), actor.cuda(), capacity=rt.max_batch)
        ans = rt.ask("calculator", _cuda(qs), sc, op="sum", retries=2)
        assert torch.equal(ans.st.cpu(), sc2["st"][order]) and torch.equal(ans.val.cpu(), sc2["val"][order])
        grp = torch.repeat_interleave(torch.arange(Q), offsets[1:] - offsets[:-1]).to(torch.int32)
        ref = G.gather_ref(ans.val, ans.st, grp, Q, "sum")
        for f in FIELDS:
            assert torch.equal(getattr(ans, f).cpu(), ref[f]), f
        assert 0 < int((ans.status == STATUS_FAILED).sum()) < Q
        led = rt.stats()["ledger"]
        assert led["sends"] == 1 and led["messages"] == n
    finally:
        rt.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_ask_multirank_fakecomm():
    """Two in-process ranks, each asks its own questions through ``DeviceRuntime.ask`` of a
    runtime that is given the rank's FakeComm exchange; rank 1's second Ask expands into
    nothing and joins the collective Send with an empty batch."""
    from ptype_amd.runtime import DeviceRuntime

    R_, n, M = 2, 6000, 1 << 13
    fc = hip().FakeComm(R_)
    sizes, offsets, members, qs = broadcast_case(n)
    results, inner, errors = [None] * R_, [None] * R_, []
    start = threading.Barrier(R_)

    def asks(r):
        if r == 0:
            return [(qs, "sum"), (MsgBatch(qs.actor.flip(0), qs.a0, qs.a1, None, METHOD_CALC_MULTIPLY), "min")]
        nothing = MsgBatch(torch.tensor([1, 6, -3, 40], dtype=torch.int32), qs.a0[:4], qs.a1[:4], None,
                           METHOD_CALC_MULTIPLY)
        return [(MsgBatch(qs.actor, qs.a1, qs.a0 * 3, None, METHOD_CALC_MULTIPLY), "max"), (nothing, "sum")]

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
                    sc = S.Scatter.members(offsets.cuda(), members.cuda(), capacity=M)
                    start.wait(timeout=60)
                    out = []
                    for q, op in asks(r):
                        ans = rt.ask("calculator", _cuda(q), sc, op=op)
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
    sc = S.Scatter.members(offsets, members)
    for r in range(R_):
        for (q, op), got in zip(asks(r), results[r]):
            ref = S.scatter_ref(sc, q)
            missing = ref["actor"] >= n
            assert torch.equal(got["st"], torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), (r, op)
            assert torch.equal(got["val"][~missing], (ref["a0"] * ref["a1"])[~missing]), (r, op)
            want = G.gather_ref(got["val"], got["st"], ref["group"], q.M, op)
            for f in FIELDS:
                assert torch.equal(got[f], want[f]), (r, op, f)
            assert torch.equal(got["first"], ref["first"]) and torch.equal(got["n"], ref["n"])
    assert inner[1][1] == 0 and inner[0][1] > 0 and results[1][1]["count"].tolist() == [0] * 4


# ---------------------------------------------------------------- Client.Ask through Join
def test_client_ask_through_join_gpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    cfg, c = _join(tmp_path, ports, True)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        sizes, offsets, members, qs = broadcast_case(c.runtime.total_actors)
        sc = S.Scatter.members(offsets.cuda(), members.cuda(), capacity=1 << 14)
        ref = S.scatter_ref(sc, qs)
        client = c.NewClient("calculator", C.ConnConfig())
        plain = client.Send(MsgBatch(ref["actor"].cuda(), ref["a0"].cuda(), ref["a1"].cuda(), None, METHOD_CALC_MULTIPLY))
        for k, op in enumerate(("sum", "max", "sum")):
            ans = client.Ask(_cuda(qs), sc, op=op)
            assert torch.equal(ans.val, plain[0]) and torch.equal(ans.st, plain[1])
            want = G.gather_ref(plain[0], plain[1], ref["group"], qs.M, op)
            for f in FIELDS:
                assert torch.equal(getattr(ans, f).cpu(), want[f]), (op, f)
        assert int((ans.status == STATUS_NO_ACTOR).sum()) == 2
        assert c.Stats()["runtime"]["scatter"] == {"asks": 3, "questions": 3 * qs.M, "rows": 3 * ref["total"], "oob": 6}
        assert c.Stats()["runtime"]["ledger"]["sends"] == 4
        client.Close()
    finally:
        server.Close()
