"""Reply gather on the GPU: the kernels (csrc/hip/gather.hip) against the numpy
reference, by exact equality, and ``gather=`` through the exchange, the runtime,
a captured graph and Join."""
import threading

import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.models import optimus
from ptype_amd.ops import gather as G
from ptype_amd.ops import hip
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK, STATUS_FAILED,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange, SendGraph

from test_coalesce import multiply_batch, retry_mix
from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_gather import I64_MAX, I64_MIN, same
from test_ledger_gpu import STATUSES, _join
from test_send_retries import retry_scenario, world1

pytestmark = pytest.mark.gpu

T = 2048  # messages per tile of reply_gather (checked below against the module)
L = 2048  # groups a block keeps in LDS
OPS = ["sum", "min", "max", "first_ne"]
MS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
GS = [1, 2, 64, L - 1, L, L + 1, 4 * L + 3]
LAYOUTS = ["runs", "one", "random", "random_oob"]


def constants():
    assert hip().reply_gather_tile() == T
    lim = hip().reply_gather_limits()
    assert lim["lds_groups"] == L == G.LDS_GROUPS and lim["max_groups"] == G.MAX_GROUPS == 1 << 26
    assert lim["acc_words"] == G.ACC_WORDS and tuple(lim["ops"]) == G.OPS and lim["no_row"] == 0xFFFFFFFF


def layout(kind, M, groups, gen):
    if kind == "one":
        return torch.zeros(M, dtype=torch.int32)
    if kind == "runs":  # ascending runs that cross lane, wave-row and tile boundaries
        lens = torch.tensor([1, 2, 63, 64, 65, 257])[torch.randint(0, 6, (M + 1,), generator=gen)]
        ids = torch.repeat_interleave(torch.arange(M + 1), lens)[:M]
        return (ids % groups).to(torch.int32)
    if kind == "random":
        return torch.randint(0, groups, (M,), generator=gen).to(torch.int32)
    g = torch.randint(-1, groups + max(2, groups // 8), (M,), generator=gen).to(torch.int32)
    g[torch.randint(0, max(M, 1), (M // 16,), generator=gen)] = -(1 << 31)
    return g


def replies(M, gen, all_ok, full_range=False):
    if full_range:
        val = torch.randint(-2**62, 2**62, (M,), generator=gen) * 2 + torch.randint(0, 2, (M,), generator=gen)
        if M:
            where = torch.randint(0, M, (max(1, M // 8),), generator=gen)
            val[where] = torch.tensor([I64_MIN, I64_MAX])[torch.randint(0, 2, (where.numel(),), generator=gen)]
    else:
        val = torch.randint(-2**62, 2**62, (M,), generator=gen)
    if all_ok:
        st = torch.zeros(M, dtype=torch.int32)
    else:
        st = STATUSES[torch.randint(0, STATUSES.numel(), (M,), generator=gen)]
        st[torch.rand(M, generator=gen) < 0.7] = STATUS_OK
    return val, st


def check(g, val, st, grp, groups, op, sen):
    g.reduce(val.cuda(), st.cuda())
    want = G.gather_ref(val, st, grp, groups, op, None if sen is None else sen.cpu())
    same(g, want)
    assert torch.equal(g.acc.cpu(), G.Gather.acc_image(groups, op))  # re-armed by the finish kernel
    assert int(g.oob) == int((grp >= groups).sum())
    return want


def test_constants_match_the_header():
    constants()


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("op", OPS)
def test_gather_kernel_against_reference(op, kind):
    constants()
    gen = torch.Generator().manual_seed(100 + 10 * OPS.index(op) + LAYOUTS.index(kind))
    for M in MS:
        for groups in GS:
            grp = layout(kind, M, groups, gen)
            sen = None
            if op == "first_ne":
                sen = torch.randint(-2**62, 2**62, (groups,), generator=gen).cuda()
            g = G.Gather(grp.cuda(), groups, op, sen)
            for all_ok in (True, False):
                val, st = replies(M, gen, all_ok)
                if sen is not None and M:  # about half of the replies equal their group's sentinel
                    eq = (torch.rand(M, generator=gen) < 0.5) & (grp >= 0) & (grp < groups)
                    val[eq] = sen.cpu()[grp[eq].to(torch.int64)]
                check(g, val, st, grp, groups, op, sen)


def test_gather_refuses_tensors_on_another_device():
    """A CPU tensor handed to a cuda Gather raises before any launch (its pointer must
    never reach a kernel), and the outputs stay as they were."""
    grp = torch.arange(8, dtype=torch.int32).cuda() % 2
    with pytest.raises(ValueError, match="another device"):
        G.Gather(grp, 2, "first_ne", torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="another device"):
        G.Gather(grp.cpu(), 2, "first_ne", torch.zeros(2, dtype=torch.int64, device="cuda"))
    g = G.Gather(grp, 2, "sum")
    val, st = torch.arange(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)
    g.reduce(val.cuda(), st.cuda())
    before = g.outputs()
    assert before["value"].tolist() == [12, 16]
    for v, s in ((val, st), (val.cuda(), st), (val, st.cuda())):
        with pytest.raises(ValueError, match="another device"):
            g.reduce(v, s)
    torch.cuda.synchronize()
    same(g, before)
    assert torch.equal(g.acc.cpu(), G.Gather.acc_image(2, "sum"))
    gc = G.Gather(grp.cpu(), 2, "sum")
    with pytest.raises(ValueError, match="another device"):
        gc.reduce(val.cuda(), st.cuda())
    # through a Send: the replies of a cuda exchange into a CPU Gather
    ex, state = world1(8, 8, device="cuda")
    b = MsgBatch(torch.arange(8, dtype=torch.int32).cuda(), val.cuda(), val.cuda(), None, METHOD_CALC_MULTIPLY)
    with pytest.raises(ValueError, match="another device"):
        ex.send(b, gather=gc)


@pytest.mark.parametrize("op,kind,groups,blocks", [("first_ne", "runs", 64, 512), ("sum", "random_oob", L + 1, 2048)])
def test_gather_blocks_stride_over_tiles(op, kind, groups, blocks):
    """More tiles than the launch has blocks (512 with the LDS accumulators, 2048
    without): a block folds several tiles before it flushes."""
    constants()
    assert hip().reply_gather_limits()["blocks_lds" if groups <= L else "blocks_hbm"] == blocks
    gen = torch.Generator().manual_seed(5)
    M = blocks * T + T + 3
    grp = layout(kind, M, groups, gen)
    sen = torch.randint(0, 3, (groups,), generator=gen).cuda() if op == "first_ne" else None
    val, st = replies(M, gen, all_ok=False)
    if sen is not None:
        val = torch.randint(0, 3, (M,), generator=gen)
    check(G.Gather(grp.cuda(), groups, op, sen), val, st, grp, groups, op, sen)


@pytest.mark.parametrize("op", OPS)
def test_gather_kernel_full_range_values(op):
    constants()
    gen = torch.Generator().manual_seed(7)
    for M, groups, kind in [(65, 2, "random"), (T + 1, L, "runs"), (3 * T + 17, L + 1, "random_oob")]:
        grp = layout(kind, M, groups, gen)
        sen = I64_MAX if op == "first_ne" else None
        g = G.Gather(grp.cuda(), groups, op, sen)
        for all_ok in (True, False):
            val, st = replies(M, gen, all_ok, full_range=True)
            want = check(g, val, st, grp, groups, op, None if sen is None else torch.tensor([sen]))
            assert int(want["count"].sum()) > 0
        assert bool((val == I64_MIN).any()) and bool((val == I64_MAX).any())


@pytest.mark.parametrize("op", OPS)
def test_gather_repeated_use_and_unaligned_views(op):
    constants()
    gen = torch.Generator().manual_seed(8)
    M, groups = T + 65, 300
    # (first_ne: the sentinel itself is a view at an odd element offset, 8-byte aligned only)
    sen = torch.randint(0, 3, (groups + 1,), generator=gen).cuda()[1:] if op == "first_ne" else None
    assert sen is None or sen.data_ptr() % 16 == 8
    # one Gather, three inputs in a row; between them an M = 0 reduce (a Gather's M is its
    # group's length, so the empty reduce is another object's, on the same stream: it must
    # leave the first object's outputs and accumulators as they are)
    grp = layout("runs", M, groups, gen)
    g = G.Gather(grp.cuda(), groups, op, sen)
    empty = G.Gather(torch.zeros(0, dtype=torch.int32, device="cuda"), groups, op, sen)
    none = torch.zeros(0, dtype=torch.int64)
    for k in range(3):
        val, st = replies(M, gen, all_ok=k == 0)
        if sen is not None:
            val = torch.randint(0, 3, (M,), generator=gen)
        want = check(g, val, st, grp, groups, op, sen)
        check(empty, none, none.to(torch.int32), none.to(torch.int32), groups, op, sen)
        same(g, want)
        assert torch.equal(g.acc.cpu(), G.Gather.acc_image(groups, op))
    # views at an odd element offset: not 16-byte aligned, each column by another amount
    val, st = replies(M + 1, gen, all_ok=False)
    grp1 = layout("random_oob", M + 1, groups, gen)
    vg, sg, gg = val.cuda()[1:], st.cuda()[1:], grp1.cuda()[1:]
    assert vg.data_ptr() % 16 == 8 and sg.data_ptr() % 16 == 4 and gg.data_ptr() % 16 == 4
    g = G.Gather(gg, groups, op, sen)
    assert g.group.data_ptr() == gg.data_ptr() and (sen is None or g.sentinel.data_ptr() == sen.data_ptr())
    g.reduce(vg, sg)
    same(g, G.gather_ref(val[1:], st[1:], grp1[1:], groups, op, None if sen is None else sen.cpu()))
    assert torch.equal(g.acc.cpu(), G.Gather.acc_image(groups, op))


@pytest.mark.parametrize("op,groups", [("sum", 64), ("first_ne", L + 1)])
def test_gather_reduce_captured_alone(op, groups):
    constants()
    gen = torch.Generator().manual_seed(9)
    M = T + 5
    grp = layout("runs", M, groups, gen)
    sen = torch.randint(0, 3, (groups,), generator=gen).cuda() if op == "first_ne" else None
    g = G.Gather(grp.cuda(), groups, op, sen)
    val = torch.zeros(M, dtype=torch.int64, device="cuda")
    st = torch.zeros(M, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g.reduce(val, st)  # warm-up outside the capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.reduce(val, st)
    for k in range(3):
        v, t = replies(M, gen, all_ok=k == 0)
        if sen is not None:
            v = torch.randint(0, 3, (M,), generator=gen)
        val.copy_(v), st.copy_(t)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        same(g, G.gather_ref(v, t, grp, groups, op, None if sen is None else sen.cpu()))
        assert torch.equal(g.acc.cpu(), G.Gather.acc_image(groups, op)), k


def test_send_graph_gathers_every_replayed_step():
    constants()
    M, groups = T + 5, 100
    ex, state = world1(M, M, device="cuda")
    gen = torch.Generator().manual_seed(13)
    a0, a1 = torch.randint(-2**62, 2**62, (M,), generator=gen), torch.randint(-2**62, 2**62, (M,), generator=gen)
    ids = torch.randint(0, M + M // 8, (M,), generator=gen).to(torch.int32)  # some ids outside the registry
    req = MsgBatch(ids.cuda(), a0.cuda(), a1.cuda(), None, METHOD_CALC_MULTIPLY)
    out_val = torch.empty(M, dtype=torch.int64, device="cuda")
    out_status = torch.empty(M, dtype=torch.int32, device="cuda")
    grp = layout("runs", M, groups, gen)
    g = G.Gather(grp.cuda(), groups, "sum")
    graph = SendGraph(ex, req, out_val, out_status, repeat=3, gather=g)
    for k in range(2):
        if k:  # the graph reads whatever req holds at the replay
            req.a0.copy_(a1), req.a1.copy_(a1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_status.cpu(), torch.where(ids >= M, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32))
        same(g, G.gather_ref(out_val, out_status, grp, groups, "sum"))
        assert int((g.status != STATUS_OK).sum()) > 0
        assert torch.equal(g.acc.cpu(), G.Gather.acc_image(groups, "sum"))
    # capture() hands the gather on as well
    g2 = G.Gather(grp.cuda(), groups, "max")
    graph2 = ex.capture(req, out_val, out_status, gather=g2)
    graph2.replay()
    torch.cuda.synchronize()
    same(g2, G.gather_ref(out_val, out_status, grp, groups, "max"))


# ---------------------------------------------------------------- world 1 through the exchange and the runtime
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_send_all_with_gather_world1_gpu(delivery):
    M, n_c = 4096 + 65, 1000
    n = M + n_c
    sc = retry_scenario(M, n_c, seed=11)
    ex, state = world1(n, n, device="cuda", delivery=delivery)
    req = MsgBatch(sc["actor"].cuda(), sc["a0"].cuda(), None, None, sc["method"].cuda())
    grp = (torch.arange(n, dtype=torch.int32) // 9)
    groups = int(grp.max()) + 1
    g = G.Gather(grp.cuda(), groups, "sum")
    val, st = ex.send_all(req, retries=2, gather=g)
    assert torch.equal(st.cpu(), sc["st"]) and torch.equal(val.cpu(), sc["val"])
    assert ex.stats().retried == sc["retried"]
    same(g, G.gather_ref(val, st, grp, groups, "sum"))  # on the final replies: a retried message once
    assert 0 < int((g.status == STATUS_FAILED).sum()) < groups
    # send(): one attempt, no retries, some ids outside the registry
    gen = torch.Generator().manual_seed(12)
    ids = torch.randint(0, n + n // 8, (n,), generator=gen).to(torch.int32)
    a0, a1 = torch.randint(-2**62, 2**62, (n,), generator=gen), torch.randint(-2**62, 2**62, (n,), generator=gen)
    req2 = MsgBatch(ids.cuda(), a0.cuda(), a1.cuda(), None, METHOD_CALC_MULTIPLY)
    g2 = G.Gather(grp.cuda(), groups, "min")
    val2, st2 = ex.send(req2, gather=g2)
    assert torch.equal(st2.cpu(), torch.where(ids >= n, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32))
    same(g2, G.gather_ref(val2, st2, grp, groups, "min"))


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_send_gather_coalesce_cache_ledger_gpu(delivery):
    M, keys, groups = 5000, 300, 77
    b = multiply_batch(M, keys, 64, seed=8)
    bg = _cuda(b)
    grp = torch.randint(-1, groups + 3, (M,), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    rt, rt_plain = gpu_runtime(delivery, ledger=True), gpu_runtime(delivery)
    try:
        want = rt_plain.send("calculator", bg)
        for kw in ({}, {"coalesce": True}, {"cache": True}, {"coalesce": True, "cache": True}):
            g = G.Gather(grp.cuda(), groups, "first_ne", 0)
            for send in range(2):  # the second cached Send is all hits
                val, st = rt.send("calculator", bg, gather=g, **kw)
                assert torch.equal(val, want[0]) and torch.equal(st, want[1])
                same(g, G.gather_ref(val, st, grp, groups, "first_ne", 0))
        assert rt.stats()["ledger"]["sends"] == 8  # the ledger and the gather are both on
        assert rt.stats()["cache"]["hits"] > 0
    finally:
        rt.close()
        rt_plain.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_send_gather_retries_gpu(delivery):
    b, where = retry_mix()
    bg = _cuda(b)
    grp = (torch.arange(b.M, dtype=torch.int32) % 50)
    rt, rt_plain = gpu_runtime(delivery), gpu_runtime(delivery)
    try:
        want = rt_plain.send("calculator", bg, retries=2)
        g = G.Gather(grp.cuda(), 50, "max")
        val, st = rt.send("calculator", bg, retries=2, coalesce=True, gather=g)
        assert torch.equal(val, want[0]) and torch.equal(st, want[1])
        assert int((st.cpu()[where] == STATUS_FAILED).sum()) == 16
        same(g, G.gather_ref(val, st, grp, 50, "max"))
    finally:
        rt.close()
        rt_plain.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_send_all_with_gather_multirank_fakecomm():
    """Two in-process ranks, each with a Gather of its own: a rank gathers the batch it
    sent (the caller's view), whichever rank ran the messages."""
    R_, M, n, groups = 2, 4096 + 65, 6000, 3000
    fc = hip().FakeComm(R_)
    batches = []
    for r in range(R_):
        gen = torch.Generator().manual_seed(40 + r)
        m = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO], dtype=torch.int16)[torch.randint(0, 2, (M,), generator=gen)]
        batches.append((torch.randint(0, n + 500 * r, (M,), generator=gen).to(torch.int32),  # rank 1: some unknown ids
                        torch.randint(-30000, 30000, (M,), generator=gen), torch.randint(-30000, 30000, (M,), generator=gen),
                        m, layout("runs" if r else "random", M, groups, gen)))
    results, errors = [None] * R_, []
    start = threading.Barrier(R_)

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
                actor, a0, a1, m, grp = batches[r]
                g = G.Gather(grp.cuda(), groups, "sum" if r else "min")
                req = MsgBatch(actor.cuda(), a0.cuda(), a1.cuda(), None, m.cuda())
                start.wait(timeout=60)
                val, sts = ex.send_all(req, gather=g)
                s.synchronize()
                results[r] = (val.cpu(), sts.cpu(), g.outputs())
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
    for r in range(R_):
        actor, a0, a1, m, grp = batches[r]
        val, sts, out = results[r]
        missing = actor >= n
        assert torch.equal(sts, torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), r
        assert torch.equal(val[~missing], torch.where(m == METHOD_ECHO, a0, a0 * a1)[~missing]), r
        want = G.gather_ref(val, sts, grp, groups, "sum" if r else "min")
        for f in G.Gather.FIELDS:
            assert torch.equal(out[f], want[f]), (r, f)
    assert int((results[1][2]["status"] != STATUS_OK).sum()) > 0 and bool((results[0][2]["status"] == STATUS_OK).all())


# ---------------------------------------------------------------- optimus
def test_fanout_as_gather_equals_prime_gather():
    gen = torch.Generator().manual_seed(21)
    targets = torch.cat([torch.tensor([2, 3, 4, 5, 9, 97, 121, 1009, 1024]), torch.randint(2, 500, (191,), generator=gen)])
    rt = gpu_runtime("direct", actors=64)
    try:
        rt.host(optimus.SERVICE)
        f = optimus.FanOut(targets, rt.total_actors, rt.device)
        assert f.batch.method == METHOD_PRIME_CHECK and f.M <= 1 << 13
        g = f.as_gather()
        val, st = rt.send(optimus.SERVICE, f.batch, gather=g)
        ans, status = f.gather(val, st)
        assert torch.equal(g.value, ans) and torch.equal(g.status, status) and bool((status == STATUS_OK).all())
        same(g, G.gather_ref(val, st, g.group, f.T, "first_ne", f.targets.cpu()))
        want = torch.tensor([next((d for d in range(2, t) if t % d == 0), t) for t in targets.tolist()])
        assert torch.equal(ans.cpu(), want)
        # failed ranges at random rows: the existing kernel and the Gather decide alike
        st2 = st.clone()
        rows = torch.randperm(f.M, generator=gen)[:f.M // 10].cuda()
        st2[rows] = STATUS_FAILED
        ans2, status2 = f.gather(val, st2)
        g.reduce(val, st2)
        assert torch.equal(g.value, ans2) and torch.equal(g.status, status2)
        assert 0 < int((status2 != STATUS_OK).sum()) < f.T
    finally:
        rt.close()


# ---------------------------------------------------------------- Client.Send through Join
def test_client_send_gather_through_join_gpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    cfg, c = _join(tmp_path, ports, True)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        M = c.runtime.total_actors
        a = torch.arange(M, dtype=torch.int64, device="cuda") - 100
        ids = torch.arange(M, dtype=torch.int32, device="cuda")
        ids[::50] += M  # unknown actors: STATUS_NO_ACTOR rows
        b = MsgBatch(ids, a, a + 7, None, METHOD_CALC_MULTIPLY)
        grp = (torch.arange(M, dtype=torch.int32) // 20)
        groups = int(grp.max()) + 1
        client = c.NewClient("calculator", C.ConnConfig())
        plain = client.Send(b)
        g = G.Gather(grp.cuda(), groups, "min")
        for _ in range(2):
            val, st = client.Send(b, gather=g)
            assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
            same(g, G.gather_ref(val, st, grp, groups, "min"))
        assert int((g.status == STATUS_NO_ACTOR).sum()) > 0 and int((g.status == STATUS_OK).sum()) > 0
        assert c.Stats()["runtime"]["ledger"]["sends"] == 3
        client.Close()
    finally:
        server.Close()
