"""Send coalescing on a real MI355X: the grouping, selection and fan-out kernels
(csrc/hip/coalesce.hip) against the host references (``ops.coalesce.group_ref``,
torch indexing), and ``coalesce=True`` through world-1 runtimes, in-process
multi-rank FakeComm exchanges and ``Client.Send``.  All comparisons are exact
integer equality."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import coalesce as CO
from ptype_amd.ops import hip
from ptype_amd.ops import ledger as L
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_PRIME_CHECK,
                                   STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_coalesce import multiply_batch, random_batch, retry_mix

pytestmark = pytest.mark.gpu

T = 2048  # messages per block of the grouping kernel (checked below against the module)


def _cuda(b):
    c = (lambda t: None if t is None else t.cuda())
    return MsgBatch(b.actor.cuda(), b.a0.cuda(), c(b.a1), c(b.a2), b.method if isinstance(b.method, int)
                    else b.method.cuda())


def _check(b, table_log2=None, bg=None):
    """group + select of ``b`` on the GPU against the references: lead, idx, pos, K and
    the gathered columns, exactly.  Returns (lead, K)."""
    bg = _cuda(b) if bg is None else bg
    lead = CO.group(bg, table_log2=table_log2)
    ref = CO.group_ref(b)
    assert lead.dtype == torch.int32 and lead.is_cuda and torch.equal(lead.cpu(), ref)
    sub, idx, pos, K = CO.select(bg, lead)
    rsub, ridx, rpos, rK = CO.select(b, ref)
    assert K == rK and idx.dtype == torch.int32 and torch.equal(idx.cpu(), ridx)
    assert pos.dtype == torch.int32 and torch.equal(pos.cpu(), rpos)
    assert torch.equal(sub.actor.cpu(), rsub.actor) and torch.equal(sub.a0.cpu(), rsub.a0)
    for got, want in ((sub.a1, rsub.a1), (sub.a2, rsub.a2)):
        assert (got is None) == (want is None) and (want is None or torch.equal(got.cpu(), want))
    if isinstance(b.method, int):
        assert sub.method == b.method
    else:
        assert sub.method.dtype == torch.int16 and torch.equal(sub.method.cpu(), rsub.method)
    return ref, K


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_group_and_select_sizes(M):
    assert hip().coalesce_tile() == T
    assert [bool(hip().coalesce_pure(m)) for m in range(9)] == [m in (1, 2, 3) for m in range(9)]
    # about half of the messages repeat an earlier key: 4 actors x span^2 arguments ~ M / 1.8 keys, and N keys
    # drawn x N times leave the share 1 - (1 - exp(-x)) / x of the draws as repeats (0.54 at x = 1.8)
    span = max(2, int(round((M / 8) ** 0.5)) + 1)
    b = random_batch(M, 10 + M, span=span, a2=False, methods=METHOD_CALC_MULTIPLY)
    lead, K = _check(b)
    if M > 1000:
        assert 0.3 * M < M - K < 0.7 * M
    _check(random_batch(M, 20 + M))  # a method column with pure and stateful methods, all three arguments


def test_one_group_of_identical_messages():
    M = 3 * T + 17
    one = (lambda v, dt: torch.full((M,), v, dtype=dt))
    for method in (METHOD_PRIME_CHECK, one(METHOD_ECHO, torch.int16)):
        lead, K = _check(MsgBatch(one(7, torch.int32), one(-3, torch.int64), one(1 << 40, torch.int64),
                                  one(5, torch.int64), method))
        assert K == 1 and bool((lead == 0).all())


def test_all_distinct():
    M = 3 * T + 17
    g = torch.Generator().manual_seed(3)
    b = MsgBatch(torch.randint(0, 50, (M,), generator=g).to(torch.int32), torch.randperm(M, generator=g) - 1000,
                 None, None, METHOD_CALC_MULTIPLY)
    lead, K = _check(b)
    assert K == M


@pytest.mark.parametrize("dist", [64, T])
def test_duplicate_pairs_at_a_fixed_distance(dist):
    M = 2 * T + 300
    a0 = torch.arange(M, dtype=torch.int64) * 3
    first = torch.arange(0, M - dist, 2 * dist + 1)  # i and i + dist hold one key; nothing else repeats
    a0[first + dist] = a0[first]
    lead, K = _check(MsgBatch(torch.zeros(M, dtype=torch.int32), a0, None, None, METHOD_ECHO))
    assert K == M - first.numel() and torch.equal(lead[first + dist].to(torch.int64), first)


def test_keys_that_differ_in_one_field():
    i64 = torch.iinfo(torch.int64)
    actor = torch.tensor([5, 5 - 2**31, 7, 7, 7, 7, 7, 7, 7, 7], dtype=torch.int32)  # bit 31 only
    a0 = torch.tensor([1, 1, 1, 1 + (1 << 32), i64.min, i64.max, 3, 3, 3, 3])       # above bit 31; min / max
    a1 = torch.tensor([2, 2, 2, 2, 2, 2, -1, 0, 4, 4])
    a2 = torch.tensor([0, 0, 0, 0, 0, 0, 0, 0, i64.min, -1])
    lead, K = _check(MsgBatch(actor, a0, a1, a2, METHOD_ECHO))
    assert K == 10
    col = torch.tensor([METHOD_ECHO, METHOD_CALC_MULTIPLY] * 5, dtype=torch.int16)
    lead, K = _check(MsgBatch(torch.zeros(10, dtype=torch.int32), torch.ones(10, dtype=torch.int64), None, None, col))
    assert K == 2  # the method is part of the key
    # the ten keys again and again, across waves and blocks: message i's leader is i % 10
    n = (3 * T + 17 + 9) // 10
    lead, K = _check(MsgBatch(actor.repeat(n), a0.repeat(n), a1.repeat(n), a2.repeat(n), METHOD_CALC_MULTIPLY))
    assert K == 10 and torch.equal(lead.to(torch.int64), torch.arange(10 * n) % 10)


def test_uniform_method_against_a_method_column():
    M = T + 65
    b = random_batch(M, 31, methods=METHOD_CALC_MULTIPLY)
    lead, K = _check(b)
    lead2, K2 = _check(MsgBatch(b.actor, b.a0, b.a1, b.a2, torch.full((M,), METHOD_CALC_MULTIPLY, dtype=torch.int16)))
    assert K == K2 and torch.equal(lead, lead2)
    lead3, K3 = _check(MsgBatch(b.actor, b.a0, b.a1, b.a2, METHOD_COUNTER_ADD))
    assert K3 == M


def test_absent_columns_equal_zero_columns():
    M = T + 65
    b = random_batch(M, 32, a1=False, a2=False, methods=METHOD_ECHO, span=40)
    z = torch.zeros(M, dtype=torch.int64)
    lead, K = _check(b)
    for a1, a2 in ((z, None), (None, z), (z, z)):
        lead2, K2 = _check(MsgBatch(b.actor, b.a0, a1, a2, METHOD_ECHO))
        assert K2 == K and torch.equal(lead2, lead)


def test_mixed_methods_only_the_pure_rows_group():
    M = 2 * T + 9
    g = torch.Generator().manual_seed(33)
    col = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD], dtype=torch.int16)[
        torch.randint(0, 2, (M,), generator=g)]
    b = MsgBatch(torch.full((M,), 3, dtype=torch.int32), torch.full((M,), 2, dtype=torch.int64),
                 torch.full((M,), 9, dtype=torch.int64), None, col)
    lead, K = _check(b)
    mul = col == METHOD_CALC_MULTIPLY
    first = int(torch.nonzero(mul)[0])
    assert bool((lead[mul] == first).all()) and torch.equal(lead[~mul].to(torch.int64), torch.nonzero(~mul).flatten())
    assert K == int((~mul).sum()) + 1


def test_long_probe_chains_and_the_wrap():
    """Two sets of 64 distinct keys that share a home slot of a 1024-slot table, one
    of them on the last slot (its chain wraps to slot 0), three copies of each key."""
    log2, per = 10, 64
    cand = np.arange(400_000, dtype=np.int64)
    home = CO.key_hash(9, METHOD_CALC_MULTIPLY, cand, 5, 0) & np.uint64((1 << log2) - 1)
    sets = [cand[home == np.uint64(s)][:per] for s in ((1 << log2) - 1, 500)]
    assert all(s.size == per for s in sets)
    for s, slot in zip(sets, ((1 << log2) - 1, 500)):  # the numpy hash is the device's, bit for bit
        assert all(hip().coalesce_hash(9, METHOD_CALC_MULTIPLY, int(x), 5, 0) & ((1 << log2) - 1) == slot for x in s)
    a0 = torch.from_numpy(np.concatenate(sets * 3))
    M = a0.numel()
    a0 = a0[torch.randperm(M, generator=torch.Generator().manual_seed(34))]
    b = MsgBatch(torch.full((M,), 9, dtype=torch.int32), a0, torch.full((M,), 5, dtype=torch.int64), None,
                 METHOD_CALC_MULTIPLY)
    lead, K = _check(b, table_log2=log2)
    assert K == 2 * per and M == 6 * per
    with pytest.raises(ValueError):
        CO.group(_cuda(b), table_log2=8)  # fewer than 2 M slots


def test_unaligned_column_views():
    M = T + 9
    b = random_batch(M + 1, 35)
    bg = _cuda(b)
    view = (lambda x: MsgBatch(x.actor[1:], x.a0[1:], x.a1[1:], x.a2[1:], x.method[1:]))  # odd element offsets
    lead, K = _check(view(b), bg=view(bg))
    # select and fanout given lead / pos views at an odd offset
    gl = torch.cat([torch.zeros(1, dtype=torch.int32), lead]).cuda()[1:]
    sub, idx, pos, K2 = CO.select(view(bg), gl)
    assert K2 == K and torch.equal(idx.cpu().to(torch.int64), torch.nonzero(lead == torch.arange(M)).flatten())
    v2, s2 = torch.arange(K + 1, dtype=torch.int64).cuda()[1:], torch.arange(K + 1, dtype=torch.int32).cuda()[1:]
    gp = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), pos])[1:]
    val, st = CO.fanout(gl, gp, v2, s2)
    j = pos.cpu().to(torch.int64)[lead.to(torch.int64)]
    assert torch.equal(val.cpu(), j + 1) and torch.equal(st.cpu(), (j + 1).to(torch.int32))


TS = 4096  # rows per block of the selection (the retry path's tile, checked below)

LEADS = {
    "all": lambda M: torch.arange(M, dtype=torch.int32),
    "row0": lambda M: torch.zeros(M, dtype=torch.int32),
    "every7": lambda M: (torch.arange(M) - torch.arange(M) % 7).to(torch.int32),
    "last": lambda M: torch.cat([torch.zeros(max(M - 1, 0), dtype=torch.int32),
                                 torch.full((min(M, 1),), M - 1, dtype=torch.int32)]),
}


def _select_alone(M):
    """``CO.select`` of hand-made ``lead`` columns on the GPU against its CPU path: idx,
    pos, K and every gathered column, exactly (no grouping kernel runs)."""
    i = torch.arange(M, dtype=torch.int64)
    b = MsgBatch(i.to(torch.int32) * 5 - 7, i * 3 - 2**40, None, i * i + 1, (i % 251).to(torch.int16))
    bg = _cuda(b)
    for name, make in LEADS.items():
        lead = make(M)
        assert lead.numel() == M and bool((lead.to(torch.int64) <= i).all())
        assert torch.equal(lead[lead.to(torch.int64)], lead)  # a leader leads itself
        rsub, ridx, rpos, rK = CO.select(b, lead)
        leads = [lead.cuda()]
        if name == "every7":  # and as a view 4 bytes past a 16-byte boundary
            leads.append(torch.cat([torch.zeros(1, dtype=torch.int32), lead]).cuda()[1:])
            assert M == 0 or leads[1].data_ptr() % 16 == 4
        for gl in leads:
            sub, idx, pos, K = CO.select(bg, gl)
            assert K == rK and idx.dtype == torch.int32 and torch.equal(idx.cpu(), ridx), (M, name)
            assert pos.dtype == torch.int32 and torch.equal(pos.cpu(), rpos), (M, name)
            assert torch.equal(sub.actor.cpu(), rsub.actor) and torch.equal(sub.a0.cpu(), rsub.a0), (M, name)
            assert sub.a1 is None and rsub.a1 is None and torch.equal(sub.a2.cpu(), rsub.a2), (M, name)
            assert sub.method.dtype == torch.int16 and torch.equal(sub.method.cpu(), rsub.method), (M, name)


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, TS - 1, TS, TS + 1, 3 * TS + 17])
def test_select_alone_at_its_own_tile(M):
    assert hip().retry_tile() == TS
    _select_alone(M)


def test_select_alone_more_tiles_than_summing_threads():
    """257 tiles + a partial one: the block that sums the tile counts below it (256
    threads) takes more than one value per thread."""
    _select_alone(257 * TS + 5)


@pytest.mark.parametrize("M", [1, 63, 65, T + 1, 3 * T + 17])
def test_fanout_against_torch_indexing(M):
    for seed, kw in enumerate(({}, {"methods": METHOD_ECHO, "span": 2, "actors": 1}, {"span": 1000, "actors": 1000})):
        b = random_batch(M, 50 + seed, **kw)  # K from a handful to M
        lead = CO.group_ref(b)
        _, idx, pos, K = CO.select(b, lead)
        g = torch.Generator().manual_seed(M)
        v2, s2 = torch.randint(-2**62, 2**62, (K,), generator=g), torch.randint(0, 7, (K,), generator=g).to(torch.int32)
        val, st = CO.fanout(lead.cuda(), pos.cuda(), v2.cuda(), s2.cuda())
        j = pos.to(torch.int64)[lead.to(torch.int64)]
        assert val.dtype == torch.int64 and st.dtype == torch.int32
        assert torch.equal(val.cpu(), v2[j]) and torch.equal(st.cpu(), s2[j]), (M, K)


# ---------------------------------------------------------------- world 1 on the GPU
def runtime(delivery="auto", actors=64, **kw):
    from ptype_amd.runtime import DeviceRuntime

    rt = DeviceRuntime(torch.device("cuda", 0), actors=actors, service="calculator", shm=False, max_batch=1 << 13,
                       delivery=delivery, **kw)
    rt.place_local()
    return rt


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_send_coalesce_world1_gpu(delivery):
    M, keys = 5000, 300
    b = multiply_batch(M, keys, 64, seed=8)
    bg = _cuda(b)
    rt = runtime(delivery)
    try:
        plain = rt.send("calculator", bg)
        sent = rt.exchange.counters.sent
        val, st = rt.send("calculator", bg, coalesce=True)
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
        assert torch.equal(val.cpu(), b.a0 * b.a1) and bool((st == STATUS_OK).all())
        assert rt.exchange.counters.sent - sent == keys  # the leaders, not M
        assert rt.stats()["coalesce"] == {"sends": 1, "messages": M, "executed": keys}
        # a duplicate group addressed to an unregistered actor: every member answers STATUS_NO_ACTOR
        actor = b.actor.clone()
        actor[::5] = 9999
        ug = MsgBatch(actor.cuda(), bg.a0, bg.a1, None, METHOD_CALC_MULTIPLY)
        val, st = rt.send("calculator", ug, coalesce=True)
        plain = rt.send("calculator", ug)
        assert torch.equal(st, plain[1]) and torch.equal(val, plain[0])
        assert bool((st.cpu()[::5] == STATUS_NO_ACTOR).all()) and int((st == STATUS_NO_ACTOR).sum()) == M // 5
        assert rt.stats()["coalesce"]["executed"] < keys + M // 5
        rt.exchange._capturing = True  # as inside ActorExchange.capture
        try:
            with pytest.raises(ValueError, match="captur"):
                rt.send("calculator", bg, coalesce=True)
        finally:
            rt.exchange._capturing = False
    finally:
        rt.close()


def test_stateful_method_is_never_coalesced_gpu():
    M = 5000
    rt = runtime()
    try:
        b = MsgBatch(torch.full((M,), 11, dtype=torch.int32, device="cuda"),
                     torch.ones(M, dtype=torch.int64, device="cuda"), None, None, METHOD_COUNTER_ADD)
        val, st = rt.send("calculator", b, coalesce=True)
        assert int(rt.state[11]) == M and bool((st == STATUS_OK).all())
        assert torch.equal(val.sort().values.cpu(), torch.arange(1, M + 1))
        assert rt.stats()["coalesce"] == {"sends": 1, "messages": M, "executed": M}
    finally:
        rt.close()


def test_coalesce_with_retries_gpu():
    b, where = retry_mix(5000)
    bg = _cuda(b)
    rt_plain, rt = runtime(), runtime()
    try:
        want = rt_plain.send("calculator", bg, retries=2)
        val, st = rt.send("calculator", bg, retries=2, coalesce=True)
        assert torch.equal(val, want[0]) and torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state)
        assert int((st.cpu()[where] == STATUS_FAILED).sum()) == 16 and rt.exchange.stats().retries == 2
        assert rt.stats()["coalesce"]["executed"] <= 64 + 64 * 9
    finally:
        rt.close()
        rt_plain.close()


def test_coalesce_with_a_ledger_gpu():
    M = 5000
    g = torch.Generator().manual_seed(12)
    col = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD], dtype=torch.int16)[
        torch.randint(0, 3, (M,), generator=g)]
    actor = torch.randint(0, 70, (M,), generator=g).to(torch.int32)  # ids 64..69 are not registered
    b = MsgBatch(actor, torch.randint(0, 3, (M,), generator=g), torch.randint(0, 3, (M,), generator=g), None, col)
    rt = runtime(ledger=True)
    try:
        val, st = rt.send("calculator", _cuda(b), coalesce=True)
        r = rt.stats()["ledger"]
        ok = st.cpu() == STATUS_OK
        assert r["sends"] == 1 and r["messages"] == M and r["mismatch"] == 0
        assert r["audited"] == int((ok & (col != METHOD_COUNTER_ADD)).sum())
        assert r["calls"]["Calculator.Multiply"]["ok"] == int((ok & (col == METHOD_CALC_MULTIPLY)).sum())
        assert (r["digest_sum"], r["digest_xor"]) == L.digest(val, st)
        assert rt.stats()["coalesce"]["executed"] < M
        rt.send("calculator", _cuda(b), coalesce=True, account=False)
        assert rt.stats()["ledger"] == r
    finally:
        rt.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
@pytest.mark.parametrize("R_", [2, 4])
def test_coalesced_sends_multirank_fakecomm(R_):
    """Every rank coalesces a batch of its own (a different number of distinct keys
    each, the last rank none repeated) over three Sends: each rank makes exactly
    one collective Send per coalesced Send, so the ranks stay in step."""
    M, n, sends = 5000, 6000, 3
    fc = hip().FakeComm(R_)
    batches = []
    for r in range(R_):
        if r == R_ - 1:
            a = torch.arange(M, dtype=torch.int64)
            batches.append(MsgBatch((a % n).to(torch.int32), a - 7, a + 1, None, METHOD_CALC_MULTIPLY))
        else:
            batches.append(multiply_batch(M, 200 + 150 * r, n, seed=60 + r))
    results, counters, errors = [None] * R_, [None] * R_, []
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
                co = CO.Coalescer("cuda", M)
                req = _cuda(batches[r])
                start.wait(timeout=60)
                out = []
                for _ in range(sends):
                    (val, sts), fanned = co.send(req, ex.send_all)
                    out.append((val.cpu(), sts.cpu(), fanned))
                s.synchronize()
                results[r] = out
                counters[r] = dict(co.counters)
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
        b = batches[r]
        K = M if r == R_ - 1 else 200 + 150 * r
        for val, sts, fanned in results[r]:
            assert bool((sts == STATUS_OK).all()) and torch.equal(val, b.a0 * b.a1), r
            assert fanned == (K < M)
        assert counters[r] == {"sends": sends, "messages": sends * M, "executed": sends * K}, r


# ---------------------------------------------------------------- Client.Send through Join
@pytest.mark.parametrize("default", [False, True])
def test_client_send_coalesce_through_join_gpu(tmp_path, ports, monkeypatch, default):
    """``Client.Send(batch, coalesce=True)`` with ``gpu.coalesce`` unset, and
    ``gpu.coalesce: true`` with no argument."""
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    pp, pc = ports(), ports()
    cfg = C.Config()
    cfg.service_name, cfg.node_name, cfg.port = "calculator", "gpu0", ports()
    cfg.member = C.member_config(name="m0", dir=str(tmp_path / "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                 apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                 acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                 heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
    cfg.has_gpu = True
    cfg.gpu.device, cfg.gpu.actors, cfg.gpu.max_batch = 0, 64, 1 << 13
    if default:
        cfg.gpu.coalesce = True
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        assert c.runtime.coalesce is default
        M, keys = 5000, 300
        b = multiply_batch(M, keys, c.runtime.total_actors, seed=9)
        bg = _cuda(b)
        client = c.NewClient("calculator", C.ConnConfig())
        val, st = client.Send(bg) if default else client.Send(bg, coalesce=True)
        assert torch.equal(val.cpu(), b.a0 * b.a1) and bool((st == STATUS_OK).all())
        assert c.Stats()["runtime"]["coalesce"] == {"sends": 1, "messages": M, "executed": keys}
        plain = client.Send(bg, coalesce=False)
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
        assert c.Stats()["runtime"]["coalesce"]["sends"] == 1
        client.Close()
    finally:
        server.Close()
        c.Close()
