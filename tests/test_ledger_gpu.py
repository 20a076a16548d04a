"""The Send ledger on a real MI355X: the accounting kernel (csrc/hip/ledger.hip)
against its numpy reference, and ``ledger=`` / ``account=`` through the world-1
exchange, a captured SendGraph, in-process FakeComm ranks and ``Client.Send``.
All comparisons are exact integer equality."""
import threading

import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import hip
from ptype_amd.ops import ledger as L
from ptype_amd.ops.batch import MsgBatch, zipf_actors
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_RETRY_TEST,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange, SendGraph

from test_send_retries import retry_scenario, world1

pytestmark = pytest.mark.gpu

T = 8192  # messages per block of ledger_account (checked below against the module)
N_LOAD = 1000
U64 = (1 << 64) - 1
METHODS = torch.tensor([1, 3, 5, 0, 0x7E, 0x7FFF, -1], dtype=torch.int16)
STATUSES = torch.tensor([0, 1, 2, 3, 4, 5, 6, -1, 40], dtype=torch.int32)


def _inputs(M, a1=True, mcol=True, seed=0, method=METHOD_CALC_MULTIPLY):
    """A random batch and random replies (CPU): methods and statuses from the sets
    above, 62-bit values and arguments, actor ids in [0, 2 * N_LOAD) so that half are
    past the load table; half of the Multiply / Echo rows carry the right reply."""
    g = torch.Generator().manual_seed(1000 * seed + M % 997)
    col = (lambda: torch.randint(-2**62, 2**62, (M,), generator=g))
    m = METHODS[torch.randint(0, len(METHODS), (M,), generator=g)] if mcol else method
    b = MsgBatch(torch.randint(0, 2 * N_LOAD, (M,), generator=g).to(torch.int32), col(), col() if a1 else None, None, m)
    status = STATUSES[torch.randint(0, len(STATUSES), (M,), generator=g)]
    value = col()
    mm = m.to(torch.int64) if mcol else torch.full((M,), method, dtype=torch.int64)
    right = torch.where(mm == METHOD_ECHO, b.a0, b.a0 * (b.a1 if a1 else torch.zeros_like(b.a0)))
    value = torch.where(torch.rand(M, generator=g) < 0.5, right, value)
    return b, value, status


def _cuda(b):
    c = (lambda t: None if t is None else t.cuda())
    return MsgBatch(b.actor.cuda(), b.a0.cuda(), c(b.a1), c(b.a2), b.method if isinstance(b.method, int) else b.method.cuda())


def _total(refs):
    """The ledger words after the Sends whose ``account_ref`` words are ``refs``."""
    words = torch.zeros(L.LEDGER_WORDS, dtype=torch.int64)
    dxor = 0
    for w in refs:
        words += w
        dxor ^= int(w[L.W_DIGEST_XOR])
    words[L.W_DIGEST_XOR] = dxor
    return words


def test_ledger_layout_matches_the_header():
    w = hip().ledger_words()
    assert hip().ledger_tile() == T
    assert (w["calls"], w["method_slots"], w["status_slots"]) == (L.W_CALLS, L.METHOD_SLOTS, L.STATUS_SLOTS)
    assert (w["messages"], w["sends"], w["digest_sum"], w["digest_xor"]) == (L.W_MESSAGES, L.W_SENDS, L.W_DIGEST_SUM,
                                                                            L.W_DIGEST_XOR)
    assert (w["audited"], w["mismatch"], w["load_oob"]) == (L.W_AUDITED, L.W_MISMATCH, L.W_LOAD_OOB)
    assert w["words"] == L.LEDGER_WORDS and w["copies"] == L.COPIES and w["ticket_words"] == L.TICKET_WORDS


# 65 * T + 3: 66 blocks, more than the ticket's 64 groups (its second level runs)
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 65 * T + 3])
def test_ledger_kernel_against_reference(M):
    b, value, status = _inputs(M)
    led = L.Ledger("cuda", actors=N_LOAD)
    led.account(_cuda(b), value.cuda(), status.cuda())
    words, load = L.account_ref(b, value, status, N_LOAD)
    assert torch.equal(led.words.cpu(), words) and torch.equal(led.load.cpu(), load)
    assert not bool(led.ticket.any())  # the ticket words are zero again
    r = led.read()
    assert r["sends"] == 1 and r["messages"] == M and (r["digest_sum"], r["digest_xor"]) == L.digest(value, status)


def test_ledger_counts_every_launch():
    led = L.Ledger("cuda", actors=N_LOAD)
    refs, loads = [], torch.zeros(N_LOAD, dtype=torch.int64)
    for k, M in enumerate([0, 1, T + 1, 0, 65 * T + 3, 64]):
        b, value, status = _inputs(M, seed=k)
        led.account(_cuda(b), value.cuda(), status.cuda())
        w, ld = L.account_ref(b, value, status, N_LOAD)
        refs.append(w)
        loads += ld
    assert torch.equal(led.words.cpu(), _total(refs)) and torch.equal(led.load.cpu(), loads)
    assert led.read()["sends"] == 6  # the empty Sends included
    led.reset()
    assert not bool(led.words.any()) and not bool(led.load.any())


@pytest.mark.parametrize("a1,mcol,method", [(False, False, METHOD_CALC_MULTIPLY), (True, False, METHOD_CALC_MULTIPLY),
                                            (False, False, METHOD_ECHO), (True, False, METHOD_RETRY_TEST),
                                            (True, False, 0x7E), (False, True, 0), (True, True, 0)])
def test_ledger_column_variants(a1, mcol, method):
    M = 3 * T + 17
    b, value, status = _inputs(M, a1, mcol, seed=3, method=method)
    for n_load in (0, N_LOAD):
        led = L.Ledger("cuda", actors=n_load)
        led.account(_cuda(b), value.cuda(), status.cuda())
        words, load = L.account_ref(b, value, status, n_load)
        assert torch.equal(led.words.cpu(), words)
        assert (led.load is None and load is None) or torch.equal(led.load.cpu(), load)


def test_ledger_uniform_all_ok_is_one_bin():
    """The common case: a uniform method, every status OK (counted in registers)."""
    M = 3 * T + 17
    b, value, _ = _inputs(M, True, False, seed=4)
    value = b.a0 * b.a1
    led = L.Ledger("cuda")
    led.account(_cuda(b), value.cuda(), torch.zeros(M, dtype=torch.int32, device="cuda"))
    r = led.read()
    assert r["calls"] == {"Calculator.Multiply": {"ok": M}} and r["audited"] == M and r["mismatch"] == 0


@pytest.mark.parametrize("pattern", ["one", "per_segment", "per_16_lanes", "mod7", "zipf"])
def test_ledger_hot_actors(pattern):
    """Ids that repeat inside a wave's row of 64: all lanes one actor (one leader
    round), one actor per 256-message segment, four actors per row, seven per row
    (more than the leader rounds: the rest add on their own), Zipf traffic."""
    M, n = 3 * T + 17, 5000
    i = torch.arange(M)
    ids = {"one": lambda: torch.full((M,), 4321), "per_segment": lambda: i // 256, "per_16_lanes": lambda: i // 64,
           "mod7": lambda: (i // 4) % 7 * 11, "zipf": lambda: zipf_actors(M, n, s=1.1, seed=5).cpu()}[pattern]()
    ids = ids.to(torch.int32)
    b = MsgBatch(ids, torch.zeros(M, dtype=torch.int64), None, None, METHOD_ECHO)
    led = L.Ledger("cuda", actors=n)
    led.account(_cuda(b), torch.zeros(M, dtype=torch.int64, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda"))
    want = torch.bincount(ids.to(torch.int64), minlength=n)
    assert torch.equal(led.load.cpu(), want)
    r = led.read()
    hot_id, hot_n = r["hot"][0]
    assert hot_n == int(want.max()) and int(want[hot_id]) == hot_n and r["load_oob"] == 0
    if pattern in ("one", "zipf"):  # a single busiest actor
        assert hot_id == int(want.argmax())
    assert [c for _, c in r["hot"]] == sorted((c for _, c in r["hot"]), reverse=True)


def test_ledger_audit():
    M, k = 2 * T + 77, 5
    g = torch.Generator().manual_seed(8)
    a0, a1 = torch.randint(-2**62, 2**62, (M,), generator=g), torch.randint(-2**62, 2**62, (M,), generator=g)
    ids = torch.zeros(M, dtype=torch.int32)
    st = torch.zeros(M, dtype=torch.int32, device="cuda")
    b = MsgBatch(ids.cuda(), a0.cuda(), a1.cuda(), None, METHOD_CALC_MULTIPLY)
    value = (a0 * a1).cuda()
    led = L.Ledger("cuda")
    led.account(b, value, st)
    r = led.read()
    assert r["audited"] == M and r["mismatch"] == 0
    value[torch.tensor([0, 63, T, T + 1, M - 1], device="cuda")] += 1  # k replies corrupted on the device
    led.reset()
    led.account(b, value, st)
    r = led.read()
    assert r["audited"] == M and r["mismatch"] == k
    # Echo and CounterAdd mixed in: only the Multiply and Echo rows are audited
    m = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD], dtype=torch.int16)[
        torch.randint(0, 3, (M,), generator=g)]
    right = torch.where(m == METHOD_ECHO, a0, a0 * a1)
    right = torch.where(m == METHOD_COUNTER_ADD, a0 + 1, right)  # (whatever a counter answered)
    led.reset()
    led.account(MsgBatch(ids.cuda(), a0.cuda(), a1.cuda(), None, m.cuda()), right.cuda(), st)
    r = led.read()
    assert r["audited"] == int((m != METHOD_COUNTER_ADD).sum()) and r["mismatch"] == 0
    assert r["calls"]["Counter.Add"]["ok"] == int((m == METHOD_COUNTER_ADD).sum())


def test_ledger_unaligned_views():
    M = T + 9
    b, _, _ = _inputs(M, seed=6)
    _, value, status = _inputs(M + 1, seed=7)
    led = L.Ledger("cuda", actors=N_LOAD)
    led.account(_cuda(b), value.cuda()[1:], status.cuda()[1:])  # 8 and 4 bytes past a 16-byte boundary
    words, load = L.account_ref(b, value[1:], status[1:], N_LOAD)
    assert torch.equal(led.words.cpu(), words) and torch.equal(led.load.cpu(), load)
    # batch columns at an odd offset too
    b1, _, _ = _inputs(M + 1, seed=8)
    led.reset()
    led.account(_cuda(b1).slice(1, M + 1), value.cuda()[1:], status.cuda()[1:])
    words, load = L.account_ref(b1.slice(1, M + 1), value[1:], status[1:], N_LOAD)
    assert torch.equal(led.words.cpu(), words) and torch.equal(led.load.cpu(), load)


# ---------------------------------------------------------------- world 1 through the exchange
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_send_all_with_ledger_world1_gpu(delivery):
    M, n_c = 4096 + 65, 1000
    n = M + n_c
    sc = retry_scenario(M, n_c, seed=11)
    ex, state = world1(n, n, device="cuda", delivery=delivery)
    led = L.Ledger("cuda", actors=n)
    req = MsgBatch(sc["actor"].cuda(), sc["a0"].cuda(), None, None, sc["method"].cuda())
    val, st = ex.send_all(req, retries=2, ledger=led)
    assert torch.equal(st.cpu(), sc["st"]) and torch.equal(val.cpu(), sc["val"])
    assert ex.stats().retried == sc["retried"]
    w1, load1 = L.account_ref(req, val, st, n)
    want = torch.bincount(sc["method"].to(torch.int64) * 8 + sc["st"].to(torch.int64), minlength=128)
    assert torch.equal(w1[:128], want)  # a retried message is counted once, with its final status
    assert torch.equal(led.words.cpu(), w1) and torch.equal(led.load.cpu(), load1)
    # Multiply, some ids outside the registry
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, n + n // 8, (M,), generator=g).to(torch.int32)
    a0, a1 = torch.randint(-2**62, 2**62, (M,), generator=g), torch.randint(-2**62, 2**62, (M,), generator=g)
    req2 = MsgBatch(ids.cuda(), a0.cuda(), a1.cuda(), None, METHOD_CALC_MULTIPLY)
    val2, st2 = ex.send_all(req2, ledger=led)
    missing = ids >= n
    assert int(missing.sum()) > 0
    assert torch.equal(st2.cpu(), torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32))
    w2, load2 = L.account_ref(req2, val2, st2, n)
    assert torch.equal(led.words.cpu(), _total([w1, w2])) and torch.equal(led.load.cpu(), load1 + load2)
    r = led.read()
    assert r["sends"] == 2 and r["mismatch"] == 0 and r["audited"] == int((~missing).sum())
    assert r["calls"]["Calculator.Multiply"] == {"ok": int((~missing).sum()), "no_actor": int(missing.sum())}
    assert r["load_oob"] == int(missing.sum())
    d1, d2 = L.digest(val, st), L.digest(val2, st2)
    assert r["digest_sum"] == (d1[0] + d2[0]) & U64 and r["digest_xor"] == d1[1] ^ d2[1]


def test_send_graph_accounts_every_replayed_step():
    M = T + 5
    ex, state = world1(M, M, device="cuda")
    g = torch.Generator().manual_seed(13)
    a0, a1 = torch.randint(-2**62, 2**62, (M,), generator=g), torch.randint(-2**62, 2**62, (M,), generator=g)
    req = MsgBatch(torch.randperm(M, generator=g).to(torch.int32).cuda(), a0.cuda(), a1.cuda(), None, METHOD_CALC_MULTIPLY)
    out_val = torch.empty(M, dtype=torch.int64, device="cuda")
    out_status = torch.empty(M, dtype=torch.int32, device="cuda")
    led = L.Ledger("cuda", actors=M)
    graph = SendGraph(ex, req, out_val, out_status, repeat=3, ledger=led)
    assert led.read()["sends"] == 2  # the two warm-up sends are accounted too
    led.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_val.cpu(), a0 * a1) and bool((out_status == STATUS_OK).all())
    one, load = L.account_ref(req, out_val, out_status, M)
    r = led.read()
    assert r["sends"] == 6 and r["messages"] == 6 * M
    assert torch.equal(led.words[:128].cpu(), 6 * one[:128]) and torch.equal(led.load.cpu(), 6 * load)
    assert r["digest_sum"] == 6 * L.digest(out_val, out_status)[0] & U64
    assert r["digest_xor"] == 0  # an even number of identical steps
    assert r["audited"] == 6 * M and r["mismatch"] == 0
    # capture() hands the ledger on as well
    graph2 = ex.capture(req, out_val, out_status, ledger=led)
    led.reset()
    graph2.replay()
    torch.cuda.synchronize()
    assert led.read()["sends"] == 1 and led.read()["digest_xor"] == L.digest(out_val, out_status)[1]


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_send_all_with_ledger_multirank_fakecomm():
    """Two in-process ranks, each with a ledger of its own: a rank accounts the batch
    it sent (the caller's view), whichever rank ran the messages."""
    R_, M, n = 2, 4096 + 65, 6000
    fc = hip().FakeComm(R_)
    batches = []
    for r in range(R_):
        g = torch.Generator().manual_seed(40 + r)
        m = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO], dtype=torch.int16)[torch.randint(0, 2, (M,), generator=g)]
        if r == 1:
            m[:] = METHOD_CALC_MULTIPLY
        batches.append((torch.randint(0, n + 500 * r, (M,), generator=g).to(torch.int32),  # rank 1: some unknown ids
                        torch.randint(-30000, 30000, (M,), generator=g), torch.randint(-30000, 30000, (M,), generator=g), m))
    results, ledgers, errors = [None] * R_, [None] * R_, []
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
                led = L.Ledger("cuda", actors=n)
                actor, a0, a1, m = batches[r]
                req = MsgBatch(actor.cuda(), a0.cuda(), a1.cuda(), None, m.cuda())
                start.wait(timeout=60)
                val, sts = ex.send_all(req, ledger=led)
                s.synchronize()
                results[r] = (val.cpu(), sts.cpu())
                ledgers[r] = (led.words.cpu(), led.load.cpu(), led.read())
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
        actor, a0, a1, m = batches[r]
        val, sts = results[r]
        missing = actor >= n
        assert torch.equal(sts, torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), r
        assert torch.equal(val[~missing], torch.where(m == METHOD_ECHO, a0, a0 * a1)[~missing]), r
        words, load = L.account_ref(MsgBatch(actor, a0, a1, None, m), val, sts, n)
        assert torch.equal(ledgers[r][0], words) and torch.equal(ledgers[r][1], load), r
        rd = ledgers[r][2]
        assert rd["sends"] == 1 and rd["messages"] == M and rd["mismatch"] == 0 and rd["audited"] == int((~missing).sum())
        assert rd["load_oob"] == int(missing.sum())
    assert "Echo" in ledgers[0][2]["calls"] and "Echo" not in ledgers[1][2]["calls"]  # independent ledgers
    assert int(ledgers[1][2]["load_oob"]) > 0 and int(ledgers[0][2]["load_oob"]) == 0


# ---------------------------------------------------------------- Client.Send through Join
def _join(tmp_path, ports, ledger):
    pp, pc = ports(), ports()
    cfg = C.Config()
    cfg.service_name, cfg.node_name, cfg.port = "calculator", "gpu0", ports()
    cfg.member = C.member_config(name="m0", dir=str(tmp_path / "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                 apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                 acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                 heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
    cfg.has_gpu = True
    cfg.gpu.device, cfg.gpu.actors, cfg.gpu.max_batch = 0, 4096 + 65, 1 << 16
    cfg.gpu.ledger = ledger
    return cfg, C.Join(C.background(), cfg)


@pytest.mark.parametrize("ledger", [True, False])
def test_client_send_ledger_through_join_gpu(tmp_path, ports, monkeypatch, ledger):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    cfg, c = _join(tmp_path, ports, ledger)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        M = c.runtime.total_actors
        a = torch.arange(M, dtype=torch.int64, device="cuda") - 100
        b = MsgBatch(torch.arange(M, dtype=torch.int32, device="cuda"), a, a + 7, None, METHOD_CALC_MULTIPLY)
        client = c.NewClient("calculator", C.ConnConfig())
        for _ in range(2):
            val, st = client.Send(b)
        assert torch.equal(val, a * (a + 7)) and bool((st == STATUS_OK).all())
        if ledger:
            led = c.Stats()["runtime"]["ledger"]
            assert led["calls"] == {"Calculator.Multiply": {"ok": 2 * M}} and led["sends"] == 2
            assert led["audited"] == 2 * M and led["mismatch"] == 0 and led["digest_xor"] == 0
            assert led["digest_sum"] == 2 * L.digest(val, st)[0] & U64
            assert led["hot"][0][1] == 2 and led["load_oob"] == 0
            client.Send(b, account=False)
            assert c.Stats()["runtime"]["ledger"] == led
            client.Send(b, account=True)
            assert c.Stats()["runtime"]["ledger"]["calls"]["Calculator.Multiply"]["ok"] == 3 * M
        else:
            assert "ledger" not in c.Stats()["runtime"] and c.runtime.ledger is None
            with pytest.raises(ValueError, match="ledger"):
                client.Send(b, account=True)
        client.Close()
    finally:
        server.Close()
        c.Close()
