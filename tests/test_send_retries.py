"""Bounded retries of a batched Send (``send_all(retries=...)``, ops/retry.py).

The reference's client runs every call inside ``withRetry(c.cfg.Retries, ...)``
and re-selects a connection per attempt (cluster/rpc.go:59-116); its tests use
the ``RPCRetryTest`` actor that fails until ``called >= callsBeforePass``
(cluster/rpc_test.go:55-77).  Here the same actor (``METHOD_RETRY_TEST``) runs
behind the batch path on CPU tensors: at most ``1 + retries`` attempts per
message, a message that succeeded is never run again, and each retry is routed
afresh.  All comparisons are exact.
"""
import pytest
import torch

from ptype_amd.ops import retry as R
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_RETRY_TEST, METHOD_SEQ_FOLD,
                                   STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NO_METHOD, STATUS_NOT_DELIVERED, STATUS_OK,
                                   STATUS_OVERFLOW, STATUS_RANK_LOST, STATUS_THROTTLED)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_dataplane import Host, _member


def retry_scenario(M, n_counters=0, seed=0):
    """M RetryTest messages, one per actor [0, M), callsBeforePass = 1 + i % 4;
    ``n_counters`` CounterAdd messages to actors [M, M + n_counters) mixed in at
    random places (then with an int16 method column).  Returns the batch columns
    on the CPU and the expected (value, status, state) after ``retries=2``."""
    a0 = 1 + torch.arange(M, dtype=torch.int64) % 4
    actor = torch.arange(M, dtype=torch.int32)
    method = torch.full((M,), METHOD_RETRY_TEST, dtype=torch.int16)
    ok = a0 <= 3
    val = torch.where(ok, a0, torch.zeros_like(a0))
    st = torch.where(ok, STATUS_OK, STATUS_FAILED).to(torch.int32)
    state = torch.minimum(a0, torch.full_like(a0, 3))
    retried = int((a0 >= 2).sum() + (a0 >= 3).sum())  # round 1 + round 2
    if n_counters:
        c0 = 5 + torch.arange(n_counters, dtype=torch.int64) % 3
        a0, val, state = torch.cat([a0, c0]), torch.cat([val, c0]), torch.cat([state, c0])
        actor = torch.cat([actor, torch.arange(M, M + n_counters, dtype=torch.int32)])
        method = torch.cat([method, torch.full((n_counters,), METHOD_COUNTER_ADD, dtype=torch.int16)])
        st = torch.cat([st, torch.zeros(n_counters, dtype=torch.int32)])
        p = torch.randperm(M + n_counters, generator=torch.Generator().manual_seed(seed))
        actor, a0, method, val, st = actor[p], a0[p], method[p], val[p], st[p]
    return {"actor": actor, "a0": a0, "method": method if n_counters else METHOD_RETRY_TEST, "val": val, "st": st,
            "state": state, "retried": retried}


def world1(n, max_batch, device="cpu", **kw):
    tab = RegistryTable(2 * n, device=device)
    ids = torch.arange(n)
    tab.upsert(actor_keys(ids), torch.zeros(n, dtype=torch.int32), ids.to(torch.int32))
    state = torch.zeros(n, dtype=torch.int64, device=device)
    return ActorExchange(tab, max_batch, state=state, **kw), state


# ---------------------------------------------------------------- ops.retry on CPU tensors
def test_select_reference_and_merge():
    g = torch.Generator().manual_seed(5)
    M = 1000
    status = torch.randint(0, 7, (M,), generator=g).to(torch.int32)
    b = MsgBatch(torch.arange(M, dtype=torch.int32), torch.arange(M, dtype=torch.int64) * 3,
                 torch.arange(M, dtype=torch.int64) * 5, None, torch.arange(M).to(torch.int16))
    sub, idx, K = R.select(b, status, (STATUS_FAILED, STATUS_NO_ACTOR))
    want = torch.nonzero((status == STATUS_FAILED) | (status == STATUS_NO_ACTOR)).flatten()
    assert K == want.numel() and idx.dtype == torch.int32 and torch.equal(idx.to(torch.int64), want)
    assert torch.equal(sub.actor, b.actor[want]) and torch.equal(sub.a0, b.a0[want])
    assert torch.equal(sub.a1, b.a1[want]) and sub.a2 is None and torch.equal(sub.method, b.method[want])
    # the default picks STATUS_FAILED only; a uniform method stays a scalar
    sub, idx, K = R.select(MsgBatch(b.actor, b.a0, None, None, METHOD_RETRY_TEST), status)
    assert torch.equal(idx.to(torch.int64), torch.nonzero(status == STATUS_FAILED).flatten())
    assert sub.method == METHOD_RETRY_TEST and sub.a1 is None and K == idx.numel()
    # nothing selected
    sub, idx, K = R.select(b, torch.zeros(M, dtype=torch.int32))
    assert K == 0 and idx.numel() == 0 and sub.M == 0
    # merge: an indexed assignment of both outputs
    val, st = torch.arange(M, dtype=torch.int64), status.clone()
    v2, s2 = -torch.arange(want.numel(), dtype=torch.int64) - 1, torch.zeros(want.numel(), dtype=torch.int32)
    ev, es = val.clone(), st.clone()
    ev[want], es[want] = v2, s2
    R.merge(val, st, want.to(torch.int32), v2, s2)
    assert torch.equal(val, ev) and torch.equal(st, es)


def test_send_pending_driver():
    """The sub-batch driver of the reply cache, the breaker and the limiter
    (``send_pending``) with a fake ``send``: how often it is called and with what,
    what ``after`` sees, the counts reported before the Send, and the merge."""
    M = 10
    b = MsgBatch(torch.arange(M, dtype=torch.int32), torch.arange(M, dtype=torch.int64) * 3, None, None,
                 METHOD_RETRY_TEST)
    log = []

    def send(sub):
        log.append(("send", sub))
        return sub.a0 + 100, torch.full((sub.M,), STATUS_FAILED, dtype=torch.int32), "extra", 7

    count = (lambda held, sent: log.append(("count", held, sent)))
    after = (lambda sub, out: log.append(("after", sub, out)))
    outputs = (lambda st: (-torch.arange(M, dtype=torch.int64), torch.tensor(st, dtype=torch.int32)))

    # K == 0, not collective: the outputs as they are, no call
    val, st = outputs([STATUS_OK] * M)
    out = R.send_pending(b, val, st, send, False, count, after)
    assert out[0] is val and out[1] is st and len(out) == 2 and log == [("count", M, 0)]
    # K == 0, collective: one call with an empty batch; nothing is merged
    del log[:]
    out = R.send_pending(b, val, st, send, True, count, after)
    assert [e[0] for e in log] == ["count", "send", "after"] and log[0] == ("count", M, 0)
    assert log[1][1].M == 0 and log[2][1] is log[1][1]
    assert out[0] is val and out[1] is st and out[2:] == ("extra", 7)
    assert torch.equal(val, -torch.arange(M)) and st.tolist() == [STATUS_OK] * M
    # K == M: the batch itself goes out, send's result comes back as it is, after sees the batch
    del log[:]
    val, st = outputs([R.PENDING] * M)
    out = R.send_pending(b, val, st, send, False, count, after)
    assert [e[0] for e in log] == ["count", "send", "after"] and log[0] == ("count", 0, M)
    assert log[1][1] is b and log[2][1] is b and log[2][2] is out and out[2:] == ("extra", 7)
    assert torch.equal(out[0], b.a0 + 100) and out[0] is not val
    # 0 < K < M: after sees the sub-batch, the replies are merged into the rows that travelled
    del log[:]
    val, st = outputs([R.PENDING if i % 3 == 1 else STATUS_THROTTLED for i in range(M)])
    out = R.send_pending(b, val, st, send, False, count, after)
    went = [1, 4, 7]
    assert [e[0] for e in log] == ["count", "send", "after"] and log[0] == ("count", M - 3, 3)
    sub = log[1][1]
    assert sub is log[2][1] and sub.actor.tolist() == went and sub.a0.tolist() == [3, 12, 21]
    assert sub.method == METHOD_RETRY_TEST and torch.equal(log[2][2][0], sub.a0 + 100)
    assert out[0] is val and out[1] is st and out[2:] == ("extra", 7)
    assert val.tolist() == [3 * i + 100 if i in went else -i for i in range(M)]
    assert st.tolist() == [STATUS_FAILED if i in went else STATUS_THROTTLED for i in range(M)]
    # without an after hook
    del log[:]
    R.send_pending(b, *outputs([R.PENDING] * M), send, False, count)
    assert [e[0] for e in log] == ["count", "send"]


def test_retry_on_validation():
    assert R.retry_mask() == 1 << STATUS_FAILED
    assert R.retry_mask((STATUS_FAILED, STATUS_NOT_DELIVERED, STATUS_NO_ACTOR, STATUS_NO_METHOD)) == (
        1 << STATUS_FAILED | 1 << STATUS_NOT_DELIVERED | 1 << STATUS_NO_ACTOR | 1 << STATUS_NO_METHOD)
    for bad in (STATUS_OVERFLOW, STATUS_RANK_LOST):
        with pytest.raises(ValueError, match="not retried here"):
            R.retry_mask((STATUS_FAILED, bad))
    for bad in (STATUS_OK, 7, -1, 40):
        with pytest.raises(ValueError, match="not retryable"):
            R.retry_mask((bad,))
    with pytest.raises(ValueError):
        R.retry_mask(())
    b = MsgBatch(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        R.select(b, torch.zeros(4, dtype=torch.int32), (STATUS_OVERFLOW,))


# ---------------------------------------------------------------- a world-1 CPU exchange
def test_send_all_retries_cpu():
    M = 64
    sc = retry_scenario(M)
    ex, state = world1(M, M)
    val, st = ex.send_all(MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST), retries=2)
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"]) and torch.equal(state, sc["state"])
    s = ex.stats()
    assert s.retries == 2 and s.retried == int((sc["a0"] >= 2).sum() + (sc["a0"] >= 3).sum()) == sc["retried"]
    # enough attempts for everyone: a third round runs for a0 == 4 only
    ex, state = world1(M, M)
    val, st = ex.send_all(MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST), retries=5)
    assert bool((st == STATUS_OK).all()) and torch.equal(val, sc["a0"]) and torch.equal(state, sc["a0"])
    assert ex.stats().retries == 3  # stops once nothing is left to retry


def test_send_all_without_retries_is_unchanged():
    M = 64
    sc = retry_scenario(M)
    ex, state = world1(M, M)
    val, st = ex.send_all(MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST), retries=0)
    assert torch.equal(st, torch.where(sc["a0"] >= 2, STATUS_FAILED, STATUS_OK).to(torch.int32))
    assert torch.equal(state, torch.ones(M, dtype=torch.int64))
    assert ex.stats().retries == 0 and ex.stats().retried == 0


def test_send_all_retries_mixed_methods_cpu():
    M, n_c = 64, 40
    sc = retry_scenario(M, n_c, seed=3)
    ex, state = world1(M + n_c, M + n_c)
    val, st = ex.send_all(MsgBatch(sc["actor"], sc["a0"], None, None, sc["method"]), retries=2)
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"])
    assert torch.equal(state, sc["state"])  # every counter holds exactly one application
    assert ex.stats().retries == 2


def test_send_all_reroute_sees_each_rounds_failed_logical_ids():
    M = 64
    sc = retry_scenario(M)
    ex, state = world1(M, M)
    logical = sc["actor"] + 1000  # the caller's ids: actor i is logical id 1000 + i
    calls = []

    def reroute(ids):
        calls.append(ids.clone())
        return (ids - 1000).to(torch.int32)

    val, st = ex.send_all(MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST), retries=2, reroute=reroute,
                          logical=logical)
    assert len(calls) == 2
    assert torch.equal(calls[0], logical[sc["a0"] >= 2]) and torch.equal(calls[1], logical[sc["a0"] >= 3])
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"]) and torch.equal(state, sc["state"])
    # without `logical` the batch's own actor column is what gets re-routed
    ex, state = world1(M, M)
    calls.clear()
    ex.send_all(MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST), retries=1,
                reroute=lambda ids: calls.append(ids.clone()) or ids)
    assert len(calls) == 1 and torch.equal(calls[0], sc["actor"][sc["a0"] >= 2])


def test_send_all_retries_refuses_ordered_and_bad_arguments():
    M = 16
    ex, state = world1(M, M)
    ids = torch.arange(M, dtype=torch.int32)
    a0 = torch.ones(M, dtype=torch.int64)
    with pytest.raises(ValueError, match="ordered"):
        ex.send_all(MsgBatch(ids, a0, None, None, METHOD_SEQ_FOLD), retries=1)
    col = torch.full((M,), METHOD_RETRY_TEST, dtype=torch.int16)
    col[5] = METHOD_SEQ_FOLD
    with pytest.raises(ValueError, match="ordered"):
        ex.send_all(MsgBatch(ids, a0, None, None, col), retries=1)
    with pytest.raises(ValueError, match="not retried here"):
        ex.send_all(MsgBatch(ids, a0, None, None, METHOD_RETRY_TEST), retries=1, retry_on=(STATUS_OVERFLOW,))
    with pytest.raises(ValueError):
        ex.send_all(MsgBatch(ids, a0, None, None, METHOD_RETRY_TEST), retries=-1)
    assert bool((state == 0).all())  # refused before anything ran
    ex.send_all(MsgBatch(ids, a0, None, None, METHOD_SEQ_FOLD))  # (no retries: an ordered batch is fine)
    ex._capturing = True
    with pytest.raises(ValueError, match="captur"):
        ex.send_all(MsgBatch(ids, a0, None, None, METHOD_RETRY_TEST), retries=1)


def test_fake_agreement_is_bound_to_its_communicator():
    """The in-process ranks' agreement is looked up by the communicator's address: a
    FakeComm created after another one was freed can get that address and must get an
    agreement of its own size (a 4-rank comm once inherited a freed 2-rank comm's and
    its ranks 2 and 3 failed with an IndexError, the others at the barrier)."""
    from ptype_amd.parallel.exchange import _FakeAgree

    class Comm:
        def __init__(self, size):
            self.size = size

    old = Comm(2)
    a = _FakeAgree.of(old)
    assert a.R == 2 and _FakeAgree.of(old) is a
    key = id(old)
    del old  # freed: a new communicator at the same address (moved there by hand: deterministic)
    new = Comm(4)
    _FakeAgree._by_comm[id(new)] = _FakeAgree._by_comm.pop(key)
    b = _FakeAgree.of(new)
    assert b is not a and b.R == 4 and len(b.vals) == 4
    assert _FakeAgree.of(new) is b


def test_runtime_send_retries_cpu():
    from ptype_amd.runtime import DeviceRuntime

    M = 64
    sc = retry_scenario(M)
    rt = DeviceRuntime(torch.device("cpu"), actors=M, service="calculator")
    rt.place_local()
    b = MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST)
    val, st = rt.send("calculator", b, retries=2)
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"]) and torch.equal(rt.state, sc["state"])
    assert rt.exchange.stats().retries == 2
    with pytest.raises(ValueError, match="resend_overflow"):
        rt.send("calculator", b, resend_overflow=False, retries=1)
    rt.close()


def join_world1(C, tmp_path, ports, cpu=True, actors=64, **gpu):
    pp, pc = ports(), ports()
    cfg = C.Config()
    cfg.service_name, cfg.node_name, cfg.port = "w1", "n0", ports()
    cfg.member = _member(C, 0, [pp], [pc], f"e0=http://127.0.0.1:{pp}", str(tmp_path))
    cfg.has_gpu = True
    cfg.gpu.cpu, cfg.gpu.world, cfg.gpu.actors = cpu, 1, actors
    for k, v in gpu.items():
        setattr(cfg.gpu, k, v)
    srv = C.Serve(cfg.port, Host(), host="127.0.0.1")
    return cfg, srv, C.Join(C.background(), cfg)


def test_client_send_retries_through_join_cpu(tmp_path, ports, monkeypatch):
    """Join -> NewClient -> Client.Send(batch, retries=2) on a CPU runtime (the
    elastic Send loop: the retry rounds run inside its try)."""
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd import cluster as C

    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3)
    try:
        rt = c.runtime
        M = rt.total_actors
        sc = retry_scenario(M)
        client = c.NewClient("w1", C.ConnConfig(retries=2))
        b = MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST)
        val, st = client.Send(b, retries=client.cfg.retries)
        assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"]) and torch.equal(rt.state, sc["state"])
        ex = c.Stats()["runtime"]["exchange"]
        assert ex["retries"] == 2 and ex["retried"] == sc["retried"]
        # retries=None: one attempt, as before
        rt.state.zero_()
        val, st = client.Send(b)
        assert torch.equal(st, torch.where(sc["a0"] >= 2, STATUS_FAILED, STATUS_OK).to(torch.int32))
        assert c.Stats()["runtime"]["exchange"]["retries"] == 2
        mul = MsgBatch(sc["actor"], sc["a0"], sc["a0"], None, METHOD_CALC_MULTIPLY)
        val, st = client.Send(mul, retries=2)  # nothing fails: no round runs
        assert bool((st == STATUS_OK).all()) and torch.equal(val, sc["a0"] * sc["a0"])
        assert c.Stats()["runtime"]["exchange"]["retries"] == 2
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_runtime_send_retries_reroute_through_the_replica_round_robin():
    """Every retry is routed again: with two replicas and an odd batch, a message's
    retry lands on the other replica (whose RetryTest actor has not been called
    yet), the second retry back on the first -- and the router's counter advances
    by the number of retried messages per round."""
    from ptype_amd.parallel.replicas import ReplicaRouter
    from ptype_amd.runtime import DeviceRuntime

    W, P, M = 2, 16, 15
    recs = [{"rank": r, "world": W, "count": P, "node": f"p{r}", "replica": True, "address": f"10.0.0.{r}",
             "port": 7000 + r} for r in range(W)]
    ids = torch.arange(M, dtype=torch.int32)
    b = MsgBatch(ids, torch.full((M,), 2, dtype=torch.int64), None, None, METHOD_RETRY_TEST)
    first = (1 + torch.arange(M)) % W  # round robin from index 1: the replica of the first attempt
    for retries, seq in ((1, 2 * M), (2, 3 * M)):
        rt = DeviceRuntime(torch.device("cpu"), actors=W * P, service="Prime")  # replica r's actor a: id a * W + r
        rt.place_local()
        router = ReplicaRouter("Prime", W, "10.1.0.9", 3, records=recs)
        assert router.sel == [0, 1]
        val, st = rt.send("Prime", b, router=router, retries=retries)
        assert router.seq == seq
        state = rt.state.view(P, W)[:M]
        own, other = state.gather(1, first[:, None]).flatten(), state.gather(1, (1 - first)[:, None]).flatten()
        if retries == 1:  # attempt 2 ran on the other replica: called once there, still failing
            assert bool((st == STATUS_FAILED).all()) and bool((own == 1).all()) and bool((other == 1).all())
        else:  # attempt 3 is back on the first replica: its second call passes
            assert bool((st == STATUS_OK).all()) and bool((val == 2).all())
            assert bool((own == 2).all()) and bool((other == 1).all())
        rt.close()
