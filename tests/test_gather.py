"""Reply gather on the host: the numpy reference on hand-built cases, its agreement
with the optimus gather, the argument checks and ``gather=`` through the runtime on
CPU tensors (ops/gather.py)."""
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.models import optimus
from ptype_amd.ops import gather as G
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_RETRY_TEST, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK,
                                   STATUS_OVERFLOW)

from test_coalesce import multiply_batch, retry_mix
from test_coalesce import runtime as cpu_runtime
from test_send_retries import join_world1, retry_scenario, world1

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
OK, F, NA = STATUS_OK, STATUS_FAILED, STATUS_NO_ACTOR


def i64(x):
    return torch.tensor(x, dtype=torch.int64)


def i32(x):
    return torch.tensor(x, dtype=torch.int32)


def ref(val, st, group, groups, op, sentinel=None):
    r = G.gather_ref(i64(val), i32(st), i32(group), groups, op, sentinel)
    return {k: v.tolist() for k, v in r.items()}


def same(g, want):
    """A Gather's outputs equal a gather_ref dict, field for field."""
    got = g.outputs()
    for f in G.Gather.FIELDS:
        assert got[f].dtype == want[f].dtype and torch.equal(got[f], want[f]), f


# ---------------------------------------------------------------- gather_ref, numbers written out
def test_first_ne_bad_row_before_at_and_after_the_hit():
    #        row:  0   1   2   3   4   5   6   7   8   9  10  11
    group = [0,  0,  0,  1,  1,  1,  2,  2,  2,  3,  3,  3]
    val = [7,  5,  9,  7,  5,  9,  7,  5,  9,  7,  7,  7]
    # group 0: a failure before the hit; group 1: the failure is the would-be hit row (so the
    # next differing OK row is the hit, behind the failure); group 2: a failure after the hit;
    # group 3: no hit, a failure at its last row
    st = [F,  OK, OK, OK, NA, OK, OK, OK, F,  OK, OK, NA]
    r = ref(val, st, group, 4, "first_ne", 7)
    assert r["value"] == [7, 7, 5, 7]
    assert r["bad_row"] == [0, 4, -1, 11]
    assert r["status"] == [F, NA, OK, NA]
    assert r["count"] == [3, 3, 3, 3] and r["n_ok"] == [2, 2, 2, 2] and r["oob"] == [0]
    # the same rows under sum / min / max: every non-OK row counts, OK rows still fold
    r = ref(val, st, group, 4, "sum")
    assert r["value"] == [14, 16, 12, 14] and r["bad_row"] == [0, 4, 8, 11] and r["status"] == [F, NA, F, NA]
    assert ref(val, st, group, 4, "min")["value"] == [5, 7, 5, 7]
    assert ref(val, st, group, 4, "max")["value"] == [9, 9, 7, 7]


@pytest.mark.parametrize("op,identity", [("sum", 0), ("min", I64_MAX), ("max", I64_MIN), ("first_ne", 42)])
def test_group_without_rows_and_without_ok_rows(op, identity):
    # group 0: no rows; group 1: two failed rows; group 2: one OK row
    r = ref([3, 4, 5], [F, NA, OK], [1, 1, 2], 3, op, 42 if op == "first_ne" else None)
    assert r["value"] == [identity, identity, 5]
    assert r["count"] == [0, 2, 1] and r["n_ok"] == [0, 0, 1]
    assert r["bad_row"] == [-1, 0, -1] and r["status"] == [OK, F, OK]
    # no message at all: every group reads its identities
    r = ref([], [], [], 2, op, 42 if op == "first_ne" else None)
    assert r["value"] == [identity, identity] and r["count"] == [0, 0] and r["n_ok"] == [0, 0]
    assert r["bad_row"] == [-1, -1] and r["status"] == [OK, OK] and r["oob"] == [0]


def test_sum_wraps_and_extreme_values():
    r = ref([I64_MAX, 1, I64_MIN, I64_MIN, 5], [OK] * 5, [0, 0, 1, 1, 2], 3, "sum")
    assert r["value"] == [I64_MIN, 0, 5]  # 2^63 - 1 + 1 wraps; -2^63 twice is 0 mod 2^64
    vals, grp = [I64_MAX, I64_MIN, 0, I64_MAX, I64_MIN], [0, 0, 0, 1, 2]
    assert ref(vals, [OK] * 5, grp, 3, "min")["value"] == [I64_MIN, I64_MAX, I64_MIN]
    assert ref(vals, [OK] * 5, grp, 3, "max")["value"] == [I64_MAX, I64_MAX, I64_MIN]
    # a failed extreme value is not folded
    assert ref(vals, [OK, F, OK, OK, OK], grp, 3, "min")["value"] == [0, I64_MAX, I64_MIN]
    # first_ne: INT64_MIN differs from the sentinel INT64_MAX
    assert ref(vals, [OK] * 5, grp, 3, "first_ne", I64_MAX)["value"] == [I64_MIN, I64_MAX, I64_MIN]


def test_negative_and_out_of_range_ids():
    r = ref([1, 2, 4, 8, 16, 32], [OK, OK, F, OK, OK, F], [0, -1, -7, 2, 3, 1], 2, "sum")
    assert r["value"] == [1, 0] and r["count"] == [1, 1] and r["n_ok"] == [1, 0]
    assert r["oob"] == [2]  # ids 2 and 3; negative ids are not counted
    assert r["bad_row"] == [-1, 5] and r["status"] == [OK, F]


def test_sentinel_per_group_and_scalar():
    val, grp = [5, 6, 5, 6], [0, 0, 1, 1]
    assert ref(val, [OK] * 4, grp, 2, "first_ne", 5)["value"] == [6, 6]
    assert ref(val, [OK] * 4, grp, 2, "first_ne", i64([5, 6]))["value"] == [6, 5]
    assert ref(val, [OK] * 4, grp, 2, "first_ne", i64([5]))["value"] == [6, 6]
    g = G.Gather(i32(grp), 2, "first_ne", i64([5, 6])).reduce(i64(val), i32([OK] * 4))
    assert g.value.tolist() == [6, 5]
    g = G.Gather(i32(grp), 2, "first_ne", 5).reduce(i64(val), i32([OK] * 4))
    assert g.value.tolist() == [6, 6] and g.sentinel.tolist() == [5, 5]


# ---------------------------------------------------------------- the optimus gather
TARGETS = [2, 3, 4, 5, 9, 11, 25, 49, 97, 121, 143, 221, 1009, 1024, 7919 // 7, 997]


def prime_replies(f):
    """What Prime.Check answers for every range of a FanOut's batch."""
    lo, hi, t = f.batch.a0.tolist(), f.batch.a1.tolist(), f.batch.a2.tolist()
    return i64([optimus.Prime(0).Check(optimus.Args(a, b, c)) for a, b, c in zip(lo, hi, t)])


def test_first_ne_equals_the_optimus_gather():
    f = optimus.FanOut(i64(TARGETS), 8, "cpu")
    val = prime_replies(f)
    st = torch.zeros(f.M, dtype=torch.int32)
    g = f.as_gather()
    assert g.op == "first_ne" and g.groups == len(TARGETS) and g.M == f.M
    ans, status = optimus.gather_ref(val, st, f.first, f.n, f.targets)
    assert ans.tolist() == [2, 3, 2, 5, 3, 11, 5, 7, 97, 11, 11, 13, 1009, 2, 3, 997]
    g.reduce(val, st)
    assert torch.equal(g.value, ans) and torch.equal(g.status, status)
    assert torch.equal(g.count.to(torch.int64), f.n) and torch.equal(g.n_ok, g.count)
    gen = torch.Generator().manual_seed(3)
    for _ in range(8):  # failures at random rows: before, at and after the deciding range
        st = torch.zeros(f.M, dtype=torch.int32)
        rows = torch.randperm(f.M, generator=gen)[:max(1, f.M // 20)]
        st[rows] = i32([F, NA, STATUS_OVERFLOW])[torch.randint(0, 3, (rows.numel(),), generator=gen)]
        ans, status = optimus.gather_ref(val, st, f.first, f.n, f.targets)
        g.reduce(val, st)
        assert torch.equal(g.value, ans) and torch.equal(g.status, status)
        assert int((status != OK).sum()) > 0
        ans2, status2 = f.gather(val, st)
        assert torch.equal(ans2, ans) and torch.equal(status2, status)


# ---------------------------------------------------------------- argument checks
def test_gather_value_errors():
    grp = torch.zeros(8, dtype=torch.int32)
    for bad_g in (0, -1, (1 << 26) + 1):
        with pytest.raises(ValueError, match="groups"):
            G.Gather(grp, bad_g, "sum")
    with pytest.raises(ValueError, match="int32"):
        G.Gather(grp.to(torch.int64), 2, "sum")
    with pytest.raises(ValueError, match="int32"):
        G.Gather([0, 1], 2, "sum")
    with pytest.raises(ValueError, match="op"):
        G.Gather(grp, 2, "mean")
    with pytest.raises(ValueError, match="sentinel"):
        G.Gather(grp, 2, "first_ne")
    with pytest.raises(ValueError, match="sentinel"):
        G.Gather(grp, 2, "first_ne", torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="sentinel"):
        G.Gather(grp, 2, "first_ne", torch.zeros(3, dtype=torch.int64))
    g = G.Gather(grp, 2, "sum")
    with pytest.raises(ValueError, match="messages"):
        g.reduce(torch.zeros(7, dtype=torch.int64), torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        g.reduce(torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        g.reduce(torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="messages"):
        g.check_batch(9)
    # a wrong device: the sentinel, either reply column, or both
    meta = (lambda t: t.to("meta"))
    with pytest.raises(ValueError, match="another device"):
        G.Gather(grp, 2, "first_ne", meta(torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match="another device"):
        G.Gather(meta(grp), 2, "first_ne", torch.zeros(2, dtype=torch.int64))
    val8, st8 = torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)
    for v, s in ((meta(val8), st8), (val8, meta(st8)), (meta(val8), meta(st8))):
        with pytest.raises(ValueError, match="another device"):
            g.reduce(v, s)
    assert g.count.tolist() == [0, 0]  # nothing was reduced
    G.Gather(grp, 1 << 26, "sum").check_batch(8)  # the largest G
    # a Send refuses a Gather of another length before it sends anything
    ex, state = world1(16, 16)
    a = torch.arange(16, dtype=torch.int64)
    b = MsgBatch(torch.arange(16, dtype=torch.int32), a, a, None, METHOD_CALC_MULTIPLY)
    for send in (ex.send, ex.send_all):
        with pytest.raises(ValueError, match="messages"):
            send(b, gather=g)
    assert ex.counters.sent == 0


def test_m_zero_is_legal():
    g = G.Gather(torch.zeros(0, dtype=torch.int32), 3, "min")
    g.reduce(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert g.value.tolist() == [I64_MAX] * 3 and g.count.tolist() == [0] * 3 and g.status.tolist() == [OK] * 3


# ---------------------------------------------------------------- through the exchange and the runtime
def test_exchange_send_and_send_all_gather_cpu():
    M, n_c = 64, 16
    sc = retry_scenario(M, n_c)
    ex, state = world1(M + n_c, M + n_c)
    req = MsgBatch(sc["actor"], sc["a0"], None, None, sc["method"])
    grp = (torch.arange(M + n_c, dtype=torch.int32) // 7)
    g = G.Gather(grp, 12, "sum")
    val, st = ex.send_all(req, retries=2, gather=g)
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"])  # the per-message replies are unchanged
    same(g, G.gather_ref(val, st, grp, 12, "sum"))
    assert int((g.status != OK).sum()) > 0  # callsBeforePass 4 still fails after two retries
    state.zero_()
    val, st = ex.send(req, gather=g)  # one attempt: more failures, gathered as they are
    same(g, G.gather_ref(val, st, grp, 12, "sum"))
    assert int((st == F).sum()) > int((sc["st"] == F).sum())


@pytest.mark.parametrize("op", ["sum", "min", "max", "first_ne"])
@pytest.mark.parametrize("kw", [{}, {"coalesce": True}, {"cache": True}, {"coalesce": True, "cache": True}])
def test_runtime_send_gather_with_coalesce_and_cache_cpu(op, kw):
    M, keys = 700, 90
    b = multiply_batch(M, keys, 64, seed=5)
    grp = torch.randint(-1, 40, (M,), generator=torch.Generator().manual_seed(6)).to(torch.int32)
    rt, rt_plain = cpu_runtime(ledger=True), cpu_runtime()
    want = rt_plain.send("calculator", b)
    g = G.Gather(grp, 37, op, 0 if op == "first_ne" else None)
    for _ in range(2):  # the second cached Send is all hits
        val, st = rt.send("calculator", b, gather=g, **kw)
        assert torch.equal(val, want[0]) and torch.equal(st, want[1])
        same(g, G.gather_ref(val, st, grp, 37, op, 0))
    assert int(g.oob) == int((grp >= 37).sum()) > 0
    assert rt.stats()["ledger"]["sends"] == 2  # the ledger and the gather may both be on
    rt.send("calculator", b, **kw)  # without the argument the outputs stay
    same(g, G.gather_ref(val, st, grp, 37, op, 0))
    rt.close()
    rt_plain.close()


@pytest.mark.parametrize("ledger", [False, True])
def test_runtime_send_gather_retry_scenario_cpu(ledger):
    M = 64
    sc = retry_scenario(M)
    b = MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST)
    grp = (torch.arange(M, dtype=torch.int32) % 5)
    rt = cpu_runtime(ledger=ledger)
    g = G.Gather(grp, 5, "min")
    val, st = rt.send("calculator", b, retries=2, gather=g)
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"])  # the plain retried Send's replies
    same(g, G.gather_ref(val, st, grp, 5, "min"))
    assert g.value.tolist() == [1] * 5 and g.n_ok.tolist() == [10, 10, 10, 9, 9] and g.status.tolist() == [F] * 5
    assert g.bad_row.tolist() == [15, 11, 7, 3, 19]  # the lowest i with i % 4 == 3 in each residue class mod 5
    if ledger:
        assert rt.stats()["ledger"]["sends"] == 1
    rt.close()


def test_runtime_send_gather_with_retries_cpu():
    b, where = retry_mix()
    grp = (torch.arange(b.M, dtype=torch.int32) % 50)
    for kw in ({}, {"coalesce": True}, {"coalesce": True, "cache": True}):
        rt_plain, rt = cpu_runtime(), cpu_runtime()
        want = rt_plain.send("calculator", b, retries=2)
        g = G.Gather(grp, 50, "max")
        val, st = rt.send("calculator", b, retries=2, gather=g, **kw)
        assert torch.equal(val, want[0]) and torch.equal(st, want[1])
        assert int((st[where] == F).sum()) == 16
        same(g, G.gather_ref(val, st, grp, 50, "max"))
        rt.close()
        rt_plain.close()
    # resend_overflow=False: a plain send, its non-OK rows gathered as they are
    rt = cpu_runtime()
    g = G.Gather(grp, 50, "sum")
    val, st = rt.send("calculator", b, resend_overflow=False, gather=g)
    same(g, G.gather_ref(val, st, grp, 50, "sum"))
    with pytest.raises(ValueError, match="messages"):
        rt.send("calculator", multiply_batch(10, 5, 64), gather=g)
    rt.close()


def test_client_send_gather_through_join_cpu(tmp_path, ports, monkeypatch):
    """Join -> NewClient -> Client.Send(batch, gather=g) on a CPU runtime whose group
    Join formed: the elastic Send loop gathers the Send once, after the retry rounds."""
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")

    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3, ledger=True)
    try:
        rt = c.runtime
        assert rt.membership is not None
        M = rt.total_actors
        sc = retry_scenario(M)
        client = c.NewClient("w1", C.ConnConfig(retries=2))
        b = MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST)
        grp = (torch.arange(M, dtype=torch.int32) // 8)
        g = G.Gather(grp, M // 8, "sum")
        val, st = client.Send(b, retries=2, gather=g)
        assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"])
        same(g, G.gather_ref(val, st, grp, M // 8, "sum"))
        assert g.status.tolist() == [F] * (M // 8) and g.bad_row.tolist() == [3 + 8 * k for k in range(M // 8)]
        assert g.value.tolist() == [2 * (1 + 2 + 3)] * (M // 8)
        assert c.Stats()["runtime"]["ledger"]["sends"] == 1
        mul = MsgBatch(sc["actor"], sc["a0"], sc["a0"], None, METHOD_CALC_MULTIPLY)
        g2 = G.Gather(grp, M // 8, "first_ne", 1)
        val, st = client.Send(mul, gather=g2)
        same(g2, G.gather_ref(val, st, grp, M // 8, "first_ne", 1))
        assert g2.value.tolist() == [4] * (M // 8)  # rows 1, 4, 9, 16, ...: the first product that is not 1
        client.Close()
    finally:
        c.Close()
        srv.Close()
