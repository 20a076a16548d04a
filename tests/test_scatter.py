"""Call scatter on the host: the numpy reference against a sequential Python loop, its
agreement with the optimus FanOut, the argument checks and ``ask`` through the runtime on
CPU tensors (ops/scatter.py)."""
import pytest
import torch

from ptype_amd.models import optimus
from ptype_amd.ops import gather as G
from ptype_amd.ops import scatter as S
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK, STATUS_NO_ACTOR, STATUS_OK)

from test_coalesce import runtime as cpu_runtime
from test_send_retries import world1

I64_MAX = (1 << 63) - 1
FIELDS = ("value", "status", "n_ok", "count", "bad_row")


def i64(x):
    return torch.tensor(x, dtype=torch.int64)


def i32(x):
    return torch.tensor(x, dtype=torch.int32)


def questions(actor, a0, a1=None, a2=None, method=METHOD_CALC_MULTIPLY):
    f = (lambda x: None if x is None else i64(x))
    m = method if isinstance(method, int) else torch.tensor(method, dtype=torch.int16)
    return MsgBatch(i32(actor), i64(a0), f(a1), f(a2), m)


def oracle(rule, qs):
    """The rules of the module docstring, one question and one row at a time."""
    rows, first, n, oob = [], [], [], 0
    for q in range(qs.M):
        first.append(len(rows))
        m = qs.method if isinstance(qs.method, int) else int(qs.method[q])
        if rule.rule == "ranges":
            t = int(qs.a0[q])
            cnt = 0 if t <= 0 else (t - 1) // rule.step + 1
            for k in range(cnt):
                lo = rule.first_lo if k == 0 and rule.first_lo is not None else k * rule.step
                rows.append(((rule.actor_base + len(rows)) % rule.n_actors, lo, (k + 1) * rule.step, t, m, q))
        else:
            g = int(qs.actor[q])
            if not 0 <= g < rule.G:
                oob += 1
                cnt = 0
            else:
                lo, hi = int(rule.offsets_host[g]), int(rule.offsets_host[g + 1])
                cnt = hi - lo
                for k in range(cnt):
                    rows.append((int(rule.members_host[lo + k]), int(qs.a0[q]),
                                 None if qs.a1 is None else int(qs.a1[q]), None if qs.a2 is None else int(qs.a2[q]),
                                 m, q))
        n.append(cnt)
    return rows, first, n, oob


def check_ref(rule, qs):
    rows, first, n, oob = oracle(rule, qs)
    r = S.scatter_ref(rule, qs)
    assert r["total"] == len(rows) and r["oob"] == oob
    assert r["first"].tolist() == first and r["n"].tolist() == n
    assert r["first"].dtype == torch.int64 and r["n"].dtype == torch.int32
    assert r["actor"].dtype == torch.int32 and r["group"].dtype == torch.int32 and r["a0"].dtype == torch.int64
    assert r["actor"].tolist() == [x[0] for x in rows] and r["group"].tolist() == [x[5] for x in rows]
    for j, name in enumerate(("a0", "a1", "a2"), start=1):
        if rows and rows[0][j] is None:
            assert r[name] is None
        elif r[name] is not None:
            assert r[name].tolist() == [x[j] for x in rows], name
    if isinstance(qs.method, int):
        assert r["method"] == qs.method
    else:
        assert r["method"].dtype == torch.int16 and r["method"].tolist() == [x[4] for x in rows]
    return r


def same_expansion(exp, ref):
    """An Expansion equals a scatter_ref dict, field for field."""
    assert exp.total == ref["total"] and exp.oob == ref["oob"]
    b = exp.batch
    for got, name in ((b.actor, "actor"), (b.a0, "a0"), (b.a1, "a1"), (b.a2, "a2"), (exp.group, "group"),
                      (exp.first, "first"), (exp.n, "n")):
        want = ref[name]
        assert (got is None) == (want is None), name
        if want is not None:
            assert got.dtype == want.dtype and torch.equal(got.cpu(), want), name
    if isinstance(ref["method"], int):
        assert b.method == ref["method"]
    else:
        assert b.method.dtype == torch.int16 and torch.equal(b.method.cpu(), ref["method"])


# ---------------------------------------------------------------- scatter_ref against the loop
@pytest.mark.parametrize("first_lo", [None, 2, -7])
@pytest.mark.parametrize("step", [1, 10, 7])
def test_ranges_reference_against_the_loop(step, first_lo):
    t = [0, -1, -(1 << 62), 1, step - 1, step, step + 1, 3 * step, 3 * step + 1, 97, 0, 0, 5]
    rule = S.Scatter.ranges(step, 5, first_lo=first_lo, actor_base=3)
    r = check_ref(rule, questions([9] * len(t), t, [1] * len(t), None, METHOD_PRIME_CHECK))
    assert r["total"] > 0 and 0 in r["n"].tolist()
    # a method column is copied per row; no questions at all
    check_ref(rule, questions([0] * len(t), t, method=list(range(len(t)))))
    r = check_ref(rule, questions([], []))
    assert r["total"] == 0 and r["first"].numel() == 0


def test_ranges_counts_do_not_overflow():
    rule = S.Scatter.ranges((1 << 31) - 1, 4)
    t = [1 << 62, I64_MAX, (1 << 31) - 1, 1 << 31, 0]
    n, total, oob = S.scatter_counts(rule, questions([0] * 5, t))
    want = [0 if x <= 0 else (x - 1) // rule.step + 1 for x in t]
    assert [int(x) for x in n] == want and total == sum(want) and oob == 0
    # 2**62 - 1 = (2**31 - 1) * (2**31 + 1) and 2**63 - 2 is twice that: both counts are past int32
    assert want[0] == (1 << 31) + 2 and want[1] == (1 << 32) + 3
    with pytest.raises(ValueError, match="rows exceed"):
        S.scatter_ref(rule, questions([0] * 5, t))
    # step 1: the total saturates at 2**64 - 1
    n, total, _ = S.scatter_counts(S.Scatter.ranges(1, 4), questions([0] * 3, [I64_MAX] * 3))
    assert [int(x) for x in n] == [I64_MAX] * 3 and total == (1 << 64) - 1


def test_members_reference_against_the_loop():
    #       group:   0        1   2 (empty)  3
    members = i32([5, 6, 7,  9,             1, 1, 2, 8])
    offsets = i64([0, 3, 4, 4, 8])
    rule = S.Scatter.members(offsets, members)
    g = [0, 3, 2, 4, -1, 1, 0, -(1 << 31), 2, 3, 100]
    k = len(g)
    r = check_ref(rule, questions(g, list(range(k)), [-x for x in range(k)], [7] * k))
    assert r["oob"] == 4 and r["n"].tolist() == [3, 4, 0, 0, 0, 1, 3, 0, 0, 4, 0]
    assert r["actor"].tolist()[:7] == [5, 6, 7, 1, 1, 2, 8]
    # the columns the questions lack stay None; a method column is copied per row
    check_ref(rule, questions(g, list(range(k))))
    check_ref(rule, questions(g, list(range(k)), [3] * k, None, [METHOD_ECHO if x % 2 else METHOD_CALC_MULTIPLY
                                                                   for x in range(k)]))
    check_ref(rule, questions([], []))
    check_ref(rule, questions([2, 2, -5], [1, 2, 3]))  # nothing but empty and unknown groups
    # no group at all
    none = S.Scatter.members(i64([0]), i32([]))
    r = check_ref(none, questions([0, 1], [1, 2]))
    assert r["total"] == 0 and r["oob"] == 2
    rule.set_members(i64([0, 1]), i32([42]))
    assert check_ref(rule, questions([0, 1, 0], [1, 2, 3]))["actor"].tolist() == [42, 42]


# ---------------------------------------------------------------- FanOut
@pytest.mark.parametrize("targets,n_actors", [([2, 3, 4, 91, 97, 7919, 7921], 64), ([1, 10, 11, 20, 21, 5], 7),
                                              ([1009], 1), ([], 3)])
def test_ranges_equals_fanout(targets, n_actors):
    tg = i64(targets)
    f = optimus.FanOut(tg, n_actors, "cpu")
    sc = S.Scatter.ranges(10, n_actors, first_lo=2)
    qs = MsgBatch(torch.zeros(len(targets), dtype=torch.int32), tg, None, None, METHOD_PRIME_CHECK)
    for exp in (sc.expand(qs), sc.expand(qs)):
        assert exp.total == f.M and exp.batch.method == f.batch.method
        for name in ("actor", "a0", "a1", "a2"):
            got, want = getattr(exp.batch, name), getattr(f.batch, name)
            assert got.dtype == want.dtype and torch.equal(got, want), name
        assert torch.equal(exp.first, f.first) and torch.equal(exp.n.to(torch.int64), f.n)
        if targets:
            g = f.as_gather()
            assert torch.equal(exp.group, g.group)
            mine = exp.gather("first_ne", tg)
            assert mine.groups == g.groups and mine.op == g.op and torch.equal(mine.sentinel, g.sentinel)
    same_expansion(exp, S.scatter_ref(sc, qs))


# ---------------------------------------------------------------- errors
def test_constructor_errors():
    for step in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="step"):
            S.Scatter.ranges(step, 4)
    for n_actors in (0, -3, 1 << 31):
        with pytest.raises(ValueError, match="n_actors"):
            S.Scatter.ranges(10, n_actors)
    with pytest.raises(ValueError, match="capacity"):
        S.Scatter.ranges(10, 4, capacity=0)
    with pytest.raises(ValueError, match="never decrease"):
        S.Scatter.members(i64([0, 3, 2, 4]), i32([1, 2, 3, 4]))
    with pytest.raises(ValueError, match="start at 0"):
        S.Scatter.members(i64([1, 3]), i32([1, 2, 3]))
    with pytest.raises(ValueError, match="members has"):
        S.Scatter.members(i64([0, 2, 3]), i32([1, 2, 3, 4]))
    with pytest.raises(ValueError, match="int64"):
        S.Scatter.members(i32([0, 1]), i32([1]))
    with pytest.raises(ValueError, match="int32"):
        S.Scatter.members(i64([0, 1]), i64([1]))
    with pytest.raises(ValueError, match="not a members rule"):
        S.Scatter.ranges(10, 4).set_members(i64([0]), i32([]))


def test_expand_errors_leave_the_outputs_untouched():
    sc = S.Scatter.ranges(10, 4, capacity=12, q_capacity=3)
    exp = sc.expand(questions([0, 0], [50, 70]))  # 5 + 7 rows: exactly the capacity
    assert exp.total == 12 and exp.batch.M == 12
    before = {k: getattr(sc, k).clone() for k in ("actor", "a0", "a1", "a2", "group")}
    with pytest.raises(ValueError, match="13 rows, the capacity is 12"):
        sc.expand(questions([0, 0], [50, 71]))
    with pytest.raises(ValueError, match="q_capacity"):
        sc.expand(questions([0] * 4, [1] * 4))
    with pytest.raises(TypeError):
        sc.expand(MsgBatch(i64([0]), i64([1])))
    with pytest.raises(ValueError, match="length"):
        sc.expand(MsgBatch(i32([0, 0]), i64([1])))
    for k, v in before.items():
        assert torch.equal(getattr(sc, k), v), k
    # the views of a smaller expansion do not show the rows of the larger one before it
    small = sc.expand(questions([0], [11]))
    assert small.total == 2 and small.batch.a0.tolist() == [0, 10] and small.group.tolist() == [0, 0]
    with pytest.raises(ValueError, match="nothing to gather"):
        sc.expand(questions([], [])).gather("sum")


# ---------------------------------------------------------------- ask on the CPU runtime
def world1_runtime(n, max_batch, service):
    """A CPU DeviceRuntime over the one-rank exchange of test_send_retries."""
    from ptype_amd.runtime import DeviceRuntime

    rt = DeviceRuntime(torch.device("cpu"), actors=n, service=service, max_batch=max_batch)
    rt._exchange, rt.state = world1(n, max_batch)
    return rt


@pytest.mark.parametrize("op", ["sum", "min", "max", "first_ne"])
def test_ask_equals_the_send_of_the_reference_batch_cpu(op):
    n = 40
    gen = torch.Generator().manual_seed(3)
    sizes = torch.tensor([3, 0, 1, 7, 0, 0, 12, 2])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    members = torch.randint(0, n + 6, (int(sizes.sum()),), generator=gen).to(torch.int32)  # some unknown actors
    sc = S.Scatter.members(offsets, members, capacity=256)
    g_ids = [0, 3, 9, 1, 6, -1, 2, 7, 6, 4]
    Q = len(g_ids)
    qs = questions(g_ids, torch.randint(-50, 50, (Q,), generator=gen).tolist(),
                   torch.randint(-50, 50, (Q,), generator=gen).tolist())
    sen = 4 if op == "first_ne" else None
    rt, rt_plain = world1_runtime(n, 256, "calculator"), world1_runtime(n, 256, "calculator")
    ref = S.scatter_ref(sc, qs)
    plain = rt_plain.send("calculator", MsgBatch(ref["actor"], ref["a0"], ref["a1"], ref["a2"], ref["method"]))
    want = G.gather_ref(plain[0], plain[1], ref["group"], Q, op, sen)
    for _ in range(2):
        ans = rt.ask("calculator", qs, sc, op=op, sentinel=sen)
        assert torch.equal(ans.val, plain[0]) and torch.equal(ans.st, plain[1])
        for f in FIELDS:
            assert torch.equal(getattr(ans, f), want[f]), f
        assert ans.oob == 2 and torch.equal(ans.first, ref["first"]) and torch.equal(ans.n, ref["n"])
    assert ans.count.tolist() == ref["n"].tolist()
    assert op == "first_ne" or int((ans.status == STATUS_NO_ACTOR).sum()) > 0  # (first_ne stops at its hit)
    assert rt.stats()["scatter"] == {"asks": 2, "questions": 2 * Q, "rows": 2 * ref["total"], "oob": 4}
    assert rt_plain.stats()["scatter"] == {"asks": 0, "questions": 0, "rows": 0, "oob": 0}
    # nothing to send: every question answers its identity (or sentinel) with STATUS_OK and no Send runs
    sent = rt.exchange.counters.sent
    ans = rt.ask("calculator", questions([1, -1, 99], [1, 2, 3], [1, 1, 1]), sc, op=op, sentinel=sen)
    assert rt.exchange.counters.sent == sent and ans.val.numel() == 0
    assert ans.value.tolist() == [sen if sen is not None else G.IDENTITY[op]] * 3
    assert ans.count.tolist() == [0, 0, 0] and ans.status.tolist() == [STATUS_OK] * 3 and ans.oob == 2
    ans = rt.ask("calculator", questions([], []), sc, op=op, sentinel=sen)
    assert ans.value.numel() == 0 and ans.n.numel() == 0
    # the Send's own wrappers and errors
    ans = rt.ask("calculator", qs, sc, op=op, sentinel=sen, coalesce=True, cache=True)
    for f in FIELDS:
        assert torch.equal(getattr(ans, f), want[f]), f
    with pytest.raises(ValueError, match="gather"):
        rt.ask("calculator", qs, sc, gather=G.Gather(ref["group"], Q, "sum"))
    small = world1_runtime(n, 16, "calculator")
    with pytest.raises(ValueError, match="exceeds max_batch"):
        small.ask("calculator", qs, sc, op=op, sentinel=sen)
    for r in (rt, rt_plain, small):
        r.close()


def test_ask_device_finds_the_smallest_divisor_cpu():
    targets = [2, 3, 4, 91, 97, 7919, 7921]
    rt = cpu_runtime()
    for tg in (targets, targets[::-1][:3]):  # another question on the same Scatter
        ans, status = optimus.ask_device(rt, i64(tg))
        want = [next((d for d in range(2, t) if t % d == 0), t) for t in tg]
        assert ans.tolist() == want and status.tolist() == [STATUS_OK] * len(tg)
    assert rt.stats()["scatter"]["asks"] == 2
    rt.close()
