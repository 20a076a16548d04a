"""The rate limiter on a real MI355X: the demand, step, slots, count, resolve, admit, rearm
and clear kernels (csrc/hip/limit.hip) against the numpy model (``ops.limit.LimiterRef``),
the statuses, state words and counters compared after every Send and the workspace
checked to be at rest, and ``limit=True`` through world-1 runtimes, in-process multi-rank
FakeComm exchanges and ``Client.Send``.  All comparisons are exact integer equality."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import hip
from ptype_amd.ops import limit as LM
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.gather import Gather
from ptype_amd.ops.mailbox import audit_fold
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_RETRY_TEST, METHOD_SEQ_FOLD, STATUS_OK,
                                   STATUS_THROTTLED)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_breaker import ids_batch
from test_coalesce import runtime as cpu_runtime
from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_limit import SCRIPT, echo, echo_batch, limit_scenario, run_script

pytestmark = pytest.mark.gpu

T = 2048  # messages per tile of the streaming kernels (checked below against the module)
THR = STATUS_THROTTLED
BIG = 3 * T + 17  # four levels of the radix select at 4 bits per level


def pair(n, **kw):
    return LM.Limiter("cuda", actors=n, **kw), LM.LimiterRef(actors=n, **kw)


def both(gpu, ref, actor, bg=None, **kw):
    """One limited Send of ``ids_batch(actor)`` through the kernels and the model; the inner
    Send echoes the row.  Everything is compared; returns the statuses."""
    b = ids_batch(actor)
    rval, rst = ref.send(b, echo, **kw)[:2]
    val, st = gpu.send(_cuda(b) if bg is None else bg,
                       lambda sub: (sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32, device="cuda")), **kw)[:2]
    assert st.is_cuda and torch.equal(st.cpu(), rst) and torch.equal(val.cpu(), rval)
    assert np.array_equal(gpu.words(), ref.words())
    assert gpu.counters == ref.counters and gpu.tick == ref.tick and gpu.over == ref.over
    assert gpu.at_rest()
    return rst


def first_rows(ids, a, q):
    """The rows of ``a`` past its first ``q`` in message order."""
    return torch.nonzero(torch.as_tensor(ids) == a).flatten()[q:]


# ---------------------------------------------------------------- the kernels
def test_constants_match_the_header():
    lim = hip().limit_limits()
    assert hip().limit_tile() == T == hip().breaker_tile()
    assert (lim["pending"], lim["status"], lim["max_tick"], lim["max_actors"]) == (LM.PENDING, THR, LM.MAX_TICK,
                                                                                  LM.MAX_ACTORS)
    assert (lim["digit"], lim["max_hot"], lim["hot"], lim["ctr_words"]) == (LM.DIGIT, LM.MAX_HOT, LM.HOT, LM.CTR_WORDS)
    assert lim["busy_cap"] == LM.BUSY_CAP
    assert lim["counters"] == ("throttled", "oob", "over", "n_touched")
    assert (LM.C_THROTTLED, LM.C_OOB, LM.C_OVER, LM.C_TOUCHED) == tuple(range(4))
    for M in (0, 1, 2, 16, 17, 256, 257, T, BIG, 2**31 - 1):
        assert hip().limit_levels(M) == LM.levels(M)
    assert LM.levels(BIG) >= 4


@pytest.mark.parametrize("n", [16, 4096])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, BIG])
def test_the_script_against_the_reference(M, n):
    """Nine limited Sends and a second admission at one tick: full buckets, partial
    admissions, q == 0, capped and partial refills, idle Sends, ids outside the table
    (test_limit.py asserts that the script reaches each of them)."""
    gpu, ref = pair(n, **SCRIPT)
    assert np.array_equal(gpu.words(), ref.words())  # the clear kernel
    seen = run_script(ref, M, also=gpu, to_device=_cuda)
    if M >= 63:
        assert all(v > 0 for k, v in seen.items() if k != "restart"), seen
    assert gpu.read() == ref.read()


@pytest.mark.parametrize("burst", [1, 255, 256, 257, T, T + 5, BIG - 1, BIG])
def test_every_message_to_one_actor(burst):
    """The threshold at row 0, on wave and tile edges, on every digit boundary of the radix
    select and nowhere (burst = M: not hot); then an empty bucket: K == 0."""
    gpu, ref = pair(16, rate=1, burst=burst)
    one = [7] * BIG
    st = both(gpu, ref, one)
    assert torch.nonzero(st == THR).flatten().tolist() == list(range(burst, BIG)) and ref.over == (burst < BIG)
    st = both(gpu, ref, one)  # one token gained: row 0 alone
    assert torch.nonzero(st == 0).flatten().tolist() == [0] and ref.over == 1
    for lim in (gpu, ref):
        lim.begin()
    assert gpu.admit(_cuda(ids_batch([7]))) is None and ref.admit(ids_batch([7])) is None  # this tick's token
    calls = []

    def inner(sub):
        calls.append(sub.M)
        return sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32, device=sub.a0.device)

    # the bucket is empty at this tick: nothing travels, the inner Send is skipped
    rval, rst = ref.send(ids_batch(one), inner)
    val, st = gpu.send(_cuda(ids_batch(one)), inner)
    assert calls == [] and bool((st == THR).all()) and torch.equal(st.cpu(), rst) and not bool(val.any())
    assert np.array_equal(gpu.words(), ref.words()) and gpu.at_rest() and gpu.counters == ref.counters


def test_interleaved_ids_runs_of_length_1():
    """a, b, a, b, ...: nothing combines.  Two thresholds one row apart, then one actor
    ahead of the other so that each threshold sits in a different tile."""
    ids = torch.arange(BIG) % 2 + 3
    gpu, ref = pair(16, rate=1, burst=T // 2 + 100)  # actor 3's threshold in tile 1, actor 4's one row later
    st = both(gpu, ref, ids)
    assert torch.equal(torch.nonzero(st == THR).flatten(), torch.cat([first_rows(ids, 3, T // 2 + 100),
                                                                      first_rows(ids, 4, T // 2 + 100)]).sort()[0])
    ids = torch.where(torch.arange(BIG) < 1500, 3, ids)  # actor 3 ahead: its threshold in tile 1, actor 4's in tile 2
    gpu, ref = pair(16, rate=1, burst=T - 150)
    st = both(gpu, ref, ids)
    cut3, cut4 = int(first_rows(ids, 3, T - 150)[0]), int(first_rows(ids, 4, T - 150)[0])
    assert cut3 // T != cut4 // T and st[cut3 - 2:cut3 + 1].tolist() == [0, 0, THR] and int(st[cut4]) == THR
    both(gpu, ref, ids)


def test_every_actor_hot_and_buckets_refill_by_what_they_are_owed():
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, 4096, (BIG,), generator=g)
    gpu, ref = pair(4096, rate=1, burst=1)
    st = both(gpu, ref, ids)
    assert ref.over == int((torch.bincount(ids, minlength=4096) > 1).sum()) > 1000
    assert int((st == 0).sum()) == int(torch.unique(ids).numel())
    gpu, ref = pair(4096, rate=1, burst=3)
    for send in range(3):
        ids = torch.randint(0, 4096 >> send, (BIG,), generator=g)  # fewer actors, more rows each
        both(gpu, ref, ids)
    assert ref.read()["throttled"] > BIG


def test_runs_across_wave_and_block_edges():
    """Runs of equal ids that start in one wave (256 rows) or tile and end in the next, runs
    inside one thread's four rows, and single rows: every demand is exact, and the cut
    falls inside such runs."""
    M = 2 * T + 300
    ids = torch.arange(M) % 5 + 8  # filler
    for lo, hi, a in ((250, 262, 1), (T - 3, T + 6, 2), (T + 256 * 3 - 1, T + 256 * 3 + 1, 3), (0, 3, 4), (5, 6, 5),
                      (M - 2, M, 6), (1021, 1029, 1), (2 * T - 1, 2 * T + 1, 2)):
        ids[lo:hi] = a
    gpu, ref = pair(16, rate=1, burst=10**6)
    both(gpu, ref, ids)  # nothing is hot: the demands alone
    assert (ref.words()[1:7] & np.uint64(0xFFFFFFFF)).tolist() == [12 + 8, 9 + 2, 2, 3, 1, 2]
    for burst in (1, 2, 7, 10, 13):
        gpu, ref = pair(16, rate=2, burst=burst)
        for _ in range(2):
            st = both(gpu, ref, ids)
        assert int((st[ids == 1] == 0).sum()) == min(2, burst) and int((st == THR).sum()) > 0


def test_ids_outside_the_table_and_negative_ids():
    M = T + 70
    ids = torch.arange(M) % 6
    ids[::7] = torch.tensor([16, -1, -2**31, 2**31 - 1, 1000])[torch.arange(len(ids[::7])) % 5]
    gpu, ref = pair(16, rate=3, burst=40)
    for _ in range(3):
        st = both(gpu, ref, ids)
    out = ~((ids >= 0) & (ids < 16))
    assert bool((st[out] == 0).all()) and ref.read()["oob"] == 3 * int(out.sum()) and int((st == THR).sum()) > 0
    gpu, ref = pair(16, rate=3, burst=10**6)  # nothing hot: every limited Send counts them all the same
    both(gpu, ref, ids)
    assert ref.read() == {"throttled": 0, "oob": int(out.sum())}


def test_unaligned_actor_views():
    M = T + 9
    gpu, ref = pair(64, rate=2, burst=30)
    g = torch.Generator().manual_seed(5)
    for send in range(4):
        ids = torch.randint(0, 40, (M + 1,), generator=g).to(torch.int32)
        full = MsgBatch(ids.cuda(), torch.arange(-1, M, dtype=torch.int64).cuda(), None, None, METHOD_RETRY_TEST)
        view = MsgBatch(full.actor[1:], full.a0[1:], None, None, METHOD_RETRY_TEST)  # odd element offsets
        assert view.actor.data_ptr() % 16 == 4
        both(gpu, ref, ids[1:], bg=view)
    assert ref.counters["rejected"] > 0


def test_nothing_over_quota_and_a_rank_with_nothing_admitted():
    gpu, ref = pair(16, rate=1, burst=2)
    b = _cuda(ids_batch([1, 2, 1, 3]))
    got = []
    out = gpu.send(b, lambda sub: got.append(sub) or (sub.a0.clone(), torch.zeros(4, dtype=torch.int32, device="cuda")))
    assert got[0] is b and out[1].tolist() == [0] * 4  # the batch object itself
    ref.send(ids_batch([1, 2, 1, 3]), echo)
    for lim in (gpu, ref):
        lim.begin()
    assert gpu.admit(_cuda(ids_batch([1, 2, 2]))) is None and ref.admit(ids_batch([1, 2, 2])) is None  # drained
    calls = []

    def inner(sub):
        calls.append(sub.M)
        return sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32, device="cuda")

    val, st = gpu.send(_cuda(ids_batch([1, 2, 1])), inner, collective=True)  # a rank of a group: an empty Send
    assert calls == [0] and st.tolist() == [THR] * 3 and val.tolist() == [0] * 3 and gpu.at_rest()


def test_tick_restart_and_reset():
    last = LM.MAX_TICK
    gpu, ref = pair(16, rate=1, burst=4, _start=last - 1)
    ids = torch.arange(T + 5) % 4
    both(gpu, ref, ids)
    assert int(ref.words()[1]) == (last - 1) << 32 | 4
    both(gpu, ref, ids)  # the last tick
    st = both(gpu, ref, ids)  # the restart: every bucket is full first
    assert int((st == 0).sum()) == 16 and gpu.tick == 2 and int(ref.words()[1]) == 1 << 32 | 4
    both(gpu, ref, ids)
    gpu.reset()
    ref.reset()
    assert np.array_equal(gpu.words(), ref.words()) and not ref.words()[:16].any() and gpu.at_rest()
    assert int((both(gpu, ref, ids) == 0).sum()) == 16 and gpu.tick == 4


def test_launchers_refuse_bad_arguments():
    h = hip()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    for kw in ({"M": -1}, {"M": 2**31}, {"n": 0}, {"n": 2**28 + 1}, {"now": 0}, {"now": 2**31}, {"actor": 0},
               {"actor": p + 2}, {"ctr": 0}, {"ctr": p + 4}, {"word": 0}, {"word": p + 4}, {"demand": 0},
               {"touched": p + 2}, {"busy": 0}, {"rate": 0}, {"burst": 0}):
        a = dict(actor=p, M=8, word=p, demand=p, touched=p, hot_actor=p, rem=p, prefix=p, busy=p, ctr=p, n=8, now=1, rate=1,
                 burst=1, stream=s)
        a.update(kw)
        with pytest.raises(ValueError):
            h.limit_demand(**a)
    for kw in ({"over": 0}, {"over": 9}, {"slot": 0}, {"slot": p + 4}, {"bins": 0}, {"bins_words": 15}, {"val": p + 8},
               {"st": 0}, {"demand": 0}, {"n": 0}, {"M": 2**31}):
        a = dict(actor=p, M=8, demand=p, hot_actor=p, rem=p, prefix=p, ctr=p, n=8, over=1, slot=p, bins=p, bins_words=16,
                 val=p, st=p, stream=s)
        a.update(kw)
        with pytest.raises(ValueError):
            h.limit_cut(**a)
    for kw in ({"n": 0}, {"word": 0}, {"demand": p + 2}, {"ctr": p + 4}):
        a = dict(word=p, demand=p, ctr=p, n=8, stream=s)
        a.update(kw)
        with pytest.raises(ValueError):
            h.limit_clear(**a)
    torch.cuda.synchronize()
    assert not bool(t.any())  # nothing was written


# ---------------------------------------------------------------- world 1 on the GPU
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_send_limit_gpu(delivery):
    rt = gpu_runtime(delivery, limit_rate=2, limit_burst=3)
    try:
        plain = rt.send("calculator", _cuda(echo_batch([1, 2])))
        assert rt._limiter is None and plain[1].tolist() == [STATUS_OK] * 2  # a Send without the option creates nothing
        limit_scenario(rt, dev="cuda")
        assert rt._limiter.at_rest()
        rt.exchange._capturing = True  # as inside ActorExchange.capture
        try:
            with pytest.raises(ValueError, match="limit=True.*captur"):
                rt.send("calculator", _cuda(echo_batch([1])), limit=True)
        finally:
            rt.exchange._capturing = False
    finally:
        rt.close()


@pytest.mark.parametrize("others", [{"retries": 2}, {"coalesce": True}, {"cache": True}, {"breaker": True},
                                    {"breaker": True, "coalesce": True, "cache": True, "retries": 2}],
                         ids=["retries", "coalesce", "cache", "breaker", "all"])
def test_limit_with_the_other_wrappers_equals_the_cpu_runtime_gpu(others):
    """The limiter under each other wrapper, and under all of them with the ledger and a
    gather: RPCRetryTest rows (actor a passes at its 4 (a % 7)-th call; ids 64..71 are not
    registered) between duplicated Multiply rows.  Every Send equals the CPU runtime's, and
    so do the bucket words and the counters."""
    M = 4000
    g = torch.Generator().manual_seed(31)
    actor = torch.randint(0, 80, (M,), generator=g).to(torch.int32)
    col = torch.full((M,), METHOD_CALC_MULTIPLY, dtype=torch.int16)
    a0 = torch.randint(0, 4, (M,), generator=g)
    where = torch.randperm(M, generator=g)[:64]
    col[where], actor[where] = METHOD_RETRY_TEST, torch.arange(64, dtype=torch.int32)
    a0[where] = torch.arange(64) % 7 * 4
    a0 = torch.where(actor >= 64, torch.arange(M), a0)
    b = MsgBatch(actor, a0, torch.randint(0, 4, (M,), generator=g), None, col)
    kw = {"ledger": True, "breaker_threshold": 2, "breaker_cooldown": 2, "breaker_actors": 72, "limit_rate": 3,
          "limit_burst": 9, "limit_actors": 76}
    rt, rt_cpu = gpu_runtime("direct", **kw), cpu_runtime(**kw)
    grp = (actor % 16).to(torch.int32)
    gg, gc = Gather(grp.cuda(), 16, "sum"), Gather(grp, 16, "sum")
    try:
        bg = _cuda(b)
        for send in range(5):
            want = rt_cpu.send("calculator", b, gather=gc, limit=True, **others)
            val, st = rt.send("calculator", bg, gather=gg, limit=True, **others)
            assert torch.equal(st.cpu(), want[1]) and torch.equal(val.cpu(), want[0]), send
            assert torch.equal(gg.value.cpu(), gc.value) and torch.equal(gg.status.cpu(), gc.status)
            assert torch.equal(gg.n_ok.cpu(), gc.n_ok) and torch.equal(gg.bad_row.cpu(), gc.bad_row)
        assert np.array_equal(rt._limiter.words(), rt_cpu._limiter.words()) and rt._limiter.at_rest()
        n, want = rt.stats(), rt_cpu.stats()
        for key in ("limit", "breaker", "cache", "coalesce"):
            assert n[key] == want[key], key
        for led in (n["ledger"], want["ledger"]):
            led.pop("hot")  # (the busiest actors: the order among equal loads is the reader's)
        assert n["ledger"] == want["ledger"] and torch.equal(rt.state.cpu(), rt_cpu.state)
        assert n["limit"]["throttled"] > 0 and n["limit"]["oob"] > 0 and n["limit"]["sent"] > 0
        assert n["ledger"]["calls"]["Calculator.Multiply"]["other"] > 0 and int((st == THR).sum()) > 0
    finally:
        rt.close()
        rt_cpu.close()


@pytest.mark.parametrize("delivery", ["auto", "mailbox"])
def test_ordered_rows_keep_their_fifo_around_throttled_ones_gpu(delivery):
    """SeqFold rows: the admitted ones are each actor's first rows and are compacted in
    message order, so every actor's folds chain in row order (``audit_fold``)."""
    M, n = 3000, 64
    g = torch.Generator().manual_seed(22)
    actor = torch.randint(0, 24, (M,), generator=g).to(torch.int32)
    a0 = torch.randint(1, 99, (M,), generator=g)
    rt = gpu_runtime(delivery, limit_rate=1, limit_burst=50)
    ref = LM.LimiterRef(actors=n, rate=1, burst=50)
    try:
        for send in range(2):
            before = rt.state.cpu().clone()
            val, st = rt.send("calculator", MsgBatch(actor.cuda(), a0.cuda(), None, None, METHOD_SEQ_FOLD), limit=True)
            want = ref.send(MsgBatch(actor, a0, None, None, METHOD_SEQ_FOLD), echo)[1]
            st, val = st.cpu(), val.cpu()
            assert torch.equal(st == THR, want == THR) and int((st == THR).sum()) > 0
            keep = st != THR
            ok, order = audit_fold(actor[keep].numpy(), a0[keep].numpy(), val[keep].numpy(), st[keep].numpy(),
                                   before.numpy(), rt.state.cpu().numpy())
            assert ok, order
            assert all(seq == sorted(seq) for seq in order.values())  # per-actor FIFO
    finally:
        rt.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
@pytest.mark.parametrize("R_", [2, 4])
def test_limited_sends_multirank_fakecomm(R_):
    """Every rank limits batches of its own through ``DeviceRuntime.send(limit=True)`` of a
    runtime that is given the rank's FakeComm exchange.  Rank 0 spends the tokens of its
    second batch ahead of the Send: that batch is throttled entirely and the rank joins the
    collective Send with an empty batch; its third is cut.  The other ranks stay within
    their quota.  Every rank issues exactly one inner Send per limited Send."""
    from ptype_amd.runtime import DeviceRuntime

    M, n, sends = 3000, 6000, 3
    fc = hip().FakeComm(R_)

    def batch(r, send):
        i = torch.arange(M)
        if r != 0:
            actor = ((i * 7 + r) % n).to(torch.int32)  # one row per actor
        else:
            actor = (i % 100).to(torch.int32)  # 30 rows to each of 100 actors
        return MsgBatch(actor, i.clone(), None, None, METHOD_ECHO)

    results, counters, inner, errors = [None] * R_, [None] * R_, [None] * R_, []
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
                calls = []
                rt = DeviceRuntime(torch.device("cuda", 0), actors=n // R_, service="calculator", shm=False,
                                   max_batch=M, limit_rate=10, limit_burst=30)
                rt.rank, rt.world, rt.world0, rt.table, rt._exchange = r, R_, R_, tab, ex
                inner_send = rt._send

                def counted(service, sub, *a, **kw):
                    calls.append(sub.M)
                    return inner_send(service, sub, *a, **kw)

                rt._send = counted
                try:
                    start.wait(timeout=60)
                    out = []
                    for k in range(sends):
                        b = _cuda(batch(r, k))
                        if r == 0 and k == 1:  # the tokens of this tick are gone before the Send
                            rt._limiter.begin()
                            rt._limiter.admit(b)
                        val, sts = rt.send("calculator", b, limit=True)[:2]
                        out.append((val.cpu(), sts.cpu()))
                    s.synchronize()
                    results[r], inner[r] = out, calls
                    counters[r] = rt.stats()["limit"]
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
    i = torch.arange(M)
    for r in range(R_):
        vals, sts = [x[0] for x in results[r]], [x[1] for x in results[r]]
        if r == 0:
            assert bool((sts[0] == STATUS_OK).all()) and torch.equal(vals[0], i)  # 30 rows each: the full bucket
            assert bool((sts[1] == THR).all()) and not bool(vals[1].any())
            first10 = i < 1000  # ten tokens gained: each actor's first ten rows
            assert torch.equal(sts[2] == STATUS_OK, first10) and torch.equal(sts[2] == THR, ~first10)
            assert torch.equal(vals[2], torch.where(first10, i, 0))
            assert inner[0] == [M, 0, 1000]  # the second one carried nothing, and still joined
            # (throttled counts the admission ahead of the second Send too: 20 of each actor's 30 rows)
            assert counters[0] == {"sends": 3, "messages": 3 * M, "rejected": M + 2000, "sent": M + 1000,
                                   "throttled": 2000 + M + 2000, "oob": 0, "actors": n, "rate": 10, "burst": 30}
        else:
            assert all(bool((x == STATUS_OK).all()) for x in sts) and inner[r] == [M] * 3
            assert all(torch.equal(v, i) for v in vals)
            assert counters[r]["rejected"] == 0 and counters[r]["sent"] == 3 * M and counters[r]["throttled"] == 0


# ---------------------------------------------------------------- Client.Send through Join
@pytest.mark.parametrize("default", [False, True])
def test_client_send_limit_through_join_gpu(tmp_path, ports, monkeypatch, default):
    """``Client.Send(batch, limit=True)`` with ``gpu.limit`` unset (direct delivery), and
    ``gpu.limit: true`` with no argument (mailbox delivery)."""
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
    cfg.gpu.delivery = "mailbox" if default else "direct"
    cfg.gpu.limit_rate, cfg.gpu.limit_burst = 2, 3
    if default:
        cfg.gpu.limit = True
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        rt = c.runtime
        assert rt.limit is default
        client = c.NewClient("calculator", C.ConnConfig())
        if not default:
            client.Send(_cuda(echo_batch([1, 2])))
            assert rt._limiter is None and c.Stats()["runtime"]["limit"]["sends"] == 0
        limit_scenario(rt, dev="cuda", send=(lambda b: client.Send(b)) if default
                       else (lambda b: client.Send(b, limit=True)))
        assert c.Stats()["runtime"]["limit"]["sends"] == 4
        client.Send(_cuda(echo_batch([1])), limit=False)
        assert c.Stats()["runtime"]["limit"]["sends"] == 4
        client.Close()
    finally:
        server.Close()
        c.Close()
