"""The timer queue on a real MI355X: the count, scan, file, due and take kernels
(csrc/hip/timers.hip) against the numpy model (``ops.timers.TimerRef``) -- the ring, the run
table, the control and the scratch line compared word for word after every call -- and
``schedule`` / ``tick`` through world-1 runtimes on both deliveries, in-process FakeComm ranks
and ``Client.Schedule`` / ``Client.Tick`` / ``Client.Timers``.  All comparisons are exact integer
equality."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import hip
from ptype_amd.ops import timers as TM
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.dead_letters import fnv1a64
from ptype_amd.ops.mailbox import audit_fold
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_RETRY_TEST, METHOD_SEQ_FOLD,
                                   STATUS_BREAKER_OPEN, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK, STATUS_THROTTLED)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_timers import (backoff_scenario, bad_keywords_scenario, random_call, retries_and_dead_letters_scenario,
                         schedule_and_tick_scenario)

pytestmark = pytest.mark.gpu

T = 4096  # rows per block (checked below against the module)
BIG = 3 * T + 17


def pair(entries, horizon, runs=4):
    return TM.TimerQueue("cuda", entries, horizon, runs), TM.TimerRef(entries, horizon, runs)


def same_words(ref, gpu):
    torch.cuda.synchronize()
    for name in ("ring", "runs", "ctrl", "scratch"):
        got = getattr(gpu, name).cpu().numpy().view(np.uint64).reshape(getattr(ref, name).shape)
        assert np.array_equal(got, getattr(ref, name)), name
    assert gpu.read() == dict(ref.read(), full=gpu.full) and gpu.full == ref.full


def both_schedule(gpu, ref, b, d, tag=0, bg=None, dg=None):
    """One Schedule filed by the kernels and by the model -- or refused by both -- and every
    word compared.  Returns the model's result, None for a refused call."""
    bg = _cuda(b) if bg is None else bg
    dg = (d.cuda() if isinstance(d, torch.Tensor) else d) if dg is None else dg
    try:
        want = ref.schedule(b, d, tag)
    except TM.TimerQueueFull:
        with pytest.raises(TM.TimerQueueFull):
            gpu.schedule(bg, dg, tag)
        same_words(ref, gpu)
        return None
    got = gpu.schedule(bg, dg, tag)
    assert got == want
    same_words(ref, gpu)
    return want


def both_tick(gpu, ref):
    want, got = ref.tick(), gpu.tick()
    assert (got.n, got.torn) == (want["n"], 0) and want["torn"] == 0
    for c in TM.COLUMNS:
        t = getattr(got, c)
        assert t.is_cuda and t.dtype == TM._DTYPES[c] and np.array_equal(t.cpu().numpy(), want[c]), c
    same_words(ref, gpu)
    return got.n


# ---------------------------------------------------------------- the kernels
def test_layout_matches_the_header():
    lay = hip().timer_layout()
    assert lay["tile"] == T == TM.TILE
    assert (lay["record_words"], lay["header_words"], lay["control_words"], lay["scratch_words"]) == (
        TM.RECORD_WORDS, TM.HEADER_WORDS, TM.CTRL_WORDS, TM.SCRATCH_WORDS) == (8, 8, 8, 8)
    assert lay["record"] == {"ticket": TM.W_TICKET, "due": TM.W_DUE, "row_delay": TM.W_ROW_DELAY,
                             "actor_method": TM.W_ACTOR_METHOD, "a0": TM.W_A0, "a1": TM.W_A1, "a2": TM.W_A2,
                             "tag": TM.W_TAG}
    assert lay["header"] == {"t0": TM.D_T0, "base": TM.D_BASE, "n": TM.D_N, "max_delay": TM.D_MAX_DELAY,
                             "seq": TM.D_SEQ}
    assert lay["control"] == {"now": TM.C_NOW, "head": TM.C_HEAD, "tail": TM.C_TAIL, "runs_head": TM.C_RUNS_HEAD,
                              "runs_tail": TM.C_RUNS_TAIL, "refused": TM.C_REFUSED, "delivered": TM.C_DELIVERED,
                              "torn": TM.C_TORN}
    assert lay["scratch"] == {"k": TM.S_K, "refused": TM.S_REFUSED, "max_delay": TM.S_MAX_DELAY, "head": TM.S_HEAD,
                              "runs_head": TM.S_RUNS_HEAD, "now": TM.S_NOW, "n_due": TM.S_DUE, "segs": TM.S_SEGS}
    assert (lay["min_entries"], lay["max_entries"], lay["min_horizon"], lay["max_horizon"], lay["min_runs"],
            lay["max_runs"]) == (TM.MIN_ENTRIES, TM.MAX_ENTRIES, TM.MIN_HORIZON, TM.MAX_HORIZON, TM.MIN_RUNS,
                                 TM.MAX_RUNS)
    for name in ("record", "control", "scratch"):
        assert sorted(lay[name].values()) == list(range(8))
    for H in (16, 256, 1024):
        assert hip().timer_desc_words(H) == TM.desc_words(H)


VARIANTS = [dict(a1=True, a2=True, method="col"), dict(a1=False, a2=True, method=7), dict(a1=True, a2=False, method="col"),
            dict(a1=False, a2=False, method=0xFFFF)]
SWEEP = [(M, H, E) for E in (64, 16384) for H in (16, 1024) for M in (0, 1, 63, 64, 65, T - 1, T, T + 1, BIG)
         if M <= E or (M, H, E) == (65, 16, 64)]


@pytest.mark.parametrize("M,H,E", SWEEP)
def test_schedule_and_tick_equal_the_model(M, H, E):
    """A Schedule with delays from the whole horizon and the refused values, one with short
    delays behind it, three ticks: every word after every call."""
    gpu, ref = pair(E, H)
    v = VARIANTS[SWEEP.index((M, H, E)) % 4]
    if M > E:  # the one case that must raise: 65 valid delays into 64 slots
        b, d = random_call(M, 5, H, delays="valid", **v)
        assert both_schedule(gpu, ref, b, d) is None and not ref.ring.any() and not ref.ctrl.any() and gpu.full == 1
        return
    b, d = random_call(M, M + H, H, **v)
    s = both_schedule(gpu, ref, b, d, tag=-5)
    assert s is not None and s.n + s.refused == M and (M < 8 or (s.n and s.refused))
    b2, d2 = random_call(min(M, E - s.n), M + H + 1, H, delays="short", **VARIANTS[(SWEEP.index((M, H, E)) + 1) % 4])
    assert both_schedule(gpu, ref, b2, d2, tag=6) is not None
    due = [both_tick(gpu, ref) for _ in range(3)]
    assert sum(due) >= b2.M and ref.read()["delivered"] == sum(due)


def stability_cases(M, H):
    one = torch.full((M,), 3, dtype=torch.int32)
    yield "one delay", one
    yield "two delays alternating", torch.where(torch.arange(M) % 2 == 0, 5, 2).to(torch.int32)
    yield "pairs alternating", torch.where(torch.arange(M) // 2 % 2 == 0, H, 1).to(torch.int32)
    for pos in (0, 63, 64, 255, 256, 1023, 1024, 4095, 4096, M - 1):
        d = one.clone()
        d[pos] = 2
        yield f"one odd row at {pos}", d
        d = one.clone()
        d[pos] = 0
        yield f"one refused row at {pos}", d


def test_the_sort_is_stable_across_every_group_wave_and_tile_edge():
    H = 16
    b, _ = random_call(BIG, 3, H)
    bg = _cuda(b)
    gpu, ref = pair(16384, H)
    for name, d in stability_cases(BIG, H):
        s = both_schedule(gpu, ref, b, d, bg=bg)
        assert s is not None, name
        for _ in range(H):  # (drains the queue: the next case finds room)
            ref.tick()
            gpu.tick()
        same_words(ref, gpu)
    assert ref.read()["head"] > 2 * 16384  # (the ring wrapped on the way)


@pytest.mark.parametrize("H", [16, 1024])
def test_all_delays_distinct_and_a_uniform_delay(H):
    gpu, ref = pair(16384, H)
    b, _ = random_call(H, 1, H)
    assert both_schedule(gpu, ref, b, (torch.randperm(H) + 1).to(torch.int32)).n == H
    big, _ = random_call(T + 65, 2, H, a2=False, method=9)
    for delay, n in ((H, T + 65), (1, T + 65), (0, 0), (H + 1, 0), (-1, 0), (2**31 - 1, 0)):
        s = both_schedule(gpu, ref, big, delay)
        assert s is not None and s.n == n, delay
        both_tick(gpu, ref)
    empty, _ = random_call(0, 3, H)
    assert both_schedule(gpu, ref, empty, 1).n == 0 and both_schedule(gpu, ref, empty, torch.zeros(0, dtype=torch.int32)).n == 0
    # the distinct run is live and holds the two uniform ones behind it; the K = 0 calls filed none
    assert ref.read()["runs"] == 3 and ref.read()["refused"] == 4 * (T + 65)


def test_a_delay_column_that_is_a_view_at_an_odd_offset():
    H, M = 16, T + 7
    gpu, ref = pair(16384, H)
    b, d = random_call(M, 4, H)
    buf = torch.zeros(M + 3, dtype=torch.int32, device="cuda")
    for off in (1, 2, 3):
        buf[off:off + M] = d.cuda()
        view = buf[off:off + M]
        assert view.data_ptr() % 16 != 0
        assert both_schedule(gpu, ref, b, d, dg=view) is not None
    assert both_tick(gpu, ref) > 0


def test_a_run_that_straddles_the_wrap_and_a_full_run_table():
    H = 16
    gpu, ref = pair(64, H, runs=4)
    b, d = random_call(40, 6, H, delays="short")
    assert both_schedule(gpu, ref, b, 1).n == 40
    assert both_tick(gpu, ref) == 40 and ref.read()["tail"] == 40
    s = both_schedule(gpu, ref, b, d)  # tickets 40 .. 79: slots 40 .. 63, then 0 .. 15
    assert s.first_ticket == 40 and s.n == 40 and ref.ring[0, TM.W_TICKET] == 65
    assert [both_tick(gpu, ref) for _ in range(3)] == [int((d == k).sum()) for k in (1, 2, 3)]
    one, _ = random_call(1, 7, H)
    for k in range(4):
        assert both_schedule(gpu, ref, one, 2 + k) is not None
    assert both_schedule(gpu, ref, one, 1) is None and gpu.full == 1  # R runs, then one more
    assert both_schedule(gpu, ref, one, 0).refused == 1                # (no accepted row needs no descriptor)
    assert both_tick(gpu, ref) == 0 and both_tick(gpu, ref) == 1
    assert both_schedule(gpu, ref, one, 1) is not None


def test_ticks_over_many_runs():
    """Nothing due, one run due, then 64 runs whose segments are 0 to 9 records long -- their
    boundaries fall inside quads of lanes, at wave and at block edges of the take's output --
    and a finished run behind a live tail run."""
    H, R_ = 16, 64
    gpu, ref = pair(16384, H, runs=R_)
    assert both_tick(gpu, ref) == 0
    b, d = random_call(300, 8, H, delays="short")
    both_schedule(gpu, ref, b, d)
    assert both_tick(gpu, ref) == int((d == 1).sum())
    for k in range(R_ - 1):
        M = (7 * k) % 28
        bk, dk = random_call(M, 100 + k, H, delays="short", a1=bool(k & 1))
        both_schedule(gpu, ref, bk, dk, tag=k)  # (0, 7, 14 or 21 rows: every fourth call files no run)
    assert ref.read()["runs"] == 1 + 47
    due = [both_tick(gpu, ref) for _ in range(3)]
    # (16 * 7 + 16 * 14 + 15 * 21 = 651 rows over three delays, and the first run's delays 2 and 3)
    assert min(due) > 0 and max(due) > 256 and sum(due) == 300 - int((d == 1).sum()) + 651
    assert ref.read()["runs"] == 0
    # a long run at the tail, a short one behind it
    both_schedule(gpu, ref, b, H)
    both_schedule(gpu, ref, b, 1)
    assert both_tick(gpu, ref) == 300 and ref.read()["runs"] == 2 and ref.read()["live"] == 300
    assert [both_tick(gpu, ref) for _ in range(H - 1)][-1] == 300 and ref.read()["runs"] == 0
    assert ref.read()["torn"] == 0 and ref.read()["tail"] == ref.read()["head"]
    assert gpu.peek() == ref.peek() == 0
    both_schedule(gpu, ref, b, 1)
    assert gpu.peek() == ref.peek() == 300 and gpu.read()["now"] == ref.read()["now"]
    same_words(ref, gpu)


# ---------------------------------------------------------------- world 1 on the GPU
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_schedule_and_tick_world1_gpu(delivery):
    rt = gpu_runtime(delivery, timers=True, timer_entries=64, timer_horizon=16, timer_runs=4)
    try:
        schedule_and_tick_scenario(rt, "cuda")
    finally:
        rt.close()
    rt = gpu_runtime(delivery, timers=True)
    try:
        bad_keywords_scenario(rt, "cuda")
    finally:
        rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_tick_with_retries_dead_letters_and_back_off_world1_gpu(delivery):
    rt = gpu_runtime(delivery, timers=True, dead_letters=True)
    try:
        retries_and_dead_letters_scenario(rt, "cuda")
    finally:
        rt.close()
    rt = gpu_runtime(delivery, timers=True, timer_horizon=16, dead_letters=True)
    try:
        backoff_scenario(rt, "cuda")
    finally:
        rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_an_ordered_method_folds_in_ticket_order_gpu(delivery):
    """``SeqFold`` messages to two actors, scheduled by two calls for the same tick: every
    actor ran each exactly once, one at a time, and with mailbox delivery in ticket order."""
    rt = gpu_runtime(delivery, timers=True)
    try:
        fold = (lambda actors, vals: MsgBatch(torch.tensor(actors, dtype=torch.int32).cuda(), torch.tensor(vals).cuda(),
                                              None, None, METHOD_SEQ_FOLD))
        rt.schedule(fold([7, 3, 7, 7, 3], [11, 12, 13, 14, 15]), torch.tensor([2, 2, 1, 2, 2], dtype=torch.int32).cuda())
        assert rt.tick("calculator").due.a0.tolist() == [13]
        before = rt.state.cpu().clone()
        rt.schedule(fold([3, 7, 7], [16, 17, 18]), 1)
        t = rt.tick("calculator")
        assert t.due.ticket.tolist() == [1, 2, 3, 4, 5, 6, 7] and t.due.a0.tolist() == [11, 12, 14, 15, 16, 17, 18]
        torch.cuda.synchronize()
        ok, order = audit_fold(t.due.actor.cpu().numpy(), t.due.a0.cpu().numpy(), t.value.cpu().numpy(),
                               t.status.cpu().numpy(), before.numpy(), rt.state.cpu().numpy())
        assert ok, order  # every message ran exactly once, one at a time per actor
        if delivery == "mailbox":  # (the direct path's updates are linearizable, not FIFO per actor)
            assert order == {7: [0, 2, 5, 6], 3: [1, 3, 4]}
    finally:
        rt.close()


def test_tick_with_the_breaker_and_the_limiter_gpu():
    rt = gpu_runtime(timers=True, breaker_threshold=1, limit_burst=2)
    try:
        b = MsgBatch(torch.tensor([3, 3, 3, 4], dtype=torch.int32).cuda(), torch.tensor([9, 9, 9, 1]).cuda(), None, None,
                     METHOD_RETRY_TEST)
        want = ([STATUS_FAILED, STATUS_FAILED, STATUS_THROTTLED, 0], [STATUS_FAILED] * 3 + [0],
                [STATUS_BREAKER_OPEN] * 3 + [0])
        for kw, st in zip(({"limit": True}, {"breaker": True}, {"breaker": True}), want):
            rt.schedule(b, 1)
            t = rt.tick("calculator", **kw)
            assert t.status.tolist() == st and t.due.row.tolist() == [0, 1, 2, 3]
        assert rt.timers()["delivered"] == 12 and rt.stats()["breaker"]["rejected"] == 3
    finally:
        rt.close()


def test_a_tick_larger_than_one_send_goes_in_slices_gpu():
    from ptype_amd.runtime import DeviceRuntime

    rt = DeviceRuntime(torch.device("cuda", 0), actors=64, service="calculator", shm=False, max_batch=100, timers=True)
    rt.place_local()
    try:
        cap = rt.exchange.max_chunk * rt.exchange.chunks
        M = 2 * cap + 37
        actor = torch.arange(M, dtype=torch.int32) % 64
        b = MsgBatch(actor.cuda(), torch.ones(M, dtype=torch.int64).cuda(), None, None, METHOD_COUNTER_ADD)
        rt.schedule(b, 1)
        sizes, send = [], rt.send
        rt.send = lambda service, batch, **kw: (sizes.append(batch.M), send(service, batch, **kw))[1]
        t = rt.tick("calculator")
        assert sizes == [cap, cap, 37] and t.n == M and t.status.tolist() == [0] * M
        assert t.due.row.tolist() == list(range(M))
        # Counter.Add(+1) replies the counter it left.  The method is not ordered: inside one Send an
        # actor's messages run in any order, so per actor and slice the replies are compared as a set,
        # and a later slice continues where the earlier ones ended: the slices went in ticket order
        value, state = t.value.tolist(), [0] * 64
        for lo in range(0, M, cap):
            rows = range(lo, min(lo + cap, M))
            for x in range(64):
                got = sorted(value[i] for i in rows if i % 64 == x)
                assert got == list(range(state[x] + 1, state[x] + 1 + len(got))), (lo, x)
                state[x] += len(got)
        torch.cuda.synchronize()
        assert rt.state.cpu().tolist() == state == torch.bincount(actor, minlength=64).tolist()
    finally:
        rt.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_timers_multirank_fakecomm():
    """Two in-process ranks, each with a queue of its own.  At the first tick only rank 0 has
    something due and rank 1 joins the collective Send with an empty batch; at the second both
    send what they scheduled, whichever rank runs the messages.  The ranks drive ``TimerQueue.tick``
    and ``ActorExchange.send_all`` themselves, as ``DeviceRuntime.tick`` does at world > 1; the
    runtime's own world > 1 branch (an in-process runtime has no FakeComm group) is run by no test."""
    R_, n, H = 2, 6000, 16
    fc = hip().FakeComm(R_)
    calls = []
    for r in range(R_):
        g = torch.Generator().manual_seed(50 + r)
        M = T + 65 + 100 * r
        b = MsgBatch(torch.randint(0, n + 500, (M,), generator=g).to(torch.int32),
                     torch.randint(-30000, 30000, (M,), generator=g), torch.randint(-30000, 30000, (M,), generator=g),
                     None, METHOD_CALC_MULTIPLY)
        d = torch.randint(1 if r == 0 else 2, 3, (M,), generator=g).to(torch.int32)
        calls.append((b, d))
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
                ex = ActorExchange(tab, T + 200, chunks=1, state=st, fake=(fc, r), delivery="direct")
                q = TM.TimerQueue("cuda", 16384, H, 4)
                q.schedule(_cuda(calls[r][0]), calls[r][1].cuda(), tag=r + 1)
                start.wait(timeout=60)
                out = []
                for _ in range(2):
                    due = q.tick()
                    val, sts = ex.send_all(due.batch())
                    s.synchronize()
                    out.append((due.row.cpu(), due.actor.cpu(), due.tag.cpu(), val.cpu(), sts.cpu()))
                results[r] = (out, q.ring.cpu(), q.runs.cpu(), q.ctrl.cpu(), q.read())
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
        out, ring, runs, ctrl, rd = results[r]
        b, d = calls[r]
        ref = TM.TimerRef(16384, H, 4)
        ref.schedule(b, d, tag=r + 1)
        for k in range(2):
            want = ref.tick()
            row, actor, tag, val, sts = out[k]
            assert np.array_equal(row.numpy(), want["row"]) and np.array_equal(actor.numpy(), want["actor"]), (r, k)
            assert tag.tolist() == [r + 1] * want["n"]
            rows = torch.from_numpy(want["row"].astype(np.int64))
            missing = b.actor[rows] >= n
            assert torch.equal(sts, torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), (r, k)
            assert torch.equal(val, torch.where(missing, 0, b.a0[rows] * b.a1[rows])), (r, k)
        assert np.array_equal(ring.numpy().view(np.uint64), ref.ring), r
        assert np.array_equal(runs.numpy().view(np.uint64), ref.runs), r
        assert np.array_equal(ctrl.numpy().view(np.uint64), ref.ctrl), r
        assert rd["delivered"] == b.M and rd["live"] == 0 and rd["torn"] == 0
    assert results[1][0][0][0].numel() == 0 and results[0][0][0][0].numel() > 0  # rank 1's first tick was empty


# ---------------------------------------------------------------- Client.Schedule / Tick through Join
def test_client_schedule_tick_and_timers_through_join_gpu(tmp_path, ports, monkeypatch):
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
    cfg.gpu.timers, cfg.gpu.timer_entries, cfg.gpu.timer_horizon, cfg.gpu.timer_runs = True, 128, 32, 8
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        rt = c.runtime
        assert (rt._timers.entries, rt._timers.horizon, rt._timers.n_runs) == (128, 32, 8) and rt._timers.ref is None
        client = c.NewClient("calculator", C.ConnConfig())
        schedule_and_tick_scenario(rt, "cuda", tick=client.Tick, schedule=client.Schedule, tag=fnv1a64("calculator"))
        assert client.Timers() == c.Stats()["runtime"]["timers"] and client.Timers()["horizon"] == 32
        assert [t.n for t in client.Tick(ticks=2)] == [0, 0] and client.Timers()["now"] == 5
        client.Close()
    finally:
        server.Close()
        c.Close()
