"""The circuit breaker on a real MI355X: the probe, admit, observe, step and clear
kernels (csrc/hip/breaker.hip) against the numpy model (``ops.breaker.BreakerRef``), the
state words and counters compared after every Send, and ``breaker=True`` through world-1
runtimes, in-process multi-rank FakeComm exchanges and ``Client.Send``.  All comparisons
are exact integer equality."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import breaker as BR
from ptype_amd.ops import hip
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.gather import Gather
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_RETRY_TEST, STATUS_BREAKER_OPEN,
                                   STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NO_METHOD, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_breaker import SCRIPT, breaker_scenario, ids_batch, run_script
from test_coalesce import runtime as cpu_runtime
from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime

pytestmark = pytest.mark.gpu

T = 2048  # messages per tile of the streaming kernels (checked below against the module)
REJ = STATUS_BREAKER_OPEN


def pair(n, **kw):
    return BR.Breaker("cuda", actors=n, **kw), BR.BreakerRef(actors=n, **kw)


def both(gpu, ref, actor, status_of, bg=None, pad_status=False):
    """One guarded Send of ``ids_batch(actor)`` through the kernels and the model; the inner
    Send answers ``(row, status_of(sub))``.  Everything is compared; returns the statuses."""
    b = ids_batch(actor)
    rval, rst = ref.send(b, lambda sub: (sub.a0.clone(), status_of(sub).to(torch.int32)))[:2]

    def inner(sub):
        cpu = MsgBatch(sub.actor.cpu(), sub.a0.cpu(), None, None, sub.method)
        st = status_of(cpu).to(torch.int32)
        if pad_status:  # the statuses as a view at an odd element offset
            st = torch.cat([st[:1], st]).cuda()[1:]
        return sub.a0.clone(), st.cuda()

    val, st = gpu.send(_cuda(b) if bg is None else bg, inner)[:2]
    assert st.is_cuda and torch.equal(st.cpu(), rst) and torch.equal(val.cpu(), rval)
    assert np.array_equal(gpu.words(), ref.words())
    assert gpu.counters == ref.counters and gpu.tick == ref.tick
    assert int(gpu.ctr[BR.C_TOUCHED]) == 0 and not bool(gpu.obs.any())
    return rst


def fails(*bad, status=STATUS_FAILED):
    return lambda sub: torch.where(torch.isin(sub.actor, torch.tensor(bad, dtype=torch.int32)), status, STATUS_OK)


# ---------------------------------------------------------------- the kernels
def test_constants_match_the_header():
    lim = hip().breaker_limits()
    assert hip().breaker_tile() == T
    assert (lim["pending"], lim["status"], lim["max_tick"], lim["max_actors"]) == (BR.PENDING, REJ, BR.MAX_TICK,
                                                                                  BR.MAX_ACTORS)
    assert lim["ctr_words"] == BR.CTR_WORDS
    assert lim["counters"] == ("n_open", "n_dirty", "trips", "closes", "oob", "n_touched")
    assert (BR.C_OPEN, BR.C_DIRTY, BR.C_TRIPS, BR.C_CLOSES, BR.C_OOB, BR.C_TOUCHED) == tuple(range(6))


@pytest.mark.parametrize("n", [16, 4096])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_the_script_against_the_reference(M, n):
    """Nine guarded Sends whose replies are a function of (actor, a0, tick): trips, counts
    reset by an OK, failed and successful probes, rejections, ids outside the table
    (test_breaker.py asserts that the model reaches each of them)."""
    gpu, ref = pair(n, **SCRIPT)
    assert np.array_equal(gpu.words(), ref.words())  # the clear kernel
    seen = run_script(ref, M, also=gpu, to_device=_cuda)
    if M >= 63:
        assert all(v > 0 for v in seen.values()), seen
    assert gpu.read() == ref.read()


def test_all_messages_to_one_actor():
    M = 3 * T + 17
    gpu, ref = pair(16, threshold=M + 5, cooldown=2)
    one = [7] * M
    both(gpu, ref, one, fails(7))  # every wave adds its 256 rows once: fails = M
    assert int(ref.words()[7]) == M
    both(gpu, ref, one, lambda sub: torch.where(sub.a0 == M - 1, STATUS_OK, STATUS_FAILED))  # one OK row: reset
    assert int(ref.words()[7]) == 0
    both(gpu, ref, one, fails(7))
    st = both(gpu, ref, one, fails(7))  # 2 M >= threshold: trips
    assert ref.read()["open"] == 1
    assert bool((both(gpu, ref, one, fails(7)) == REJ).all())  # K == 0
    st = both(gpu, ref, one, fails())  # half-open: row 0 probes, every other row is rejected
    assert st.tolist() == [STATUS_OK] + [REJ] * (M - 1) and ref.read() == {"open": 0, "dirty": 0, "trips": 1,
                                                                            "closes": 1, "oob": 0}
    assert bool((both(gpu, ref, one, fails()) == STATUS_OK).all())


def test_runs_across_wave_and_block_edges():
    """Runs of equal failing ids that start in one wave (256 rows) or tile and end in the
    next, runs inside one thread's four rows, and single rows: every count is exact."""
    M = 2 * T + 300
    ids = torch.arange(M) % 5 + 8  # healthy filler
    for lo, hi, a in ((250, 262, 1), (T - 3, T + 6, 2), (T + 256 * 3 - 1, T + 256 * 3 + 1, 3), (0, 3, 4), (5, 6, 5),
                      (M - 2, M, 6), (1021, 1029, 1), (2 * T - 1, 2 * T + 1, 2)):
        ids[lo:hi] = a
    gpu, ref = pair(16, threshold=10**6, cooldown=2)
    both(gpu, ref, ids, fails(1, 2, 3, 4, 5, 6))
    assert ref.words()[1:7].tolist() == [12 + 8, 9 + 2, 2, 3, 1, 2]
    both(gpu, ref, ids, lambda sub: torch.where(sub.actor < 8, torch.where(sub.a0 % 2 == 0, STATUS_FAILED, STATUS_NO_METHOD),
                                                STATUS_OK))
    both(gpu, ref, ids, fails(1, 3, 5))  # 2, 4, 6 get OK rows only: dirty actors reset


def test_two_probe_candidates_in_far_blocks():
    M = 3 * T + 17
    for rows in ((5, 3 * T + 2), (T + 7, 2 * T + 9)):  # block 0 and the last one; then blocks 1 and 2 only
        ids = torch.arange(M) % 4 + 8
        ids[list(rows)] = 3
        gpu, ref = pair(16, threshold=1, cooldown=1)
        both(gpu, ref, ids, fails(3))  # opens until 2
        st = both(gpu, ref, ids, fails(3))  # half-open: the lower row probes and fails
        assert st[list(rows)].tolist() == [STATUS_FAILED, REJ]
        flipped = ids.clone()
        flipped[rows[0]] = 8  # only the far candidate is left: it probes
        st = both(gpu, ref, flipped, fails())
        assert int(st[rows[1]]) == STATUS_OK and ref.read()["closes"] == 1


def test_ids_outside_the_table_and_negative_ids():
    M = T + 70
    ids = torch.arange(M) % 6
    ids[::7] = torch.tensor([16, -1, -2**31, 2**31 - 1, 1000])[torch.arange(len(ids[::7])) % 5]
    gpu, ref = pair(16, threshold=1, cooldown=3)
    every = (lambda sub: torch.full((sub.M,), STATUS_NO_ACTOR))
    both(gpu, ref, ids, every)
    for _ in range(3):
        st = both(gpu, ref, ids, every)
    out = ~((ids >= 0) & (ids < 16))
    assert bool((st[out] == STATUS_NO_ACTOR).all()) and ref.read()["oob"] == 3 * int(out.sum())
    assert ref.read()["open"] == 6


def test_unaligned_column_views():
    M = T + 9
    gpu, ref = pair(64, threshold=2, cooldown=1)
    g = torch.Generator().manual_seed(5)
    for send in range(5):
        ids = torch.randint(0, 40, (M + 1,), generator=g).to(torch.int32)
        full = MsgBatch(ids.cuda(), torch.arange(-1, M, dtype=torch.int64).cuda(), None, None, METHOD_RETRY_TEST)
        view = MsgBatch(full.actor[1:], full.a0[1:], None, None, METHOD_RETRY_TEST)  # odd element offsets
        assert view.actor.data_ptr() % 16 == 4
        both(gpu, ref, ids[1:], fails(*range(0, 40, 3)), bg=view, pad_status=True)
    assert ref.read()["trips"] > 0 and ref.counters["rejected"] > 0


def test_nothing_admitted_and_nothing_rejected():
    M = T + 1
    gpu, ref = pair(16, threshold=1, cooldown=4)
    both(gpu, ref, [1, 2, 3], fails(1, 2, 3))
    calls = []
    sent = gpu.counters["sent"]
    st = both(gpu, ref, torch.arange(M) % 3 + 1, fails())  # K == 0: the inner Send is skipped
    assert bool((st == REJ).all()) and gpu.counters["sent"] == sent
    st = both(gpu, ref, torch.arange(M) % 3 + 4, fails(5))  # something is open, nothing of it addressed: K == M
    assert gpu.counters["sent"] == sent + M and ref.read()["open"] == 4

    def inner(sub):
        calls.append(sub.M)
        return sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32, device="cuda")

    val, st = gpu.send(_cuda(ids_batch([1, 2, 1])), inner, collective=True)  # a rank of a group: an empty Send
    assert calls == [0] and st.tolist() == [REJ] * 3 and val.tolist() == [0] * 3


def test_tick_restart_and_reset():
    last = BR.MAX_TICK
    gpu, ref = pair(16, threshold=1, cooldown=7, _start=last - 1)
    ids = torch.arange(T + 5) % 4
    both(gpu, ref, ids, fails(1))
    assert int(ref.words()[1]) == (1 << 63) | last << 32 | int((ids == 1).sum())
    both(gpu, ref, ids, fails(1))  # the last tick: the lowest row to 1 probes
    st = both(gpu, ref, ids, fails())  # the restart: everything closes first
    assert bool((st == STATUS_OK).all()) and gpu.tick == 2 and ref.read()["open"] == 0
    both(gpu, ref, ids, fails(1, 2))
    st = both(gpu, ref, ids, fails())  # tick 3 < until: no claim of the ticks before the restart passes
    assert int((st == REJ).sum()) == int(((ids == 1) | (ids == 2)).sum())
    gpu.reset()
    ref.reset()
    assert np.array_equal(gpu.words(), ref.words()) and ref.read()["open"] == 0 and ref.read()["trips"] == 3
    assert bool((both(gpu, ref, ids, fails()) == STATUS_OK).all())


# ---------------------------------------------------------------- world 1 on the GPU
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_trips_rejects_and_probes_gpu(delivery):
    rt = gpu_runtime(delivery, breaker_threshold=2, breaker_cooldown=3)
    try:
        plain = rt.send("calculator", _cuda(ids_batch([1, 2], METHOD_ECHO)))
        assert rt._breaker is None and plain[1].tolist() == [STATUS_OK] * 2  # a Send without the option creates nothing
        breaker_scenario(rt, dev="cuda")
        rt.exchange._capturing = True  # as inside ActorExchange.capture
        try:
            with pytest.raises(ValueError, match="captur"):
                rt.send("calculator", _cuda(ids_batch([1])), breaker=True)
        finally:
            rt.exchange._capturing = False
    finally:
        rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_breaker_with_every_wrapper_equals_the_cpu_runtime_gpu(delivery):
    """retries + coalesce + cache + ledger + gather around the breaker, RPCRetryTest rows
    (actor a passes at its 4 (a % 7)-th call; ids 64..71 are not registered and trip) between
    duplicated Multiply rows: every Send equals the CPU runtime's, and so do the counters."""
    M = 4000
    g = torch.Generator().manual_seed(31)
    actor = torch.randint(0, 80, (M,), generator=g).to(torch.int32)
    col = torch.full((M,), METHOD_CALC_MULTIPLY, dtype=torch.int16)
    a0 = torch.randint(0, 4, (M,), generator=g)
    where = torch.randperm(M, generator=g)[:64]
    col[where], actor[where] = METHOD_RETRY_TEST, torch.arange(64, dtype=torch.int32)
    a0[where] = torch.arange(64) % 7 * 4
    a0 = torch.where(actor >= 64, torch.arange(M), a0)  # (keys of their own: no follower inherits a probe's reply)
    b = MsgBatch(actor, a0, torch.randint(0, 4, (M,), generator=g), None, col)
    kw = {"ledger": True, "breaker_threshold": 2, "breaker_cooldown": 2, "breaker_actors": 72}
    rt, rt_cpu = gpu_runtime(delivery, **kw), cpu_runtime(**kw)
    grp = (actor % 16).to(torch.int32)
    gg, gc = Gather(grp.cuda(), 16, "sum"), Gather(grp, 16, "sum")
    opts = {"breaker": True, "coalesce": True, "cache": True, "retries": 2}
    try:
        bg = _cuda(b)
        for send in range(6):
            want = rt_cpu.send("calculator", b, gather=gc, **opts)
            val, st = rt.send("calculator", bg, gather=gg, **opts)
            assert torch.equal(st.cpu(), want[1]) and torch.equal(val.cpu(), want[0]), send
            assert torch.equal(gg.value.cpu(), gc.value) and torch.equal(gg.status.cpu(), gc.status)
            assert torch.equal(gg.n_ok.cpu(), gc.n_ok) and torch.equal(gg.bad_row.cpu(), gc.bad_row)
        assert np.array_equal(rt._breaker.words(), rt_cpu._breaker.words())
        n, want = rt.stats(), rt_cpu.stats()
        assert n["breaker"] == want["breaker"] and n["cache"] == want["cache"] and n["coalesce"] == want["coalesce"]
        for led in (n["ledger"], want["ledger"]):
            led.pop("hot")  # (the busiest actors: the order among equal loads is the reader's)
        assert n["ledger"] == want["ledger"] and torch.equal(rt.state.cpu(), rt_cpu.state)
        assert n["breaker"]["trips"] > 8 and n["breaker"]["closes"] > 0 and n["breaker"]["rejected"] > 0
        assert n["ledger"]["calls"]["Calculator.Multiply"]["other"] > 0
    finally:
        rt.close()
        rt_cpu.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
@pytest.mark.parametrize("R_", [2, 4])
def test_guarded_sends_multirank_fakecomm(R_):
    """Every rank guards batches of its own through ``DeviceRuntime.send(breaker=True)`` of
    a runtime that is given the rank's FakeComm exchange.  Rank 0's first batch goes to
    actors that never pass: they all trip, its second batch is rejected entirely and it
    joins the collective Send with an empty batch, its third is half rejected.  The other
    ranks' actors pass.  Every rank issues exactly one inner Send per guarded Send."""
    from ptype_amd.runtime import DeviceRuntime

    M, n, sends = 3000, 6000, 3
    fc = hip().FakeComm(R_)

    def batch(r, send):
        i = torch.arange(M)
        if r != 0:
            return MsgBatch(((i * 7 + r) % n).to(torch.int32), torch.zeros(M, dtype=torch.int64), None, None,
                            METHOD_RETRY_TEST)  # passes at once
        actor = (i % 100).to(torch.int32)  # 100 actors that never pass
        a0 = torch.full((M,), 10**9)
        if send == 2:  # every other row to actors that pass
            actor = torch.where(i % 2 == 0, actor, (1000 + i).to(torch.int32))
            a0 = torch.where(i % 2 == 0, a0, 0)
        return MsgBatch(actor, a0, None, None, METHOD_RETRY_TEST)

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
                                   max_batch=M, breaker_threshold=1, breaker_cooldown=9)
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
                        val, sts = rt.send("calculator", _cuda(batch(r, k)), breaker=True)[:2]
                        out.append((val.cpu(), sts.cpu()))
                    s.synchronize()
                    results[r], inner[r] = out, calls
                    counters[r] = rt.stats()["breaker"]
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
    even = torch.arange(M) % 2 == 0
    for r in range(R_):
        sts = [x[1] for x in results[r]]
        if r == 0:
            assert bool((sts[0] == STATUS_FAILED).all()) and bool((sts[1] == REJ).all())
            assert bool((sts[2][even] == REJ).all()) and bool((sts[2][~even] == STATUS_OK).all())
            assert bool((results[0][1][0] == 0).all())
            assert inner[0] == [M, 0, M // 2]  # the second one carried nothing, and still joined
            assert counters[0] == {"sends": 3, "messages": 3 * M, "rejected": M + M // 2, "sent": M + M // 2,
                                   "open": 100, "trips": 100, "closes": 0, "oob": 0, "actors": n, "threshold": 1,
                                   "cooldown": 9}
        else:
            assert all(bool((x == STATUS_OK).all()) for x in sts) and inner[r] == [M] * 3
            assert counters[r]["rejected"] == 0 and counters[r]["sent"] == 3 * M and counters[r]["open"] == 0


# ---------------------------------------------------------------- Client.Send through Join
@pytest.mark.parametrize("default", [False, True])
def test_client_send_breaker_through_join_gpu(tmp_path, ports, monkeypatch, default):
    """``Client.Send(batch, breaker=True)`` with ``gpu.breaker`` unset (direct delivery), and
    ``gpu.breaker: true`` with no argument (mailbox delivery)."""
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
    cfg.gpu.breaker_threshold, cfg.gpu.breaker_cooldown = 2, 3
    if default:
        cfg.gpu.breaker = True
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        rt = c.runtime
        assert rt.breaker is default
        client = c.NewClient("calculator", C.ConnConfig())
        if not default:
            client.Send(_cuda(ids_batch([1, 2], METHOD_ECHO)))
            assert rt._breaker is None and c.Stats()["runtime"]["breaker"]["sends"] == 0
        breaker_scenario(rt, dev="cuda", send=(lambda b: client.Send(b)) if default
                         else (lambda b: client.Send(b, breaker=True)))
        n = c.Stats()["runtime"]["breaker"]
        assert (n["sends"], n["rejected"], n["trips"], n["closes"], n["open"]) == (8, 10, 1, 1, 0)
        client.Send(_cuda(ids_batch([1])), breaker=False)
        assert c.Stats()["runtime"]["breaker"]["sends"] == 8
        client.Close()
    finally:
        server.Close()
        c.Close()
