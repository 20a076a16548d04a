"""Send retries on a real MI355X: the selection / merge kernels
(csrc/hip/retry.hip) against their torch reference, and ``retries=`` through the
world-1 exchange, in-process multi-rank FakeComm exchanges and ``Client.Send``.
All comparisons are exact integer equality."""
import threading

import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import hip
from ptype_amd.ops import retry as R
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_RETRY_TEST, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_send_retries import retry_scenario, world1

pytestmark = pytest.mark.gpu

T = 4096  # statuses per block of retry_select (checked below against the module)
PATTERNS = ("none", "all", "first", "last", "every7", "random1pct")


def _status(M, pattern, seed=0):
    """int32[M] statuses: STATUS_FAILED where ``pattern`` selects, other codes elsewhere."""
    g = torch.Generator().manual_seed(seed)
    other = torch.tensor([STATUS_OK, 1, 4, 5, 6, -1, 40], dtype=torch.int32)[torch.randint(0, 7, (M,), generator=g)]
    sel = torch.zeros(M, dtype=torch.bool)
    if pattern == "all":
        sel[:] = True
    elif pattern == "first" and M:
        sel[0] = True
    elif pattern == "last" and M:
        sel[-1] = True
    elif pattern == "every7":
        sel[::7] = True
    elif pattern == "random1pct":
        sel = torch.rand(M, generator=g) < 0.01
    return torch.where(sel, torch.full_like(other, STATUS_FAILED), other)


def _batch(M, a1, a2, mcol, seed=1):
    g = torch.Generator().manual_seed(seed)
    col = (lambda: torch.randint(-2**62, 2**62, (M,), generator=g))
    return MsgBatch(torch.randint(0, 2**31 - 1, (M,), generator=g).to(torch.int32), col(), col() if a1 else None,
                    col() if a2 else None,
                    torch.randint(0, 2**15, (M,), generator=g).to(torch.int16) if mcol else METHOD_RETRY_TEST)


def _check_select(b, status, retry_on):
    cuda = (lambda t: None if t is None else t.cuda())
    bg = MsgBatch(b.actor.cuda(), b.a0.cuda(), cuda(b.a1), cuda(b.a2),
                  b.method if isinstance(b.method, int) else b.method.cuda())
    sub, idx, K = R.select(bg, status.cuda(), retry_on)
    rsub, ridx, rK = R.select(b, status, retry_on)  # the torch reference (nonzero + index_select)
    assert K == rK and idx.dtype == torch.int32 and torch.equal(idx.cpu(), ridx)
    assert torch.equal(sub.actor.cpu(), rsub.actor) and torch.equal(sub.a0.cpu(), rsub.a0)
    for got, want in ((sub.a1, rsub.a1), (sub.a2, rsub.a2)):
        assert (got is None) == (want is None) and (want is None or torch.equal(got.cpu(), want))
    if isinstance(b.method, int):
        assert sub.method == b.method
    else:
        assert sub.method.dtype == torch.int16 and torch.equal(sub.method.cpu(), rsub.method)
    return K


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_retry_select_sizes_and_patterns(M):
    assert hip().retry_tile() == T == R.TILE
    b = _batch(M, True, True, True)
    for i, p in enumerate(PATTERNS):
        _check_select(b, _status(M, p, seed=i), (STATUS_FAILED,))


@pytest.mark.parametrize("a1,a2,mcol", [(False, False, False), (True, False, False), (False, True, True),
                                        (True, True, False)])
def test_retry_select_column_variants(a1, a2, mcol):
    M = 3 * T + 17
    K = _check_select(_batch(M, a1, a2, mcol), _status(M, "every7"), (STATUS_FAILED,))
    assert K == (M + 6) // 7


def test_retry_select_two_status_bits():
    M = 2 * T + 5
    g = torch.Generator().manual_seed(9)
    status = torch.randint(-1, 8, (M,), generator=g).to(torch.int32)
    K = _check_select(_batch(M, True, False, True), status, (STATUS_FAILED, STATUS_NO_ACTOR))
    assert K == int(((status == STATUS_FAILED) | (status == STATUS_NO_ACTOR)).sum())


def test_retry_select_more_tiles_than_summing_threads():
    """257 tiles + a partial one: the block that sums the tile counts below it (256
    threads) takes more than one value per thread."""
    M = 257 * T + 5
    b = _batch(M, False, False, False)
    for p in ("every7", "random1pct", "last"):
        _check_select(b, _status(M, p, seed=4), (STATUS_FAILED,))


def test_retry_select_unaligned_status_view():
    M = T + 9
    b = _batch(M, True, False, False)
    status = _status(M + 1, "every7")
    bg = MsgBatch(b.actor.cuda(), b.a0.cuda(), b.a1.cuda(), None, METHOD_RETRY_TEST)
    sub, idx, K = R.select(bg, status.cuda()[1:])  # 4 bytes past a 16-byte boundary
    assert torch.equal(idx.cpu().to(torch.int64), torch.nonzero(status[1:] == STATUS_FAILED).flatten())
    assert K == idx.numel() and torch.equal(sub.a0.cpu(), b.a0[idx.cpu().to(torch.int64)])


@pytest.mark.parametrize("M,K", [(1, 1), (1000, 0), (T + 1, 77), (300_001, 150_000)])
def test_retry_merge(M, K):
    g = torch.Generator().manual_seed(M)
    idx = torch.randperm(M, generator=g)[:K].sort().values
    val, st = torch.randint(-2**62, 2**62, (M,), generator=g), torch.randint(0, 7, (M,), generator=g).to(torch.int32)
    v2, s2 = torch.randint(-2**62, 2**62, (K,), generator=g), torch.randint(0, 7, (K,), generator=g).to(torch.int32)
    ev, es = val.clone(), st.clone()
    ev[idx], es[idx] = v2, s2
    gv, gs = val.cuda(), st.cuda()
    R.merge(gv, gs, idx.to(torch.int32).cuda(), v2.cuda(), s2.cuda())
    assert torch.equal(gv.cpu(), ev) and torch.equal(gs.cpu(), es)


# ---------------------------------------------------------------- world 1 on the GPU
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_send_all_retries_world1_gpu(delivery):
    M, n_c = 4096 + 65, 1000
    sc = retry_scenario(M, n_c, seed=11)
    ex, state = world1(M + n_c, M + n_c, device="cuda", delivery=delivery)
    req = MsgBatch(sc["actor"].cuda(), sc["a0"].cuda(), None, None, sc["method"].cuda())
    val, st = ex.send_all(req, retries=2)
    assert torch.equal(st.cpu(), sc["st"]) and torch.equal(val.cpu(), sc["val"])
    assert torch.equal(state.cpu(), sc["state"])  # RetryTest actors at min(a0, 3), every counter applied once
    s = ex.stats()
    assert s.retries == 2 and s.retried == sc["retried"]
    # the uniform-method scenario, and the same batch without retries
    sc = retry_scenario(M)
    for retries in (2, 0):
        ex, state = world1(M, M, device="cuda", delivery=delivery)
        val, st = ex.send_all(MsgBatch(sc["actor"].cuda(), sc["a0"].cuda(), None, None, METHOD_RETRY_TEST),
                              retries=retries)
        if retries:
            assert torch.equal(st.cpu(), sc["st"]) and torch.equal(val.cpu(), sc["val"])
            assert torch.equal(state.cpu(), sc["state"]) and ex.stats().retried == sc["retried"]
        else:
            assert torch.equal(st.cpu(), torch.where(sc["a0"] >= 2, STATUS_FAILED, STATUS_OK).to(torch.int32))
            assert bool((state == 1).all()) and ex.stats().retries == 0


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
@pytest.mark.parametrize("R_,delivery", [(2, "direct"), (2, "auto"), (4, "direct"), (4, "auto")])
def test_send_all_retries_multirank_fakecomm(R_, delivery):
    """Every rank but the last sends RetryTest + CounterAdd messages to its own
    disjoint set of actors spread over all ranks; the last sends only Multiply, so
    it has nothing to retry in any round and must still join each one."""
    Mr, Mc, Q = 4096 + 65, 1000, 6000  # sender r owns actor ids [r * Q, (r + 1) * Q): actor a lives on rank a % R_
    n = R_ * Q
    fc = hip().FakeComm(R_)
    scs = [retry_scenario(Mr, Mc, seed=20 + r) for r in range(R_ - 1)]
    batches = []
    for r, sc in enumerate(scs):
        batches.append((sc["actor"] + r * Q, sc["a0"], torch.zeros_like(sc["a0"]), sc["method"]))
    g = torch.Generator().manual_seed(77)
    M_mul = 3000
    batches.append((torch.randint(0, n, (M_mul,), generator=g).to(torch.int32),
                    torch.randint(-30000, 30000, (M_mul,), generator=g), torch.randint(-30000, 30000, (M_mul,), generator=g),
                    torch.full((M_mul,), METHOD_CALC_MULTIPLY, dtype=torch.int16)))
    results, states, stats, errors = [None] * R_, [None] * R_, [None] * R_, []
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
                ex = ActorExchange(tab, Mr + Mc, chunks=1, state=st, fake=(fc, r), delivery=delivery)
                actor, a0, a1, m = batches[r]
                req = MsgBatch(actor.cuda(), a0.cuda(), a1.cuda(), None, m.cuda())
                start.wait(timeout=60)
                val, sts = ex.send_all(req, retries=2)
                s.synchronize()
                results[r] = (val.cpu(), sts.cpu())
                states[r] = st.cpu()
                stats[r] = ex.stats()
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
    expect_state = torch.zeros(n, dtype=torch.int64)  # by actor id
    for r, sc in enumerate(scs):
        val, sts = results[r]
        assert torch.equal(sts, sc["st"]) and torch.equal(val, sc["val"]), r
        expect_state[r * Q: r * Q + Mr + Mc] = sc["state"]
        assert stats[r].retried == sc["retried"], r
    actor, a0, a1, _ = batches[-1]
    val, sts = results[-1]
    assert bool((sts == STATUS_OK).all()) and torch.equal(val, a0 * a1)
    assert stats[-1].retried == 0
    for r in range(R_):
        assert stats[r].retries == 2, (r, stats[r].retries)
        assert torch.equal(states[r], expect_state[r::R_]), r


# ---------------------------------------------------------------- Client.Send through Join
def test_client_send_retries_through_join_gpu(tmp_path, ports, monkeypatch):
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
    cfg.gpu.device, cfg.gpu.actors, cfg.gpu.max_batch = 0, 4096 + 65, 1 << 16
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        rt = c.runtime
        M = rt.total_actors
        sc = retry_scenario(M)
        client = c.NewClient("calculator", C.ConnConfig(retries=2))
        b = MsgBatch(sc["actor"].cuda(), sc["a0"].cuda(), None, None, METHOD_RETRY_TEST)
        val, st = client.Send(b, retries=client.cfg.retries)
        assert torch.equal(st.cpu(), sc["st"]) and torch.equal(val.cpu(), sc["val"])
        assert torch.equal(rt.state.cpu(), sc["state"])
        ex = c.Stats()["runtime"]["exchange"]
        assert ex["retries"] == 2 and ex["retried"] == sc["retried"]
        rt.state.zero_()
        val, st = client.Send(b)  # no retries: one attempt
        assert torch.equal(st.cpu(), torch.where(sc["a0"] >= 2, STATUS_FAILED, STATUS_OK).to(torch.int32))
        assert c.Stats()["runtime"]["exchange"]["retries"] == 2
        client.Close()
    finally:
        server.Close()
        c.Close()
