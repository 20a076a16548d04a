"""The dead-letter queue on a real MI355X: the count, append and take kernels
(csrc/hip/dead_letters.hip) against the numpy model (``ops.dead_letters.DeadLetterRef``),
the ring and the control line compared word for word after every Send, and
``dead_letter=True`` through world-1 runtimes, a captured SendGraph, in-process FakeComm
ranks and ``Client.Send`` / ``Client.DeadLetters`` / ``Client.Redrive``.  All comparisons are
exact integer equality."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import dead_letters as DL
from ptype_amd.ops import hip
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.gather import Gather
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_dead_letters import (breaker_and_limiter_scenario, dead_letter_scenario, followers_scenario, ks_of,
                               letters_of, mixed_batch, named_mask, no_queue_scenario, random_send,
                               redrive_alone_scenario, retries_scenario, run_sequence, same_words)
from test_send_retries import world1

pytestmark = pytest.mark.gpu

T = 4096  # rows per block (checked below against the module)
BIG = 3 * T + 17


def pair(entries, mask=None):
    return DL.DeadLetters("cuda", entries, mask), DL.DeadLetterRef(entries, mask)


def both(gpu, ref, b, st, att=None, tag=0, bg=None, stg=None, attg=None):
    """One Send filed by the kernels and by the model; every word compared."""
    ref.append(b, st, att, tag)
    gpu.append(_cuda(b) if bg is None else bg, st.cuda() if stg is None else stg,
               (None if att is None else att.cuda()) if attg is None else attg, tag)
    same_words(ref, gpu)


def same_letters(got, want):
    assert (got.n, got.ticket, got.torn) == (want["n"], want["ticket"], want["torn"]) and want["torn"] == 0
    for c in DL.COLUMNS:
        t = getattr(got, c)
        assert t.is_cuda and t.dtype == DL._DTYPES[c] and np.array_equal(t.cpu().numpy(), want[c]), c


# ---------------------------------------------------------------- the kernels
def test_layout_matches_the_header():
    lay = hip().dead_letter_layout()
    assert lay["tile"] == T == DL.TILE == hip().retry_tile()
    assert (lay["record_words"], lay["control_words"]) == (DL.RECORD_WORDS, DL.CTRL_WORDS) == (8, 8)
    assert lay["record"] == {"ticket": DL.W_TICKET, "seq": DL.W_SEQ, "row_status": DL.W_ROW_STATUS,
                             "actor_method_attempts": DL.W_ACTOR_METHOD_ATTEMPTS, "a0": DL.W_A0, "a1": DL.W_A1,
                             "a2": DL.W_A2, "tag": DL.W_TAG}
    assert lay["control"] == {"head": DL.C_HEAD, "tail": DL.C_TAIL, "dropped": DL.C_DROPPED, "sends": DL.C_SENDS,
                              "base": DL.C_BASE, "torn": DL.C_TORN, "seq": DL.C_SEQ}
    assert (lay["min_entries"], lay["max_entries"], lay["max_attempts"]) == (DL.MIN_ENTRIES, DL.MAX_ENTRIES,
                                                                             DL.MAX_ATTEMPTS)
    assert sorted(lay["record"].values()) == list(range(8)) and sorted(lay["control"].values()) == list(range(7))


@pytest.mark.parametrize("entries", [64, 4096])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, BIG])
def test_kernels_against_the_model(M, entries):
    """Four Sends of random statuses from {0 .. 8, -1, 40}, the column variants taking
    turns; the ring and the control line after every one, then the letters."""
    gpu, ref = pair(entries, DL.DEFAULT_MASK | (1 << 8 if M % 2 else 0))
    for n in range(4):
        b, st, att = random_send(M, 7 * M + n, a1=n != 1, a2=n != 2, method="col" if n % 2 else 40000 + n,
                                 attempts=n >= 2)
        both(gpu, ref, b, st, att, tag=-n)
    assert gpu.read() == dict(ref.read(), redrives=0, redriven=0) and ref.read()["sends"] == 4
    same_letters(gpu.take(drain=False), ref.take(drain=False))
    same_words(ref, gpu)


def test_single_letters_on_the_wave_segment_and_tile_edges():
    gpu, ref = pair(64)
    b, _, _ = random_send(BIG, 1)
    bg = _cuda(b)
    edges = [0, BIG - 1, 255, 256, 1023, 1024, T - 1, T, 63, 64, 2 * T - 1, 2 * T, 3 * T]
    for row in edges:
        st = torch.zeros(BIG, dtype=torch.int32)
        st[row] = STATUS_FAILED
        both(gpu, ref, b, st, bg=bg)
    got = gpu.take()
    same_letters(got, ref.take())
    assert got.row.cpu().tolist() == edges and got.seq.cpu().tolist() == list(range(1, len(edges) + 1))
    st = torch.zeros(BIG, dtype=torch.int32)
    st[edges] = STATUS_NO_ACTOR  # all of them in one Send
    both(gpu, ref, b, st, bg=bg)
    assert gpu.take().row.cpu().tolist() == sorted(edges) == ref.take()["row"].tolist()


@pytest.mark.parametrize("entries", [64, 4096])
def test_every_row_a_letter(entries):
    """K = M > entries: only the last ``entries`` letters are written, each slot once."""
    M = 2 * T + 5
    gpu, ref = pair(entries)
    b, st, _ = random_send(M, 2, k=M)
    both(gpu, ref, b, st)
    both(gpu, ref, b, st, tag=5)  # and once more from a head that is no multiple of the ring
    got = gpu.take()
    assert got.n == entries and got.torn == 0 and got.row.cpu().tolist() == list(range(M - entries, M))
    r = gpu.read()
    assert (r["appended"], r["dropped"], r["unread"], r["sends"]) == (2 * M, 2 * M - entries, 0, 2)


def test_a_send_without_a_letter_leaves_the_ring_alone():
    gpu, ref = pair(64)
    b, st, _ = random_send(T + 9, 3, k=40)
    both(gpu, ref, b, st)
    ring, head = gpu.ring.clone(), gpu.read()["appended"]
    for M in (T + 9, 0):
        b0, st0, _ = random_send(M, 4, k=0)
        both(gpu, ref, b0, st0)
    r = gpu.read()
    assert torch.equal(ring, gpu.ring) and r["appended"] == head == 40 and r["sends"] == 3


def test_column_variants():
    M = T + 65
    b, st, att = random_send(M, 5, attempts=True)
    zeros = torch.zeros(M, dtype=torch.int64)
    # a1 / a2 absent against zero columns
    g1, r1 = pair(4096)
    g2, _ = pair(4096)
    both(g1, r1, MsgBatch(b.actor, b.a0, None, None, b.method), st)
    g2.append(_cuda(MsgBatch(b.actor, b.a0, zeros, zeros, b.method)), st.cuda())
    assert torch.equal(g1.ring, g2.ring) and torch.equal(g1.ctrl, g2.ctrl)
    # a uniform method against an int16 column (the id is read as u16)
    g1, r1 = pair(4096)
    g2, _ = pair(4096)
    both(g1, r1, MsgBatch(b.actor, b.a0, b.a1, b.a2, 0xFFF0), st)
    g2.append(_cuda(MsgBatch(b.actor, b.a0, b.a1, b.a2, torch.full((M,), -16, dtype=torch.int16))), st.cuda())
    assert torch.equal(g1.ring, g2.ring)
    # attempts absent against a column of zeros; a given column, saturating
    g1, r1 = pair(4096)
    g2, r2 = pair(4096)
    both(g1, r1, b, st)
    both(g2, r2, b, st, torch.zeros(M, dtype=torch.int32))
    assert torch.equal(g1.ring, g2.ring)
    g3, r3 = pair(4096)
    att[:4] = torch.tensor([65533, 65534, 65535, -1], dtype=torch.int32)
    st[:4] = STATUS_FAILED
    both(g3, r3, b, st, att)
    assert g3.take().attempts.cpu().tolist()[:4] == [65534, 65535, 65535, 65535]


def test_unaligned_views():
    M = T + 9
    gpu, ref = pair(4096)
    b, _, _ = random_send(M, 6)
    _, st1, att1 = random_send(M + 1, 7, attempts=True)
    # the status and attempts columns 4 bytes past a 16-byte boundary: scalar loads
    both(gpu, ref, b, st1[1:], att1[1:], stg=st1.cuda()[1:], attg=att1.cuda()[1:])
    # every batch column at an odd offset too
    b1, _, _ = random_send(M + 1, 8)
    both(gpu, ref, b1.slice(1, M + 1), st1[1:], bg=_cuda(b1).slice(1, M + 1), stg=st1.cuda()[1:])
    for off in (2, 3):
        both(gpu, ref, b1.slice(off, M + 1), st1[off:], bg=_cuda(b1).slice(off, M + 1), stg=st1.cuda()[off:])
    assert ref.read()["sends"] == 4 and ref.read()["appended"] > 4096  # (wrapped)


@pytest.mark.parametrize("E", [64, 256])
def test_the_shared_sequence_on_the_gpu(E):
    """test_dead_letters.py's sequence -- K in {0, 1, E - 1, E, E + 1, 3 E, ...}, drains in
    between (peek, ``max_letters``, whole) -- words and letters after every step."""
    gpu, ref = pair(E)
    seen = run_sequence(ref, gpu, E, to_device=_cuda)
    assert all(v > 0 for v in seen.values()), seen
    assert gpu.read() == dict(ref.read(), redrives=0, redriven=0) and ref.read()["sends"] == len(ks_of(E))


def test_take_across_the_wrap():
    gpu, ref = pair(64)
    for n in range(3):  # 150 letters: the unread ones are tickets 86 .. 149, slots 22 .. 63, 0 .. 21
        b, st, _ = random_send(300, 20 + n, k=50)
        both(gpu, ref, b, st, tag=n)
    peek = gpu.take(drain=False)
    same_letters(peek, ref.take(drain=False))
    assert peek.n == 64 and peek.ticket == 86 and gpu.read()["unread"] == 64
    same_letters(gpu.take(max_letters=30), ref.take(max_letters=30))  # ends before the wrap
    rest = gpu.take()
    same_letters(rest, ref.take())  # crosses it
    assert rest.n == 34 and rest.ticket == 116
    assert torch.equal(rest.a0, peek.a0[30:]) and torch.equal(rest.seq, peek.seq[30:])
    assert gpu.take().n == 0 and gpu.take(drain=False).n == 0 and gpu.read()["torn"] == 0
    same_words(ref, gpu)


# ---------------------------------------------------------------- a captured Send
def test_send_graph_files_every_replayed_step():
    M, n = T + 5, T
    ex, state = world1(n, M, device="cuda")
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(0, n + n // 8, (M,), generator=g).to(torch.int32)  # some unknown actors
    a0, a1 = torch.randint(-2**62, 2**62, (M,), generator=g), torch.randint(-2**62, 2**62, (M,), generator=g)
    req = MsgBatch(ids.cuda(), a0.cuda(), a1.cuda(), None, METHOD_CALC_MULTIPLY)
    out_val = torch.empty(M, dtype=torch.int64, device="cuda")
    out_status = torch.empty(M, dtype=torch.int32, device="cuda")
    gpu, ref = pair(4096)
    graph = ex.capture(req, out_val, out_status, dead_letters=gpu)
    assert gpu.read()["sends"] == 2  # the two warm-up sends file their letters too
    gpu.reset()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    missing = ids >= n
    K = int(missing.sum())
    assert 0 < K < 4096 // 3
    assert torch.equal(out_status.cpu(), torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32))
    for _ in range(3):
        ref.append(MsgBatch(ids, a0, a1, None, METHOD_CALC_MULTIPLY), out_status.cpu())
    same_words(ref, gpu)
    got = gpu.take()
    assert got.n == 3 * K and got.seq.cpu().tolist() == [1] * K + [2] * K + [3] * K
    assert got.row.cpu().tolist() == torch.nonzero(missing).flatten().tolist() * 3
    # a larger eager Send outgrows the workspace the graph was captured with (this queue was
    # made without max_rows): the graph keeps launching into its own, which stays alive
    ref.take()
    big, stb, _ = random_send(5 * T, 9, k=7)
    both(gpu, ref, big, stb)
    graph.replay()
    torch.cuda.synchronize()
    ref.append(MsgBatch(ids, a0, a1, None, METHOD_CALC_MULTIPLY), out_status.cpu())
    same_words(ref, gpu)
    assert len(gpu._outgrown) >= 1


# ---------------------------------------------------------------- world 1 on the GPU
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_dead_letters_and_redrive_world1_gpu(delivery):
    rt = gpu_runtime(delivery, dead_letters=True, dead_letter_entries=64)
    try:
        dead_letter_scenario(rt, dev="cuda")
    finally:
        rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_retries_coalescing_and_no_queue_world1_gpu(delivery):
    """test_dead_letters.py's CPU scenarios on the GPU: only what still failed after the
    retries is a letter, a failed leader's followers each get one, redrives alone empty
    the queue, and without the setting nothing is created."""
    rt, plain = gpu_runtime(delivery, dead_letters=True), gpu_runtime(delivery)
    try:
        retries_scenario(rt, "cuda")
        followers_scenario(rt, "cuda")
        no_queue_scenario(plain, "cuda")
        # the same at more than one tile: 500 followers per failed leader
        actor = torch.tensor([5, 700, 5, 700, 700, 6] * 500, dtype=torch.int32)
        c = MsgBatch(actor.cuda(), (actor.to(torch.int64) + 1).cuda(), (actor.to(torch.int64) - 1).cuda(), None,
                     METHOD_CALC_MULTIPLY)
        val, st = rt.send("calculator", c, coalesce=True)
        lt = letters_of(rt, drain=True)
        assert lt["row"] == torch.nonzero(actor == 700).flatten().tolist() and set(lt["status"]) == {STATUS_NO_ACTOR}
    finally:
        rt.close()
        plain.close()
    rt = gpu_runtime(delivery, dead_letters=True)
    try:
        redrive_alone_scenario(rt, "cuda")
    finally:
        rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
@pytest.mark.parametrize("named", [False, True])
def test_breaker_and_limiter_answers_are_letters_only_when_named_gpu(named, delivery):
    """The statuses the limiter's and the breaker's admit kernels write (8, 7) reach the
    append and are filed only when the mask names them."""
    rt = gpu_runtime(delivery, dead_letters=True, dead_letter_mask=named_mask(named), breaker_threshold=1,
                     limit_burst=2)
    try:
        breaker_and_limiter_scenario(rt, named, "cuda")
    finally:
        rt.close()


def test_with_every_other_wrapper_gpu():
    rt = gpu_runtime(dead_letters=True, ledger=True, breaker_threshold=100, limit_burst=100)
    plain = gpu_runtime()
    try:
        b, want = mixed_batch("cuda")
        g = Gather(torch.zeros(b.M, dtype=torch.int32, device="cuda"), 1, "sum")
        val, st = rt.send("calculator", b, coalesce=True, cache=True, breaker=True, limit=True, gather=g)
        pv, ps = plain.send("calculator", b)
        assert torch.equal(st, ps) and st.cpu().tolist() == want and torch.equal(val, pv)
        bad = [i for i, s in enumerate(want) if s]
        lt = letters_of(rt)
        assert lt["row"] == bad and lt["status"] == [want[i] for i in bad] and lt["actor"] == b.actor.cpu()[bad].tolist()
        assert rt.stats()["ledger"]["messages"] == b.M and int(g.n_ok[0]) == want.count(0)
        assert rt.stats()["dead_letters"]["sends"] == 1
    finally:
        rt.close()
        plain.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
def test_dead_letters_multirank_fakecomm():
    """Two in-process ranks, each with a queue of its own: a rank files the failures of the
    batch it sent (the caller's view), whichever rank ran the messages."""
    R_, M, n = 2, T + 65, 6000
    fc = hip().FakeComm(R_)
    batches = []
    for r in range(R_):
        g = torch.Generator().manual_seed(40 + r)
        batches.append(MsgBatch(torch.randint(0, n + 500 * (r + 1), (M,), generator=g).to(torch.int32),
                                torch.randint(-30000, 30000, (M,), generator=g),
                                torch.randint(-30000, 30000, (M,), generator=g), None, METHOD_CALC_MULTIPLY))
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
                q = DL.DeadLetters("cuda", 4096)
                start.wait(timeout=60)
                val, sts = ex.send_all(_cuda(batches[r]), dead_letters=q.bound(tag=r + 1))
                s.synchronize()
                results[r] = (sts.cpu(), q.ring.cpu(), q.ctrl.cpu(), q.read())
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
        sts, ring, ctrl, rd = results[r]
        missing = batches[r].actor >= n
        assert torch.equal(sts, torch.where(missing, STATUS_NO_ACTOR, STATUS_OK).to(torch.int32)), r
        ref = DL.DeadLetterRef(4096)
        ref.append(batches[r], sts, tag=r + 1)
        assert np.array_equal(ring.numpy().view(np.uint64), ref.ring), r
        assert np.array_equal(ctrl.numpy().view(np.uint64), ref.ctrl), r
        assert rd["appended"] == int(missing.sum()) > 0 and rd["sends"] == 1
    assert results[0][3]["appended"] != results[1][3]["appended"]  # independent queues


# ---------------------------------------------------------------- Client.Send through Join
def test_client_dead_letters_and_redrive_through_join_gpu(tmp_path, ports, monkeypatch):
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
    cfg.gpu.dead_letters, cfg.gpu.dead_letter_entries = True, 128
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        rt = c.runtime
        assert rt._dlq is not None and (rt._dlq.entries, rt._dlq.mask) == (128, DL.DEFAULT_MASK)
        client = c.NewClient("calculator", C.ConnConfig())
        dead_letter_scenario(rt, dev="cuda", send=lambda b: client.Send(b, dead_letter=True), redrive=client.Redrive,
                             tag=DL.fnv1a64("calculator"))
        d = c.Stats()["runtime"]["dead_letters"]
        assert client.DeadLetters().n == 0 and (d["entries"], d["redrives"], d["unread"], d["torn"]) == (128, 4, 0, 0)
        b, want = mixed_batch("cuda")
        client.Send(b, dead_letter=False)
        assert c.Stats()["runtime"]["dead_letters"]["sends"] == d["sends"]
        client.Send(b)  # no argument: gpu.dead_letters
        assert c.Stats()["runtime"]["dead_letters"]["sends"] == d["sends"] + 1
        tag = DL.fnv1a64("calculator")
        assert set(letters_of(rt)["tag"]) == {tag - (1 << 64) if tag >> 63 else tag}
        client.Close()
    finally:
        server.Close()
        c.Close()
