"""Boundary values of every width-adaptive record encoding, on MI355X.

Each encoding of the data plane has a "does it fit" predicate, a mask, a shift and a
fallback (spill, escape, overflow, long form); a kernel wrong by one bit at such an
edge still answers exactly for almost every random input.  These tests place values
exactly at +-2^(w-1) of the width in force (and INT32 / INT64 extremes) at the tile
positions where a sort goes wrong, predict from the integer models of
tests/_edge_cases.py what fits, and compare every reply and status for equality with
the torch int64 / ``B._handler_ref`` / ``audit_fold`` reference -- and every spill,
overflow and escape count for equality with the model, so a kernel that takes its
slow path for everything fails as well.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import _edge_cases as E
import test_packed_wire as PW
import test_sorted_exchange_gpu as SX
from ptype_amd.ops import batch as B
from ptype_amd.ops import gob as G
from ptype_amd.ops import packed as P
from ptype_amd.ops.mailbox import Mailboxes
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK, STATUS_NO_METHOD, STATUS_OK,
                                   STATUS_OVERFLOW)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))


# ----------------------------------------------------------------- a-c: world-1 mailbox record forms
def _child(config, tune):
    """All cases of one tune configuration in ONE fresh child process (the switches
    are read once per process): tests/_edge_child.py prints one JSON line."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE]))
    if tune:
        env["PTYPE_TUNE"] = tune
    else:
        env.pop("PTYPE_TUNE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_edge_child.py"), config], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(line[-1][7:])


def _check_child(out, fields):
    assert out["cases"], out
    assert set(out["placed"]) == set(fields), (sorted(out["placed"]), fields)  # every field the configuration is about
    for name, c in out["cases"].items():
        assert c["ok"], (name, c)
        assert c["model"] == c["device"], (name, c)  # every count and width: equal to the model's
    for field, n in out["placed"].items():  # a generator bug cannot empty a case
        assert n["fit"] >= 1 and n["nofit"] >= 1, (field, out["placed"])


@pytest.mark.parametrize("fused", ["1", "0"])
def test_rec8_stateless_widths_walk(fused):
    _check_child(_child("rec8", f"mbox_rec8=1,mbox_fused={fused}"),
                 ["dir.a0", "dir.a1", "dir.mailbox", "dir.sizes.a0", "state.a0", "state.a1", "state.mailbox",
                  "state.int64.a0", "state.int64.a1"])


@pytest.mark.parametrize("tune", ["", "mbox_drain_msg=1"])
def test_compact_and_long_records_at_int32_edges(tune):
    _check_child(_child("compact", tune), ["compact.a0", "compact.a1"])


def test_arrival_rec8_one_misfit_in_one_wave():
    _check_child(_child("arrival8", "mbox_rec8=1"), ["arrival8.a0", "arrival8.a1"])


def test_ordered_rec8_escapes_at_the_width_edges():
    _check_child(_child("ordered8", "mbox_rec8=1"), ["ordered8.a0"])


# ----------------------------------------------------------------- d: wire v3 on the epoch engine
def _v3(cbs, R=2, n=2000):
    """The batches through wire v3 on the GPU and the v2 CPU reference pipeline
    (test_packed_wire's simulated exchange): bit for bit.  Returns the layout."""
    M = max(b.M for b in cbs)
    C = B.stripe_capacity(M, R)
    tabs = [PW._tables(n, R, True) for _ in range(R)]
    L, got, ref = PW._packed_vs_v2(cbs, tabs, R, n, C)
    for r in range(R):
        assert torch.equal(got[r][1], ref[r][1]), r
        assert torch.equal(got[r][0], ref[r][0]), r
    return L, got


def _v3_batch(M, n, seed, edges, method=METHOD_CALC_MULTIPLY, small=8, a1=True):
    actor, a0, b1, pos = E.place(M, edges, n, seed, small=small, tile=E.SMALL_TILE)
    z = torch.zeros_like(a0)  # (an absent column: zeros, a zero-width field)
    return B.MsgBatch(actor, a0, b1 if a1 else z, z.clone(), method), pos


@pytest.mark.parametrize("mcol", [False, True])
def test_v3_full_range_arguments(mcol):
    """INT64_MIN / INT64_MAX in every argument column: 64-bit fields (the >= 64 branches
    of the mask, the fit test and the field extraction), records of 5 (two arguments)
    and 7-8 dwords (three and a method column; 8 with a 15-bit unknown method id)."""
    n, M = 2000, 1000
    ext = [E.INT64_MIN, E.INT64_MAX, -1, 0, 1]
    cbs = []
    for r in range(2):
        b, pos = _v3_batch(M - 37 * r, n, 60 + r, E.pairs(ext, ext))
        if mcol:
            g = torch.Generator().manual_seed(70 + r)
            meth = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK])[
                torch.randint(0, 3, (b.M,), generator=g)].to(torch.int16)
            a2 = torch.randint(-7, 8, (b.M,), generator=g)
            a2[pos[0]], a2[pos[1]], a2[pos[2]], a2[pos[-1]] = E.INT64_MAX, E.INT64_MIN, E.INT64_MAX, E.INT64_MIN
            pc = meth == METHOD_PRIME_CHECK  # Prime.Check: at most 16 candidates
            lo = torch.randint(-3, 20, (b.M,), generator=g)
            b.a0 = torch.where(pc, lo, b.a0)
            b.a1 = torch.where(pc, lo + torch.randint(0, 17, (b.M,), generator=g), b.a1)
            meth[pos[1]] = METHOD_PRIME_CHECK  # target INT64_MIN: the reply is the target
            b.a0[pos[1]], b.a1[pos[1]] = 2, 18
            meth[pos[2]] = METHOD_PRIME_CHECK  # target INT64_MAX = 7 * 7 * 73 * ...: divisor 7
            b.a0[pos[2]], b.a1[pos[2]] = 2, 18
            meth[pos[3]], meth[pos[4]] = METHOD_CALC_MULTIPLY, METHOD_ECHO
            b.a0[pos[3]], b.a1[pos[3]] = E.INT64_MIN, E.INT64_MAX
            b.a0[pos[4]] = E.INT64_MIN
            if r == 1:
                meth[pos[5]] = 0x7FFF  # no such method: a 15-bit method field
                b.actor[pos[6]] = n + 5  # no such actor: a 24-bit mailbox field
            b = B.MsgBatch(b.actor, b.a0, b.a1, a2, meth)
        cbs.append(b)
    L, got = _v3(cbs)
    assert L["w"][2] == 64 and L["w"][3] == 64 and L["vb"] == 8
    if mcol:
        assert L["w"][4] == 64 and L["w"][0] == 15 and L["S"] == 8, L
        assert int(got[1][1][E.edge_positions(cbs[1].M, 6, E.SMALL_TILE)[5]]) == STATUS_NO_METHOD
    else:
        assert L["w"][0] == 0 and L["w"][4] == 0 and L["S"] == 5, L


@pytest.mark.parametrize("b,below,above", [(8, 1, 2), (16, 2, 4), (32, 4, 8)])
def test_v3_reply_plane_steps_at_the_byte_boundaries(b, below, above):
    """One batch per side of every reply boundary.  Echo: the largest reply's zigzag is
    2^b - 1 (reply -(2^(b-1))), then 2^b (reply 2^(b-1)).  Multiply: the plane is sized
    by the bound 2 |a| |b| of the column maxima, which counts the magnitude alone, so the
    widest product below the step is +-(2^(b-1) - 1) (zigzag 2^b - 2 / 2^b - 3) and
    -(2^(b-1)), whose zigzag 2^b - 1 would still fit, already steps -- as +2^(b-1) does."""
    n, M, h = 2000, 1000, 1 << (b - 1)
    for edges, meth, vb in [
        ([(None, -h, 0), (None, h - 1, 0)], METHOD_ECHO, below),
        ([(None, -h, 0), (None, h, 0)], METHOD_ECHO, above),
        ([(None, h - 1, -1), (None, -(h - 1), 1), (None, h - 1, 1)], METHOD_CALC_MULTIPLY, below),
        ([(None, h, -1), (None, h - 1, 1)], METHOD_CALC_MULTIPLY, above),
        ([(None, -h, -1), (None, h - 1, 1)], METHOD_CALC_MULTIPLY, above),
    ]:
        cbs = []
        for r in range(2):
            actor, a0, a1, _ = E.place(M - 11 * r, edges, n, 80 + r, small=8, tile=E.SMALL_TILE)
            a1 = a1.clamp(-1, 1)  # (the edge messages' second arguments are within it)
            echo = meth == METHOD_ECHO
            z = torch.zeros_like(a0)  # (an absent column: zeros, a zero-width field)
            cbs.append(B.MsgBatch(actor, a0, z if echo else a1, z.clone(), meth))
        L, got = _v3(cbs)
        assert L["vb"] == vb, (b, edges, meth, L)
        top = max(E.zz(int(v)) for r in range(2) for v in got[r][0][got[r][1] == STATUS_OK].tolist())
        want = max(E.zz(x if meth == METHOD_ECHO else x * y) for _, x, y in edges)
        assert top == want and (top < (1 << (8 * vb))), (b, meth, top, want)


def test_v3_wrapping_products_take_raw_replies():
    n, M = 2000, 1000
    edges = [(None, E.INT64_MIN, -1), (None, 1 << 62, 4), (None, E.INT64_MAX, E.INT64_MAX), (None, E.INT64_MIN, E.INT64_MIN),
             (None, -1, E.INT64_MIN), (None, E.INT64_MAX, 2)]
    cbs = [_v3_batch(M - 5 * r, n, 90 + r, edges)[0] for r in range(2)]
    L, got = _v3(cbs)
    assert L["vb"] == 8
    pos = E.edge_positions(M, len(edges), E.SMALL_TILE)
    known = got[0][1][pos] == STATUS_OK
    assert bool(known.all())
    wrap = lambda v: ((v + (1 << 63)) % (1 << 64)) - (1 << 63)  # noqa: E731
    assert got[0][0][pos].tolist() == [wrap(x * y) for _, x, y in edges]
    assert wrap(E.INT64_MIN * -1) == E.INT64_MIN and wrap((1 << 62) * 4) == 0


# ----------------------------------------------------------------- e: sorted exchange (FakeComm, R = 2)
SX_R, SX_N, SX_M = 2, 4096, 2 * E.TILE + 1


def _sx_batch(M, n, seed, edges, small, method=METHOD_CALC_MULTIPLY, zero_a1=False):
    actor, a0, a1, pos = E.place(M, edges, n, seed, small=small)
    if zero_a1:
        a1 = torch.zeros_like(a1)
    return B.MsgBatch(actor.cuda(), a0.cuda(), a1.cuda(), None, method), (a0, a1, pos)


def _affine_table(n, R):
    t = RegistryTable(2 * n, device="cuda")
    ids = torch.arange(n)
    t.upsert(actor_keys(ids), (ids % R).to(torch.int32), (ids // R).to(torch.int32))
    t.enable_directory(n, affine_world=R)
    return t


def _sx_run(settle_edges, test_edges, small, n_settle_actors=SX_N, affine=False, resend=True, echo=False):
    """Per rank: three settling Multiply Sends (their extremes: ``settle_edges``), then the
    test batch through a plain ``send`` and -- ``resend`` -- the same batch through
    ``send_all``.  ``echo``: every a1 is zero and the test batch is a uniform Echo (a
    method the agreements in force never saw).  Returns per rank a dict of CPU results."""
    R, n, M = SX_R, SX_N, SX_M

    def body(r, fc, start, s):
        tab = _affine_table(n, R) if affine else SX._table(n, R)[0]
        st = torch.zeros(n // R + 1, dtype=torch.int64, device="cuda")
        ex = ActorExchange(tab, M, chunks=1, state=st, fake=(fc, r), delivery="mailbox", mailbox_ordered=False)
        start.wait()
        for k in range(3):
            b, _ = _sx_batch(M, n_settle_actors, 10 * r + k, settle_edges, small, zero_a1=echo)
            v, sts = ex.send(b)
            s.synchronize()
            assert bool((sts == STATUS_OK).all()) and torch.equal(v, b.a0 * b.a1), (r, k)
        b, (a0, a1, pos) = _sx_batch(M, n_settle_actors, 100 + r, test_edges, small,
                                     METHOD_ECHO if echo else METHOD_CALC_MULTIPLY, zero_a1=echo)
        v, sts = ex.send(b)
        s.synchronize()
        out = {"a0": a0, "a1": a1, "pos": pos, "wire": dict(ex.last_wire), "v": v.cpu(), "st": sts.cpu(),
               "ref": (b.a0 if echo else b.a0 * b.a1).cpu()}
        if resend:
            r0 = ex.counters.resends
            v, sts = ex.send_all(b)
            s.synchronize()
            out.update(v_all=v.cpu(), st_all=sts.cpu(), resends=ex.counters.resends - r0)
        stats = ex.stats()
        out.update(toowide=int(stats.toowide), failed=int(stats.failed))
        return out

    return SX._run_ranks(R, body)


def _sx_check(o, expect_overflow=None, echo=False):
    """The contract of a Send on a lagged layout: a plain ``send`` answers OK and exact
    or STATUS_OVERFLOW -- exactly the messages the model refuses -- and ``send_all`` ends
    all OK and exact; no receiver ever met a reply wider than the plane."""
    w, vb, meta = o["wire"]["w"], o["wire"]["vb"], o["wire"]["meta"]
    if echo:  # the reply is a0: within its field and within the plane
        caps = (min((1 << w[2]) - 1, (1 << (8 * vb)) - 1), (1 << w[3]) - 1)
    else:
        caps = E.sx_arg_caps(w, vb, meta[P.META_ARG0], meta[P.META_ARG0 + 1],
                             bool(meta[P.META_FLAGS + METHOD_CALC_MULTIPLY]))
        for x, y in ((caps[0], caps[1]), (caps[0] - 1, caps[1]), (caps[0], caps[1] - 1)):  # whatever they admit fits
            if vb < 8 and min(x, y) >= 0:
                assert E.multiply_reply_bits(E.unzz(x), E.unzz(y)) <= 8 * vb, (caps, x, y)
    assert list(caps) == list(o["wire"]["arg_caps"])[:2], (caps, o["wire"]["arg_caps"])
    a0, a1 = o["a0"].tolist(), o["a1"].tolist()
    admit = torch.tensor([E.sx_admits(caps, x, y) for x, y in zip(a0, a1)])
    st, v = o["st"], o["v"]
    print("sorted exchange: w", w, "vb", vb, "caps", caps, "refused by the model", int((~admit).sum()), "statuses",
          {int(k): int((st == k).sum()) for k in st.unique()}, "toowide", o["toowide"], "failed", o["failed"])
    assert o["toowide"] == 0 and o["failed"] == 0, (o["toowide"], o["failed"])
    assert bool(((st == STATUS_OK) | (st == STATUS_OVERFLOW)).all()), st.unique()
    assert torch.equal(st == STATUS_OVERFLOW, ~admit), (int((st == STATUS_OVERFLOW).sum()), int((~admit).sum()))
    assert torch.equal(v[admit], o["ref"][admit])
    if expect_overflow is not None:
        assert int((~admit).sum()) == expect_overflow
    if "st_all" in o:
        assert bool((o["st_all"] == STATUS_OK).all()), o["st_all"].unique()
        assert torch.equal(o["v_all"], o["ref"])
        assert (o["resends"] >= 1) == bool((~admit).any())
    return admit


@pytest.mark.parametrize("amax,w,vb", [(8, 5, 1), (64, 8, 2), (128, 9, 2), (32768, 17, 4)])
def test_sorted_exchange_reply_width_of_a_lagged_layout(amax, w, vb):
    """Send k runs on the layout agreed from Send k - 2: its request fields admit by bit
    width, its reply plane was sized from the VALUES of those maxima.  After Sends whose
    extreme arguments are +-amax, the widest arguments the fields hold multiply to a
    reply of up to two bits more than the plane holds (amax 8: 10 bits into 1 byte;
    128: 18 into 2 bytes; 32768: 34 into 4; 64 just fits its 2 bytes).  The sender
    admits Multiply arguments by value caps whose product bound fits the plane
    (``_edge_cases.sx_arg_caps``) and refuses the rest (STATUS_OVERFLOW, re-sent by
    ``send_all`` once the layout that saw them is in force) -- before it did, the
    receivers answered STATUS_FAILED for a valid Calculator.Multiply."""
    lo, hi = -(1 << (w - 1)), (1 << (w - 1)) - 1
    ext = [lo, hi, amax, -amax]
    res = _sx_run([(None, amax, -amax), (None, -amax, amax)], E.pairs(ext, ext), small=min(100, amax))
    for o in res:
        assert o["wire"]["agreed"] and o["wire"]["w"][2:4] == [w, w] and o["wire"]["vb"] == vb, o["wire"]
        admit = _sx_check(o)
        at = admit[o["pos"]]
        assert bool(at.any())  # (+-amax themselves are within the agreed bounds)
        assert bool((~at).any()) == (amax != 64)


def test_sorted_exchange_echo_the_agreement_never_saw():
    """The reply plane is sized from the methods the agreement in force flagged.  After
    Multiply Sends whose second argument is always zero (bound 0: a 1-byte plane) and
    whose first reaches +-128 (a 9-bit field), a uniform Echo batch fits the fields with
    replies of up to 9 bits: the sender admits what the plane holds (zigzag <= 255) and
    refuses the rest, ``send_all`` re-sends it under a layout that saw Echo.  (Admitted,
    such a reply meets the receivers' width check: STATUS_FAILED.)"""
    res = _sx_run([(None, 128, 0), (None, -128, 0)],
                  [(None, v, 0) for v in (-128, 127, 128, -129, 255, -256, 256, -257, 0, 1)], small=100, echo=True)
    for o in res:
        assert o["wire"]["w"][2:4] == [9, 0] and o["wire"]["vb"] == 1, o["wire"]
        assert not o["wire"]["meta"][P.META_FLAGS + METHOD_ECHO]
        admit = _sx_check(o, expect_overflow=6, echo=True)
        assert admit[o["pos"]].tolist() == [True, True, False, False, False, False, False, False, True, True]


def test_sorted_exchange_request_fields_at_the_edges():
    """Arguments at the ends of the fields in force (22 bits after +-2^20; the reply plane
    is 8 bytes, so the fields alone decide): exactly the values past them overflow."""
    h = 1 << 20
    res = _sx_run([(None, h, -h), (None, -h, h)],
                  E.pairs(E.edge_values(22), [3]) + E.pairs([-5], E.edge_values(22))
                  + [(None, -(1 << 21) - 1, 1 << 21), (None, (1 << 21) - 1, -(1 << 21))], small=100)
    for o in res:
        assert o["wire"]["w"][2:4] == [22, 22] and o["wire"]["vb"] == 8, o["wire"]
        admit = _sx_check(o, expect_overflow=5)
        assert int(admit[o["pos"]].sum()) == len(o["pos"]) - 5


def test_sorted_exchange_full_range_arguments():
    ext = [E.INT64_MIN, E.INT64_MAX]
    res = _sx_run(E.pairs(ext, ext), E.pairs(ext + [-1, 1], ext + [-1, 1]), small=100, resend=False)
    for o in res:
        assert o["wire"]["w"][2:4] == [64, 64] and o["wire"]["vb"] == 8, o["wire"]
        _sx_check(o, expect_overflow=0)


def test_sorted_exchange_mailbox_all_ones_is_not_the_null():
    """An affine directory of R * 2^b actors: the largest local mailbox is 2^b - 1.  The
    settling Sends carry mailboxes up to 2^b - 2 only; the mailbox field is sized by bit
    length plus one, so the all-ones null record stays distinct and the Send that
    carries 2^b - 1 is answered without a re-send."""
    b = (SX_N // SX_R).bit_length() - 1
    top = SX_N - 1
    res = _sx_run([(SX_N - 3, 1, 1), (SX_N - 4, 1, 1)], [(top, 3, 5), (top - 1, 7, -9), (top - 2, 2, 2), (top, -4, 4)],
                  small=100, n_settle_actors=SX_N - 2, affine=True)
    for o in res:
        assert o["wire"]["w"][1] == b + 1 and o["wire"]["route_mode"] == 2, o["wire"]
        _sx_check(o, expect_overflow=0)
        assert o["resends"] == 0


# ----------------------------------------------------------------- f: small companions
def test_gob_varints_at_every_byte_boundary():
    vals = [63, 64, -64, -65, E.INT64_MIN, 0]
    for k in range(1, 9):
        h = 1 << (8 * k - 1)
        vals += [v for v in (h - 1, h, -h, -h - 1) if E.INT64_MIN <= v <= E.INT64_MAX]
    M = 128
    col = torch.tensor([vals[i % len(vals)] for i in range(M)], dtype=torch.int64)
    cols = [col, col.flip(0)]
    ref_buf, ref_offs = G.encode_structs_ref(cols, 65)
    buf, offs = G.encode_structs([c.cuda() for c in cols], 65)
    assert torch.equal(offs.cpu(), ref_offs)
    assert torch.equal(buf.cpu(), ref_buf)
    back, st = G.decode_structs(buf, offs, 2, 65)
    assert not bool(st.any())
    for a, b in zip(cols, back):
        assert torch.equal(a, b.cpu())


@pytest.mark.parametrize("sharding", ["actor", "arrival"])
def test_prime_check_at_the_32_bit_switch(sharding):
    """Prime.Check's handler divides in 32 bits when 0 <= lo and 0 < target <= 2^32 - 1,
    else in 64: targets on both sides of the switch, a negative lo, lo = 0 (the i != 0
    guard) and hi cut by the target, against Python big ints."""
    T32 = (1 << 32) - 1  # 3 * 5 * 17 * 257 * 65537
    cases = [(65536, 65540, T32), (65538, 65554, T32), (65530, 65546, T32), (0, 16, T32), (0, 1, T32),
             (0, 16, 1 << 32), (1, 17, 1 << 32), (2, 18, 1 << 32), (3, 4, 1 << 32),
             (630, 646, (1 << 32) + 1), (642, 658, (1 << 32) + 1), (0, 2, (1 << 32) + 1),
             (2, 18, (1 << 31) - 1), (0, 16, (1 << 31) - 1), (0, 1, (1 << 31) - 1),
             (-3, 5, T32), (-2, 6, (1 << 31) - 1), (-16, -1, 1 << 32), (-1, 1, 7), (0, 1, 7), (0, 3, 7),
             (2, 100, 9), (5, 100, 9), (2, 18, 0), (2, 18, -6), (0, 16, 1)]
    n, M = 256, 200
    t = RegistryTable(2 * n, device=DEV)
    ids = torch.arange(n)
    t.upsert(actor_keys(ids), torch.zeros(n, dtype=torch.int32), ids.flip(0).to(torch.int32))
    t.enable_directory(n)
    cols = [torch.tensor([cases[i % len(cases)][j] for i in range(M)], dtype=torch.int64) for j in range(3)]
    assert int((torch.minimum(cols[1], cols[2]) - cols[0]).max()) <= 16
    actor = (torch.arange(M) % n).to(torch.int32)
    ref_v, ref_s = B._handler_ref(torch.full((M,), METHOD_PRIME_CHECK), actor.long(), cols[0], cols[1], cols[2], None)
    assert ref_v[:len(cases)].tolist()[:4] == [65537, T32, 65535, 1] and bool((ref_s == 0).all())
    mb = Mailboxes(DEV, shards=64, slots=4096)
    req = B.MsgBatch(actor.to(DEV), cols[0].to(DEV), cols[1].to(DEV), cols[2].to(DEV), METHOD_PRIME_CHECK)
    val, st = mb.send(req, t, None, sharding=sharding)
    torch.cuda.synchronize()
    assert bool((st == STATUS_OK).all())
    assert torch.equal(val.cpu(), ref_v)
