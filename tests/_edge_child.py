"""Child process of tests/test_encoding_edges_gpu.py: every case of ONE tune
configuration (the switches are read once per process), world-1 mailbox Sends whose
arguments sit at the edges of the record widths in force.  Prints one line
``RESULT {json}``: per case the model's prediction and what the device did (spill
counts, record bytes, the widths derived for the next Send), whether every reply and
status was exact, and how many edge values were placed on each side of each field.

usage: _edge_child.py rec8 | compact | arrival8 | ordered8
"""
import json
import sys

import torch

import _edge_cases as E
from ptype_amd.ops import batch as B
from ptype_amd.ops.mailbox import Mailboxes, audit_fold
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK, METHOD_SEQ_FOLD,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys

DEV = torch.device("cuda", 0)
M2 = 2 * E.TILE + 1        # the smallest batch that crosses two 4096-message tiles
M1 = 2 * E.SMALL_TILE + 1  # ... two 1024-message tiles
CASES: dict = {}
PLACED: dict = {}


def placed(field, fit):
    PLACED.setdefault(field, {"fit": 0, "nofit": 0})["fit" if fit else "nofit"] += 1


def table(n, directory, seed=7):
    """Every actor on rank 0 at a random mailbox (a permutation)."""
    t = RegistryTable(2 * n, device=DEV)
    ids = torch.arange(n)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    t.upsert(actor_keys(ids), torch.zeros(n, dtype=torch.int32), perm.to(torch.int32))
    if directory:
        t.enable_directory(n)
    return t, perm


def rings_ok(mb, before):
    s = mb.stats()
    ctr = mb.shard_counters()
    return (s["overflow"] == before["overflow"] and s["holes"] == before["holes"] and s["lookback_timeouts"] == 0
            and bool((ctr[:, 0] == ctr[:, 2]).all()))


# ----------------------------------------------------------------- a: stateless Multiply, 8-B records
class Walk:
    """A mailbox set whose 8-B width state the model follows Send by Send."""

    def __init__(self, name, n, directory):
        self.name, self.n, self.rank_route = name, n, directory
        self.t, self.perm = table(n, directory)
        # without a directory the state sizes the mailbox field (Multiply reads none of it)
        self.state = None if directory else torch.zeros(n, dtype=torch.int64, device=DEV)
        self.mb = Mailboxes(DEV, shards=256, slots=4096)
        self.w = E.rec8_first(0 if directory else n, n if directory else 0) + (False,)
        self.k = 0
        assert self.mb.next_record_widths is None

    def field(self, actor):
        """What a record's mailbox field carries: the actor id on rank routes, else its mailbox."""
        return actor if self.rank_route else int(self.perm[actor])

    def actors_below(self, bound, count, seed):
        """``count`` random actors whose record field is below ``bound``."""
        g = torch.Generator().manual_seed(seed)
        f = torch.randint(0, bound, (count,), generator=g)
        if self.rank_route:
            return f.to(torch.int32)
        inv = torch.empty(self.n, dtype=torch.int64)
        inv[self.perm] = torch.arange(self.n)
        return inv[f].to(torch.int32)

    def actor_of_field(self, f):
        return f if self.rank_route else int((self.perm == f).nonzero()[0])

    def send(self, tag, actor, a0, a1, pos, count=()):
        wm, w0, w1, wide = self.w
        in8 = not wide
        A, X, Y = actor.tolist(), a0.tolist(), a1.tolist()
        known = [a < self.n for a in A]
        fld = [self.field(a) if k else 0 for a, k in zip(A, known)]
        nofit = [k and in8 and not E.rec8_fits(f, x, y, self.w) for k, f, x, y in zip(known, fld, X, Y)]
        if in8:
            for p in pos:  # the edge messages, per field the Send is about
                if not known[p]:
                    continue
                if "mailbox" in count:
                    placed(self.name + ".mailbox", fld[p] < (1 << wm))
                if "a0" in count:
                    placed(self.name + ".a0", E.fits(X[p], w0))
                if "a1" in count:
                    placed(self.name + ".a1", E.fits(Y[p], w1))
        model = {"bytes": 8 if in8 else 18 if self.rank_route else 16, "spilled": sum(nofit)}
        if in8 or self.rank_route:  # 8-B and wide pure records measure the fields for the next Send
            kn = [i for i, k in enumerate(known) if k]
            nxt = E.rec8_next(E.or_bits((fld[i] for i in kn), zigzag=False), E.or_bits(X[i] for i in kn),
                              E.or_bits(Y[i] for i in kn))
        else:
            nxt = self.w
        model["next"] = list(nxt)
        before = self.mb.stats()
        req = B.MsgBatch(actor.to(DEV), a0.to(DEV), a1.to(DEV), None, METHOD_CALC_MULTIPLY)
        v, st = self.mb.send(req, self.t, self.state, ordered=False)
        torch.cuda.synchronize()
        kt = torch.tensor(known)
        ok = (torch.equal(st.cpu(), torch.where(kt, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
              and torch.equal(v.cpu()[kt], (a0 * a1)[kt]) and rings_ok(self.mb, before))
        if self.rank_route:
            ok = ok and self.mb.last_route in (3, 4)
        dev = {"bytes": int(self.mb.last_record_bytes), "spilled": self.mb.stats()["spilled"] - before["spilled"],
               "next": list(self.mb.next_record_widths)}
        CASES[f"{self.name}.{self.k}.{tag}"] = {"ok": bool(ok), "model": model, "device": dev, "in_force": list(self.w)}
        self.w = tuple(nxt)
        self.k += 1


def rec8_walk(name, directory):
    n = 8192
    W = Walk(name, n, directory)
    sm = lambda: 3  # noqa: E731  (a small second argument beside an edge value)

    def batch(edges, seed, n_actors=n, small=100, M=M2):
        return E.place(M, edges[:M], n_actors, seed, small=small)

    # arguments at the ends of their fields, one column at a time (both would outgrow 52 bits)
    wm, w0, w1, _ = W.w
    W.send("a0_edges", *batch(E.pairs(E.edge_values(w0), [sm()]), 1), count=("a0",))
    wm, w0, w1, _ = W.w
    W.send("a1_edges", *batch(E.pairs([-sm()], E.edge_values(w1)), 2), count=("a1",))
    # the mailbox / id field: a Send of low values narrows it, the next one carries 2^wm - 1 (fits)
    # and 2^wm (spills)
    lowb = 9
    a, x, y, p = batch([(None, 1, 1)], 6)
    W.send("low_ids", W.actors_below(1 << lowb, M2, 60), x, y, p)
    assert W.w[0] == lowb, W.w
    a, x, y, p = batch([(W.actor_of_field((1 << lowb) - 1), 7, 7), (W.actor_of_field(1 << lowb), 7, 7),
                        (W.actor_of_field(n - 1), -7, 7), (W.actor_of_field(0), 7, -7)], 7)
    rest = W.actors_below(1 << lowb, M2, 61)
    keep = torch.zeros(M2, dtype=torch.bool)
    keep[p] = True
    W.send("id_edges", torch.where(keep, a, rest), x, y, p, count=("mailbox",))
    # maxima whose bit lengths sum to exactly 52 (13 + 20 + 19): still 8-B records afterwards
    W.send("narrow", *batch([(None, 5, -5)], 8))
    top = W.actor_of_field(n - 1)
    W.send("sum_52", *batch([(None, -(1 << 19), 3), (None, 3, (1 << 18) - 1), (top, 1, 1)], 9))
    assert W.w == (13, 20, 19, False), W.w
    # at those widths both arguments together: every field full (fits), then one bit more on a1 --
    # 53 bits, 8-B records given up: 18-B wide pure records on rank routes, 16-B compact ones otherwise
    W.send("sum_53", *batch([(top, -(1 << 19), (1 << 18) - 1), (top, (1 << 19) - 1, -(1 << 18)), (None, 1, 1 << 18)], 10),
           count=("a0", "a1"))
    assert W.w[3], W.w
    W.send("wide_then_narrow", *batch([(None, 5, -5)], 11))
    if not directory:
        return  # mailbox routes keep 16-B records from here on (rec8_mailbox_routes_int64: a new set)
    assert not W.w[3]  # (rank routes: wide pure records measure on, a narrow Send brings 8-B records back)
    # INT64_MIN / INT64_MAX in both arguments at the first and last places of the tiles: through the spill ...
    ext = [(None, E.INT64_MIN, E.INT64_MAX), (None, E.INT64_MAX, E.INT64_MIN), (None, E.INT64_MIN, E.INT64_MIN),
           (None, E.INT64_MAX, E.INT64_MAX), (None, E.INT64_MIN, -1), (None, 1, E.INT64_MAX)]
    a, x, y, p = batch(ext, 12)
    a[p[1]] = n + 3  # no such actor: answered, and its full-range arguments widen nothing ...
    W.send("int64_spill", a, x, y, p, count=("a0", "a1"))
    W.send("int64_wide_records", *batch(ext, 13))  # ... and through the 18-B wide records
    a, x, y, p = batch([(n + 9, E.INT64_MIN, E.INT64_MAX), (None, 5, -5)], 14)
    W.send("narrow_beside_unknown", a, x, y, p)  # (... here neither: this Send's maxima are narrow)
    assert not W.w[3], W.w
    W.send("back_to_8", *batch([(None, 5, -5)], 15))
    # the batch sizes around one tile, on a fresh set (each Send at the edges of the widths in force)
    V = Walk(name + ".sizes", n, directory)
    for M in (1, E.TILE - 1, E.TILE, E.TILE + 1):
        w0 = V.w[1]
        edges = E.pairs([1 << (w0 - 1), (1 << (w0 - 1)) - 1, -(1 << (w0 - 1)), -(1 << (w0 - 1)) - 1], [sm()])
        V.send(f"M{M}", *batch(edges, 20 + M % 7, M=M), count=("a0",))


def rec8_mailbox_routes_int64(name):
    """Mailbox routes: full-range arguments through the spill, then the 16-B / long records."""
    n = 8192
    W = Walk(name, n, False)
    ext = [(None, E.INT64_MIN, E.INT64_MAX), (None, E.INT64_MAX, E.INT64_MIN), (None, E.INT64_MIN, E.INT64_MIN),
           (None, E.INT64_MAX, E.INT64_MAX), (None, E.INT64_MIN, -1), (None, 1, E.INT64_MAX)]
    W.send("int64_spill", *E.place(M2, ext, n, 31), count=("a0", "a1"))
    W.send("int64_long_records", *E.place(M2, ext, n, 32))
    W.send("stays_16", *E.place(M2, [(None, 5, -5)], n, 33))


# ----------------------------------------------------------------- b: compact 16-B / long 32-B records
I32 = [E.INT32_MIN - 1, E.INT32_MIN, E.INT32_MAX, E.INT32_MAX + 1, E.INT64_MIN, E.INT64_MAX, -1, 0]


def three_arg_batch(M, n, seed, tile):
    """Echo / Multiply / Prime.Check (at most 16 candidates) with a method column; the
    INT32 / INT64 edges on a0 and on a1, a2 zero in some long records and not in others."""
    edges = E.pairs(I32, [3]) + E.pairs([-3], I32) + E.pairs(I32[:6], I32[:6])
    actor, a0, a1, pos = E.place(M, edges, n + 40, seed, tile=tile)  # (some unknown actors)
    g = torch.Generator().manual_seed(seed + 1000)
    meth = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK])[torch.randint(0, 3, (M,), generator=g)]
    a2 = torch.randint(-50, 50, (M,), generator=g) * torch.randint(0, 2, (M,), generator=g)
    pc = meth == METHOD_PRIME_CHECK
    for j, p in enumerate(pos):  # edge messages: Multiply and Echo only, a2 zero on every other one
        meth[p] = METHOD_CALC_MULTIPLY if j % 2 else METHOD_ECHO
        a2[p] = 0 if j % 4 < 2 else I32[j % 6]
        placed("compact.a0", E.fits_i32(int(a0[p])))
        placed("compact.a1", E.fits_i32(int(a1[p])))
    pc = meth == METHOD_PRIME_CHECK
    lo = torch.randint(-2, 40, (M,), generator=g)
    a0 = torch.where(pc, lo, a0)
    a1 = torch.where(pc, lo + torch.randint(0, 17, (M,), generator=g), a1)
    tgt = torch.tensor(I32[:6] + [97, 91, 1 << 32, (1 << 32) - 1])[torch.randint(0, 10, (M,), generator=g)]
    a2 = torch.where(pc, tgt, a2)
    return actor, a0, a1, a2, meth.to(torch.int16), pos


def compact_case(tag, n, t, M, tile, **send_kw):
    mb = Mailboxes(DEV, shards=256, slots=4096)
    actor, a0, a1, a2, meth, pos = three_arg_batch(M, n, 5, tile)
    ref_v, ref_s = B._handler_ref(meth.long(), actor.long(), a0, a1, a2, None)
    known = actor < n
    before = mb.stats()
    req = B.MsgBatch(actor.to(DEV), a0.to(DEV), a1.to(DEV), a2.to(DEV), meth.to(DEV))
    v, st = mb.send(req, t, None, ordered=False, **send_kw)
    torch.cuda.synchronize()
    ok = (torch.equal(st.cpu(), torch.where(known, ref_s, torch.full_like(ref_s, STATUS_NO_ACTOR)).to(torch.int32))
          and torch.equal(v.cpu()[known], ref_v[known]) and rings_ok(mb, before))
    s = mb.stats()
    CASES["compact." + tag] = {
        "ok": bool(ok), "model": {"bytes": 32, "spilled": 0, "processed": int(known.sum())},
        "device": {"bytes": int(mb.last_record_bytes), "spilled": s["spilled"] - before["spilled"],
                   "processed": s["processed"] - before["processed"]}}


def arrival_fused_case(tag, n, t, edges, bytes_, fields=(), seed=9):
    """The fused arrival Send (uniform Multiply, two arguments, 1024-message tiles)."""
    mb = Mailboxes(DEV, shards=256, slots=4096)
    actor, a0, a1, pos = E.place(M1, edges, n + 40, seed, tile=E.SMALL_TILE)
    for p in pos:
        for f, col in (("a0", a0), ("a1", a1)):
            if f in fields:
                placed(tag.split(".")[0] + "." + f, E.fits(int(col[p]), 20))
    known = actor < n
    before = mb.stats()
    v, st = mb.send(B.MsgBatch(actor.to(DEV), a0.to(DEV), a1.to(DEV), None, METHOD_CALC_MULTIPLY), t, None,
                    ordered=False, sharding="arrival")
    torch.cuda.synchronize()
    ok = (torch.equal(st.cpu(), torch.where(known, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
          and torch.equal(v.cpu()[known], (a0 * a1)[known]) and rings_ok(mb, before))
    s = mb.stats()
    CASES[tag] = {"ok": bool(ok), "model": {"bytes": bytes_, "spilled": 0, "processed": int(known.sum())},
                  "device": {"bytes": int(mb.last_record_bytes), "spilled": s["spilled"] - before["spilled"],
                             "processed": s["processed"] - before["processed"]}}


def compact_cases():
    n = 4096
    t, _ = table(n, True)
    compact_case("onepass", n, t, M2, E.TILE, sort_mode="onepass")
    compact_case("twopass", n, t, M2, E.TILE, sort_mode="twopass")
    compact_case("arrival_two_kernels", n, t, M2, E.TILE, sharding="arrival")
    compact_case("arrival_two_kernels_small", n, t, M1, E.SMALL_TILE, sharding="arrival")
    edges = E.pairs(I32, [3]) + E.pairs([-3], I32) + E.pairs(I32[:6], I32[:6])
    arrival_fused_case("compact.arrival_fused", n, t, edges, 16)


def arrival8_cases():
    """Arrival rings with 8-B records per wave {mailbox 24 | a0 20 | a1 20}: values at the ends
    of the 20-bit fields in several waves, exactly ONE value past them in exactly one wave, so
    one Send mixes both record forms (that wave must leave the 8-B form, the others may keep
    it).  Which waves took which form is not observable -- no counter records it, and
    ``last_record_bytes`` reports only that 8-B records were allowed -- so what is checked is
    that every reply is exact and every ring drained with the forms mixed."""
    n = 4096
    t, _ = table(n, True)
    h = 1 << 19
    fit = [(None, -h, h - 1), (None, h - 1, -h), (None, -h, -h), (None, h - 1, h - 1), (None, 0, -h)]
    # edge_positions: 0, 63, 64 (a wave's run of a 1024-message tile is 128 places: wave 0 of tile 0),
    # 1023 (its wave 7), 1024 (tile 1), M - 1 (tile 2) -- the one misfit goes to place 63
    for f, bad in (("a0", (None, h, 1)), ("a1", (None, 1, -h - 1))):
        edges = [fit[0], bad] + fit[1:]
        arrival_fused_case(f"arrival8.{f}", n, t, edges, 8, fields=(f,), seed=11)
    arrival_fused_case("arrival8.all_fit", n, t, fit, 8, seed=12)


# ----------------------------------------------------------------- c: ordered 8-B records with escapes
def ordered8_cases():
    n = 64
    t, perm = table(n, True)
    state = torch.randint(0, 1 << 30, (n,), dtype=torch.int64, generator=torch.Generator().manual_seed(3)).to(DEV)
    mb = Mailboxes(DEV, shards=256, slots=4096)
    w = E.rec8_first(n, n) + (False,)
    assert mb.next_record_widths is None

    def fold(tag, values, seed, count):
        nonlocal w
        edges = [(None, v, 0) for v in values] * 12  # every value many times, among ordinary messages
        actor, a0, _, pos = E.place(M2, edges, n, seed, small=1 << 15)
        for j, p in enumerate(pos):
            actor[p] = j % n  # every actor gets edge messages between its ordinary ones
        in8 = not w[3]
        if in8 and count:
            for p in pos:
                placed("ordered8.a0", E.fits(int(a0[p]), w[1]))
        A, X = actor.tolist(), a0.tolist()
        nxt = E.rec8_next(E.or_bits((int(perm[a]) for a in A), zigzag=False), E.or_bits(X), 0) if in8 else w
        model = {"bytes": 8 if in8 else 16, "overflow": 0, "next": list(nxt)}
        before, s0 = mb.stats(), state.cpu().clone()
        v, st = mb.send(B.MsgBatch(actor.to(DEV), a0.to(DEV), None, None, METHOD_SEQ_FOLD), t, state, sort_mode="onepass")
        torch.cuda.synchronize()
        ok, info = audit_fold(perm[actor.long()], a0, v.cpu(), st.cpu(), s0, state.cpu())
        fifo = bool(ok) and all(seq == sorted(seq) for seq in info.values())
        after = mb.stats()
        dev = {"bytes": int(mb.last_record_bytes), "overflow": after["overflow"] - before["overflow"],
               "next": list(mb.next_record_widths)}
        CASES["ordered8." + tag] = {"ok": bool(ok) and fifo and rings_ok(mb, before), "model": model, "device": dev,
                                    "in_force": list(w), "info": "" if ok else str(info)[:300]}
        w = tuple(nxt)

    fold("a0_edges", E.edge_values(w[1]), 1, True)
    fold("a0_edges_again", E.edge_values(w[1]), 2, True)  # (the widths the first Send left)
    fold("int64", [E.INT64_MIN, E.INT64_MAX, -1, 1], 3, False)  # escape, and the fields outgrow 8 B
    assert w[3], w
    fold("after_wide", [E.INT64_MIN, E.INT64_MAX, 5], 4, False)  # 16-B (long) records


def main(config):
    torch.cuda.set_device(DEV)
    if config == "rec8":
        rec8_walk("dir", True)
        rec8_walk("state", False)
        rec8_mailbox_routes_int64("state.int64")
    elif config == "compact":
        compact_cases()
    elif config == "arrival8":
        arrival8_cases()
    elif config == "ordered8":
        ordered8_cases()
    else:
        raise SystemExit("unknown configuration " + config)
    print("RESULT " + json.dumps({"cases": CASES, "placed": PLACED}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
