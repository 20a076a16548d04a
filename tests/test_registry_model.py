"""The CPU registry table against the probe-free model of ``_registry_model.py``.

Every hostile scenario (wrapped probe chains, tombstones inside a chain, the growth
threshold, values that fit no route word, keys at the edges of the key space, deadlines
on the sweep boundary, duplicate keys, a table with no empty slot) and a few hundred
fixed-seed mixed ops run on ``RegistryTable(device="cpu")``; after every op the lookups
of every key seen so far and of absent keys, the found flags, ``live``, ``tombstones``,
the generation, the capacity and the pack multiset with deadlines equal the model's.
This is what lets the GPU tests take the CPU table and the CPU ``B.route`` as references
on these tables.  The model's own directory forms are pinned by hand first."""
import numpy as np
import pytest
import torch

import _registry_model as RM
from ptype_amd.ops import batch as B
from ptype_amd.ops import table as T
from ptype_amd.ops.records import METHOD_ECHO
from ptype_amd.ops.table import RegistryTable

U32 = RM.U32


def pack_rows(table):
    ent, exp = table.pack()
    ent, exp = ent.cpu(), exp.cpu()
    v = ent[:, 1]
    return sorted(zip(ent[:, 0].tolist(), (v & U32).tolist(), ((v >> 32) & U32).tolist(), exp.tolist()))


def check(table, model, keys, what=""):
    k = torch.tensor(sorted(set(keys)), dtype=torch.int64)
    r, m = table.lookup(k)
    mr, mm = model.lookup(k.numpy())
    assert r.cpu().tolist() == mr.tolist() and m.cpu().tolist() == mm.tolist(), what
    assert (table.live, table.tombstones, table.cap) == (model.live, model.tombstones, model.cap), what
    assert table.generation == model.generation, what
    assert pack_rows(table) == model.pack(), what


def slots_of(table):
    """{key: slot} of the live keys, the TOMB slots and the set of non-empty slots."""
    k = table.table[:, 0].cpu().tolist()
    live = {key: s for s, key in enumerate(k) if key not in (0, -1)}
    assert len(live) == sum(1 for key in k if key not in (0, -1))  # no key in two slots
    return live, {s for s, key in enumerate(k) if key == -1}, {s for s, key in enumerate(k) if key != 0}


# ---------------------------------------------------------------- the model, by hand
def test_model_forms_by_hand():
    m = RM.Model(16)
    m.upsert([1, 2, 4, 5, 6, 18, 0, -1], [0, 0xFD, 0xFE, 1, 2, 1, 7, 7], [5, (1 << 24) - 1, 3, 1 << 24, 0, 9, 7, 7])
    assert m.live == 6 and m.generation == 1
    assert m.dir_words(6).tolist() == [0x500, 0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE, 0x002]
    assert m.rank_bytes(6).tolist() == [0, 0xFD, 0xFF, 0xFE, 1, 2]
    p = m.presence(18, 1)
    assert p.shape[0] == 4  # (2 words of fields, rounded up to 4)
    # ids 0..5: ranks 0, fd, absent, fe (probe), 1 (here), 2; id 17: rank 1 (here)
    assert p.tolist() == [(2 << 6) | (1 << 8), 1 << 2, 0, 0]
    assert m.presence(6, 0xFD).tolist() == [(1 << 2) | (2 << 6), 0, 0, 0]
    assert m.presence(1, 0).shape[0] == 4 and m.presence(65, 0).shape[0] == 8 and m.presence(64, 0).shape[0] == 4
    assert m.resolve(0) == (0, 5) and m.resolve(2) is None and m.resolve(3) == (0xFE, 3)
    r, mb = m.resolve_many([0, 2, 3, 0xFFFFFFFF])
    assert r.tolist() == [0, -1, 0xFE, -1] and mb.tolist() == [5, 0, 3, 0]
    a = RM.Model(16)
    a.upsert([1, 2, 3, 4, 5, 9], [0, 1, 2, 0, 1, 0], [0, 0, 0, 1, 1, 77])
    assert a.affine(5, 3) and not a.affine(6, 3) and not a.affine(5, 2)
    a.upsert([3], [2], [1])
    assert not a.affine(5, 3) and a.affine(2, 3)


def test_model_field_ffffffff_names_no_actor():
    m = RM.Model(16)
    m.upsert([1 << 32, (1 << 32) - 1], [0, 0], [7, 6])
    assert m.lookup([1 << 32])[1].tolist() == [7]  # registrable
    assert m.resolve(0xFFFFFFFF) is None and m.resolve(0xFFFFFFFE) == (0, 6)  # never addressable


def test_model_hash_free_constants_match_the_table():
    for s in ("", "a", "calculator/node0", "calculator/node1", "optimus/worker2"):
        assert RM.fnv1a64(s) == T.fnv1a64(s)
    assert len(set(RM.service_keys())) == 2 and all(k < -2 for k in RM.service_keys())
    ids = np.arange(200)
    start = T.probe_start(T.mix64((ids + 1).astype(np.uint64)), 63)
    assert ids[start == 60][:12].tolist() == RM.WRAP_IDS
    assert RM.MAX_MBOX == B.MAX_MBOX


# ---------------------------------------------------------------- scenarios
@pytest.mark.parametrize("name", sorted(RM.scenarios()))
def test_cpu_table_matches_model(name):
    sc = RM.scenarios()[name]
    t, m = RegistryTable(sc["cap"], device="cpu"), RM.Model(sc["cap"])
    seen = list(sc["absent"]) + [0, -1]
    check(t, m, seen, "empty")
    for i, op in enumerate(sc["ops"]):
        seen += RM.op_keys(op)
        RM.drive(t, m, op)
        check(t, m, seen, f"{name} op {i} {op[0]}")
    t.rebuild()
    m.rebuild()
    check(t, m, seen, "rebuild")
    assert t.tombstones == 0


def test_cpu_wrap_and_tombs_slot_images():
    """What the scenario notes claim: the chain wraps, a re-upsert passes the tombstones."""
    sc = RM.scenarios()["tombs"]
    t, m = RegistryTable(64, device="cpu"), RM.Model(64)
    RM.drive(t, m, sc["ops"][0])
    live, tomb, used = slots_of(t)
    assert used == {60, 61, 62, 63, 0, 1, 2, 3, 4, 5, 6, 7} and int(t.stats[T.STAT_MAXPROBE]) == 11
    RM.drive(t, m, sc["ops"][1])
    RM.drive(t, m, sc["ops"][2])
    live, tomb, used = slots_of(t)
    assert live[RM.key_of(RM.WRAP_IDS[3])] == 8 and int(t.stats[T.STAT_MAXPROBE]) == 12 and len(tomb) == 2
    RM.drive(t, m, sc["ops"][3])
    live, tomb, used = slots_of(t)
    assert len(tomb) == 5 and tomb < {60, 61, 62, 63, 0, 1, 2, 3} and len(live) == 8
    check(t, m, RM.op_keys(sc["ops"][0]), "after the sweep")


def test_cpu_threshold_growth():
    sc = RM.scenarios()["threshold"]
    t, m = RegistryTable(16, device="cpu"), RM.Model(16)
    RM.drive(t, m, sc["ops"][0])
    assert t.cap == m.cap == 16 and t.live == 12
    RM.drive(t, m, sc["ops"][1])
    assert t.cap == m.cap == 32 and t.live == 13


def test_cpu_full_table_drops_silently():
    t = RegistryTable(16, device="cpu")
    k = torch.tensor(RM.FULL_KEYS, dtype=torch.int64)
    n = k.numel()
    t._cpu_upsert(k, torch.arange(n, dtype=torch.int32) % 3, torch.arange(n, dtype=torch.int32) + 50,
                  torch.arange(n, dtype=torch.int64) + 7)  # (no growth check)
    assert t.live == 16 and t.tombstones == 0
    r, mb = t.lookup(k)
    held = r >= 0
    assert int(held.sum()) == 16 and bool((mb[~held] == -1).all())
    m = RM.Model(64)
    m.upsert(k[held], (torch.arange(n) % 3)[held], (torch.arange(n) + 50)[held], (torch.arange(n) + 7)[held])
    absent = torch.tensor(RM._ids([1, 2, 99999]), dtype=torch.int64)
    mr, mm = m.lookup(torch.cat([k, absent]).numpy())
    r, mb = t.lookup(torch.cat([k, absent]))
    assert r.tolist() == mr.tolist() and mb.tolist() == mm.tolist()
    assert pack_rows(t) == m.pack()
    assert t.delete(torch.cat([absent, k[~held]])).tolist() == [False] * (3 + 4)
    assert t.live == 16 and t.tombstones == 0


@pytest.mark.parametrize("seed,cap", [(1, 16), (2, 32), (3, 64)])
def test_cpu_random_ops_match_model(seed, cap):
    ops, pool = RM.random_ops(seed)
    t, m = RegistryTable(cap, device="cpu"), RM.Model(cap)
    kinds = set()
    for i, op in enumerate(ops):
        RM.drive(t, m, op)
        kinds.add(op[0])
        check(t, m, pool + [RM.key_of(5000)], f"seed {seed} op {i} {op}")
    assert kinds >= {"upsert", "delete", "sweep", "rebuild"} and m.cap > cap  # it grew on the way


def test_generation_counts_calls_not_changes():
    t, m = RegistryTable(16, device="cpu"), RM.Model(16)
    e = torch.zeros(0, dtype=torch.int64)
    t.upsert(e, e.to(torch.int32), e.to(torch.int32))
    t.delete(e)
    assert t.generation == 0  # no rows: left alone
    for op in [("upsert", [0, -1], [1, 1], [1, 1], None), ("delete", RM._ids([77])), ("sweep", 5), ("clear",),
               ("upsert", RM._ids([1]), [0], [1], None), ("upsert", RM._ids([1]), [0], [1], None), ("rebuild",)]:
        RM.drive(t, m, op)
    assert t.generation == m.generation == 8 and t.live == 1


# ---------------------------------------------------------------- the CPU route as a reference
def test_cpu_route_follows_model_resolution():
    """B.route on the CPU table: a message is delivered iff the model resolves its actor
    field to a rank below R and a mailbox below 2^24; the field 0xffffffff never is."""
    sc = RM.scenarios()["keys"]
    t, m = RegistryTable(16, device="cpu"), RM.Model(16)
    for op in sc["ops"]:
        RM.drive(t, m, op)
    assert m.lookup([1 << 32])[0].tolist() == [0]  # id 2^32 - 1 is registered at rank 0
    actors = torch.tensor([0, 0xFFFFFFFF, 0xFFFFFFFE, 1, 0xFFFFFFFF], dtype=torch.int64)
    req = B.MsgBatch(actors.to(torch.int32), torch.arange(5), None, None, METHOD_ECHO)
    _, perm, stats = B.route(req, t, 2, 8)
    rank, mbox = m.resolve_many(actors.numpy())
    want = (rank >= 0) & (rank < 2) & (mbox < RM.MAX_MBOX)
    assert ((perm >= 0).numpy() == want).all() and perm.tolist() == [0, -2, 1, -2, -2]
    assert int(stats[B.STAT_NOMATCH]) == 3
