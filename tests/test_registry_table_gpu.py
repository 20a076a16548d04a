"""The GPU registry table (K5/K6/K7, csrc/hip/registry_table.hip) and its compiled forms
against the probe-free model of ``_registry_model.py``, on the hostile tables the CPU
table was checked on in ``test_registry_model.py``.

After every op the slot image is read back and checked as an open-addressing table --
one slot per key, every live key reachable from its probe start, value word and deadline
under the key, the counters -- and against the CPU table run through the same ops (the
set of occupied slots, the generation).  The route directory, the rank byte table, the
presence map and the affine verdict are compared with the model word for word.  All
comparisons are exact."""
import numpy as np
import pytest
import torch

import _registry_model as RM
from ptype_amd.ops import _ptr, _stream, hip
from ptype_amd.ops import table as T
from ptype_amd.ops.table import RegistryTable

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U32 = RM.U32
DIR_SIZES = [1, 15, 16, 17, 63, 64, 65, 4096, 1 << 18, (1 << 18) + 1]


def i64(x):
    return torch.tensor(list(x), dtype=torch.int64)


def pack_rows(ent, exp):
    ent, exp = ent.cpu(), exp.cpu()
    v = ent[:, 1]
    return sorted(zip(ent[:, 0].tolist(), (v & U32).tolist(), ((v >> 32) & U32).tolist(), exp.tolist()))


def image(t):
    tab = t.table.cpu().numpy()
    return tab[:, 0].copy(), tab[:, 1].copy(), t.expiry.cpu().numpy(), t.stats.cpu().numpy()


def check_image(g, model, c=None, what=""):
    """The slot image of `g` as a table holding exactly the model (and, with the CPU
    table `c` of the same op sequence, the same occupied slots and generation)."""
    keys, vals, exp, stats = image(g)
    cap = g.cap
    assert keys.shape[0] == cap == model.cap, what
    live = (keys != 0) & (keys != -1)
    slot = np.nonzero(live)[0]
    lk = keys[slot]
    assert np.unique(lk).shape[0] == lk.shape[0], f"{what}: a key sits in two slots"
    mk = np.fromiter(model.d.keys(), dtype=np.int64, count=len(model.d))
    assert np.array_equal(np.sort(lk), np.sort(mk)), f"{what}: live key set"
    # reachable: no EMPTY slot in [probe start, slot), cyclically
    start = T.probe_start(T.mix64(lk.view(np.uint64)), cap - 1).astype(np.int64)
    empties = np.concatenate([[0], np.cumsum(keys == 0)])
    between = np.where(slot >= start, empties[slot] - empties[start], empties[cap] - empties[start] + empties[slot])
    assert not between.any(), f"{what}: unreachable keys {lk[between != 0][:5]}"
    # the value word and the deadline under each key
    hit, r, m = model._find(lk)
    assert hit.all()
    assert np.array_equal(vals[slot].view(np.uint64), (r | (m << 32)).astype(np.uint64)), f"{what}: value words"
    want_exp = np.array([model.d[k][2] for k in lk.tolist()], dtype=np.int64)
    assert np.array_equal(exp[slot], want_exp), f"{what}: deadlines"
    ntomb = int((keys == -1).sum())
    assert int(stats[T.STAT_LIVE]) == len(model.d), what
    assert int(stats[T.STAT_TOMB]) == ntomb == model.tombstones, what
    dist = (slot - start) & (cap - 1)
    assert (int(dist.max()) if dist.size else 0) <= int(stats[T.STAT_MAXPROBE]) <= cap - 1, what
    assert int(stats[T.STAT_GEN]) == model.generation, what
    if c is not None:
        ck = c.table[:, 0].numpy()
        assert np.array_equal(keys != 0, ck != 0), f"{what}: occupied slots differ from the CPU table's"
        assert g.generation == c.generation, what


def check_answers(g, model, keys, what=""):
    k = torch.tensor(sorted(set(keys)), dtype=torch.int64)
    r, m = g.lookup(k)
    mr, mm = model.lookup(k.numpy())
    assert np.array_equal(r.cpu().numpy(), mr) and np.array_equal(m.cpu().numpy(), mm), f"{what}: lookup"
    assert pack_rows(*g.pack()) == model.pack(), f"{what}: pack"


def check_forms(g, model, n, ranks=(0,), what=""):
    g.enable_directory(n)
    for rank in ranks:
        g.set_presence_rank(rank)
        d, dn, aff = g.directory()
        assert dn == n and aff == 0
        assert np.array_equal(d.cpu().numpy().view(np.uint32), model.dir_words(n)), f"{what} n={n}: dir"
        assert np.array_equal(g.dir_rank.cpu().numpy(), model.rank_bytes(n)), f"{what} n={n}: dir_rank"
        if n > RM.PRESENCE_MAX_IDS:
            assert g.presence is None
        else:
            assert np.array_equal(g.presence.cpu().numpy().view(np.uint32), model.presence(n, rank)), \
                f"{what} n={n} rank={rank}: presence"


def run_scenario(name):
    """(gpu table, cpu table, model, keys seen) after the scenario's ops, checked after each."""
    sc = RM.scenarios()[name]
    g, c = RegistryTable(sc["cap"], device=DEV), RegistryTable(sc["cap"], device="cpu")
    m, cm = RM.Model(sc["cap"]), RM.Model(sc["cap"])
    seen = list(sc["absent"]) + [0, -1]
    for i, op in enumerate(sc["ops"]):
        what = f"{name} op {i} {op[0]}"
        seen += RM.op_keys(op)
        RM.drive(g, m, op)  # (the found flags are checked in there)
        RM.drive(c, cm, op)
        check_image(g, m, c, what)
        check_answers(g, m, seen, what)
    return g, c, m, seen


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("name", sorted(RM.scenarios()))
def test_gpu_table_scenarios(name):
    g, c, m, seen = run_scenario(name)
    g.rebuild()
    c.rebuild()
    m.rebuild()
    check_image(g, m, c, "rebuild")
    check_answers(g, m, seen, "rebuild")
    assert g.tombstones == 0


@pytest.mark.parametrize("seed,cap", [(1, 16), (3, 64)])
def test_gpu_table_random_ops(seed, cap):
    ops, pool = RM.random_ops(seed)
    g, c, m, cm = RegistryTable(cap, device=DEV), RegistryTable(cap, device="cpu"), RM.Model(cap), RM.Model(cap)
    for i, op in enumerate(ops):
        RM.drive(g, m, op)
        RM.drive(c, cm, op)
        check_image(g, m, c, f"seed {seed} op {i} {op}")
    check_answers(g, m, pool, f"seed {seed}")


def test_gpu_table_full():
    """A table with no empty slot: 20 distinct keys into 16 slots through the raw kernel
    (no growth check).  16 are kept, 4 are dropped silently, every probe loop ends."""
    g = RegistryTable(16, device=DEV)
    n = len(RM.FULL_KEYS)
    k = i64(RM.FULL_KEYS).to(DEV)
    ranks = (torch.arange(n, dtype=torch.int32) % 3).to(DEV)
    mbox = (torch.arange(n, dtype=torch.int32) + 50).to(DEV)
    exp = (torch.arange(n, dtype=torch.int64) + 7).to(DEV)
    hip().table_upsert(_ptr(g.table), g.cap, _ptr(k), _ptr(ranks), _ptr(mbox), _ptr(exp), _ptr(g.expiry), n,
                       _ptr(g.stats), _stream(g.table))
    assert g.live == 16 and g.tombstones == 0
    r, mb = g.lookup(k)
    held = (r >= 0).cpu()
    assert int(held.sum()) == 16 and bool((mb.cpu()[~held] == -1).all())
    m = RM.Model(16)
    m.d = {int(k[i]): (int(ranks[i]), int(mbox[i]), int(exp[i])) for i in range(n) if held[i]}
    m.generation = 1
    check_image(g, m, None, "full")
    absent = RM._ids([1, 2, 99999])
    check_answers(g, m, RM.FULL_KEYS + absent, "full")
    gone = i64(absent + [RM.FULL_KEYS[i] for i in range(n) if not held[i]])
    assert g.delete(gone).tolist() == [False] * 7
    m.generation += 1
    check_image(g, m, None, "full, after deleting absent keys")


def test_gpu_table_grid_stride_second_trips():
    """Capacity 2^22 and batches past one trip of every grid-stride loop: upsert and delete
    of 131073 keys (512 x 256 + 1), a lookup of 2^20 + 1 keys (4096 x 256 + 1), and sweep,
    directory build and pack over 2^22 slots (4 trips of 4096 x 256, 2 of 1024 x 2048)."""
    n, cap = 512 * 256 + 1, 1 << 22
    g, m = RegistryTable(cap, device=DEV), RM.Model(cap)
    ids = np.arange(n, dtype=np.int64) * 31 + 5
    keys = ids + 1
    rng = np.random.default_rng(7)
    ranks, mbox = rng.integers(0, 300, n), rng.integers(0, 1 << 25, n)
    dl = rng.integers(0, 3, n) * 1000  # 0: never, 1000: swept at now = 1001, 2000: stays
    RM.drive(g, m, ("upsert", keys.tolist(), ranks.tolist(), mbox.tolist(), dl.tolist()))
    check_image(g, m, None, "trips upsert")
    q = np.concatenate([keys, rng.integers(1, 1 << 40, (1 << 20) + 1 - n)])
    r, mb = g.lookup(torch.from_numpy(q))
    mr, mm = m.lookup(q)
    assert np.array_equal(r.cpu().numpy(), mr) and np.array_equal(mb.cpu().numpy(), mm)
    RM.drive(g, m, ("sweep", 1001))
    check_image(g, m, None, "trips sweep")
    assert pack_rows(*g.pack()) == m.pack()
    check_forms(g, m, 1 << 18, what="trips")
    dk = np.concatenate([keys[::2], keys[1::4] + 1])[:n]  # present, swept and never-registered keys
    dk = np.concatenate([dk, np.full(n - dk.shape[0], 3, dtype=np.int64)])
    found = g.delete(torch.from_numpy(dk)).cpu().numpy()
    _, first = np.unique(dk, return_index=True)
    want = m.delete(dk)
    assert np.array_equal(found[first], want[first]) and int(found.sum()) == int(want.sum())
    check_image(g, m, None, "trips delete")
    assert pack_rows(*g.pack()) == m.pack()


# ---------------------------------------------------------------- snapshot restore
def test_gpu_snapshot_restore_and_rebuild():
    g, _, m, seen = run_scenario("tombs")
    assert g.tombstones == 5
    ent, exp = g.snapshot_to_host()
    assert pack_rows(ent, exp) == m.pack()
    for cap in (16, 64, 256):  # smaller (grows), equal, larger
        g2, m2 = RegistryTable(cap, device=DEV), RM.Model(cap)
        g2.load_packed(ent, exp)
        m2.load_packed(m.pack())
        assert g2.cap == m2.cap
        check_image(g2, m2, None, f"restore into {cap}")
        check_answers(g2, m2, seen, f"restore into {cap}")
    g.rebuild()
    m.rebuild()
    assert g.tombstones == 0
    check_image(g, m, None, "rebuild")
    check_answers(g, m, seen, "rebuild")


# ---------------------------------------------------------------- pack shapes
def _ids_by_group(cap, groups, per_group, scan=200_000):
    """`per_group` actor ids for each probe-start group of `groups` at capacity `cap`."""
    ids = np.arange(scan, dtype=np.int64)
    start = T.probe_start(T.mix64((ids + 1).astype(np.uint64)), cap - 1).astype(np.int64)
    out = []
    for gstart in groups:
        got = ids[start == gstart][:per_group]
        assert got.shape[0] == per_group
        out += got.tolist()
    return out


@pytest.mark.parametrize("shape", ["partial_tile", "last_256", "wave_full_wave_empty"])
def test_gpu_pack_shapes(shape):
    if shape == "partial_tile":  # capacity 16: 16 slots of the first 2048-slot tile
        cap, ids = 16, [0, 1, 2, 3, 4]
    elif shape == "last_256":  # live entries only in the last 256 of 4096 slots
        cap, ids = 4096, _ids_by_group(4096, range(3840, 4096, 8), 3)
    else:  # slots 0..63 all live (four keys per group of four), slots 64.. all empty
        cap, ids = 256, _ids_by_group(256, range(0, 64, 4), 4)
    g, m = RegistryTable(cap, device=DEV), RM.Model(cap)
    n = len(ids)
    RM.drive(g, m, ("upsert", RM._ids(ids), [i % 5 for i in range(n)], [1000 + i for i in range(n)],
                    [0 if i % 3 else 50 + i for i in range(n)]))
    keys = image(g)[0]
    used = set(np.nonzero(keys)[0].tolist())
    if shape == "last_256":
        assert min(used) >= 3840
    elif shape == "wave_full_wave_empty":
        assert used == set(range(64))
    check_image(g, m, None, shape)
    check_answers(g, m, RM._ids(ids), shape)
    ent, exp = g.snapshot_to_host()
    assert pack_rows(ent, exp) == m.pack()


# ---------------------------------------------------------------- compiled forms
@pytest.mark.parametrize("name", sorted(RM.scenarios()))
def test_gpu_directory_forms(name):
    g, _, m, _ = run_scenario(name)
    for n in DIR_SIZES:
        check_forms(g, m, n, ranks=(0, 1, 0xFD), what=name)


def test_gpu_directory_forms_follow_every_mutation():
    g, _, m, _ = run_scenario("values")
    g.enable_directory(65)
    step = lambda what: check_forms(g, m, 65, ranks=(g.presence_rank,), what=what)
    step("built")
    RM.drive(g, m, ("upsert", RM._ids([3, 40, 64, 65]), [1, 1, 0xFD, 1], [9, 1 << 24, 9, 9], None))
    step("upsert")
    RM.drive(g, m, ("delete", RM._ids([0, 40])))
    step("delete")
    RM.drive(g, m, ("upsert", RM._ids([50, 51]), [1, 1], [1, 2], [10, 20]))
    RM.drive(g, m, ("sweep", 15))
    step("sweep")
    ent, exp = g.snapshot_to_host()
    ent, exp, rows = ent.clone(), exp.clone(), m.pack()
    RM.drive(g, m, ("clear",))
    step("clear")
    assert not m.d and bool((g.dir.cpu() == -1).all())
    g.load_packed(ent, exp)
    m.load_packed(rows)
    step("load_packed")
    RM.drive(g, m, ("delete", RM._ids([5])))
    RM.drive(g, m, ("rebuild",))
    step("rebuild")
    for rank in (1, 0xFD, 0):
        g.set_presence_rank(rank)
        step(f"set_presence_rank({rank})")
    check_image(g, m, None, "after the mutations")


@pytest.mark.parametrize("W,n", [(1, 50), (3, 50), (8, 50)])
def test_gpu_affine_verdict(W, n):
    g, m = RegistryTable(256, device=DEV), RM.Model(256)
    g.enable_directory(n, affine_world=W)

    def verdict(want, what):
        assert m.affine(n, W) == want, what
        assert g.directory()[2] == (W if want else 0), what

    ids = list(range(n))
    RM.drive(g, m, ("upsert", RM._ids(ids), [i % W for i in ids], [i // W for i in ids], None))
    verdict(True, "strided placement")
    RM.drive(g, m, ("upsert", RM._ids([n, n + 7]), [W + 1, 0], [12345, 0], None))  # misplaced, outside [0, n)
    verdict(True, "a misplaced id outside the range")
    RM.drive(g, m, ("upsert", RM._ids([17]), [(17 % W) + 1], [17 // W], None))
    verdict(False, "one id re-homed to another rank")
    RM.drive(g, m, ("upsert", RM._ids([17]), [17 % W], [17 // W], None))
    verdict(True, "repaired")
    RM.drive(g, m, ("upsert", RM._ids([n - 1]), [(n - 1) % W], [(n - 1) // W + 1], None))
    verdict(False, "the last id in another mailbox")
    RM.drive(g, m, ("upsert", RM._ids([n - 1]), [(n - 1) % W], [(n - 1) // W], None))
    verdict(True, "repaired")
    RM.drive(g, m, ("delete", RM._ids([n - 1])))
    verdict(False, "the last id deleted")
    RM.drive(g, m, ("upsert", RM._ids([n - 1]), [(n - 1) % W], [(n - 1) // W], None))
    verdict(True, "registered again")
    RM.drive(g, m, ("delete", RM._ids([n + 7])))
    verdict(True, "an id outside the range deleted")
