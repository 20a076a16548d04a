"""The persistent sort's tile loop and the ring drain's write-out after their memory
waits were moved (profiles/sort_drain_waits.md): the next tile's arguments are loaded
right behind a tile's record stores, a whole tile's arguments are loaded without bounds
branches, the spill vote is one flag word behind one barrier, and the drain stages its
replies into registers before it stores them.

As in test_mailbox_persist_gpu.py the same inputs go through ``mbox_persist=1`` and
``mbox_persist=0``, each in a child process, and must give the same replies, statuses
and mailbox statistics; every reply is also compared exactly against ``a0 * a1`` /
``STATUS_NO_ACTOR`` computed in torch.  The table is that file's: registered,
directory-only, hash-probed and unknown ids, so absent replies interleave with present
ones in every tile.

Shapes (the persistent kernel takes a Send of more than 512 tiles of 4096):

* ``520 * 4096``: every tile whole, the tile count a multiple of 8 (tiles dealt XCD by
  XCD), blocks of one and of two tiles -- only the whole-tile path runs;
* ``512 * 4096 + 1``: the 513th tile holds one message, as some block's second tile:
  the guarded path behind the whole-tile one, its hoisted loads past ``M``;
* ``1027 * 4096 + 4095``: a tile count that is no multiple of 8 (tile ``b + i * G``),
  two to three tiles per block, the last tile one message short.

The spill vote: exactly one message gets a field wider than the 8-B widths in force
(``a0 = 2^40 + 3``, after a Send that set the widths), in a tile that is some block's
first tile, then its last, by the dealing rule in the kernel's comment (grid ``G`` = 2
blocks per CU, capped at the tile count, a multiple of 8; with ``T % 8 == 0`` block
``b`` takes tiles ``(b % 8) * T/8 + b/8 + i * G/8``, otherwise ``b + i * G``); a second
wide message sits in lane 0 of wave 7 of another tile, so the vote must cross waves.
At 520 tiles no block of a 512-block grid has three tiles, so the middle-tile run uses
the 1028-tile shape (tiles ``b``, ``b + G``, ``b + 2G``).  A missed vote leaves a
spilled message unanswered and a tile after a spilled one must still be answered: every
reply is checked, ``spilled > 0``."""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import ROOT

TILE = 4096
M_FULL = 520 * TILE
M_LAST1 = 512 * TILE + 1
M_SHORT = 1027 * TILE + 4095

CHILD = textwrap.dedent('''
    import json, sys
    import torch
    from ptype_amd.ops import batch as B
    from ptype_amd.ops.mailbox import Mailboxes
    from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_NO_ACTOR, STATUS_OK
    from ptype_amd.ops.table import RegistryTable, actor_keys
    from ptype_amd.parallel.exchange import ActorExchange

    case, out_path = sys.argv[1], sys.argv[2]
    DEV = torch.device("cuda", 0)
    TILE = 4096
    n = 1 << 15
    t = RegistryTable(4 * n, device=DEV)
    ids = torch.cat([torch.arange(n), torch.arange(n + 100, n + 1100)])
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(31))
    t.upsert(actor_keys(ids), torch.zeros(ids.numel(), dtype=torch.int32), perm.to(torch.int32))
    t.enable_directory(n + 50)  # ids n..n+49: in the directory, unregistered; n+100..: hash probes

    def known_of(actor):
        return (actor < n) | ((actor >= n + 100) & (actor < n + 1100))

    def batch(M, seed, lo=-(1 << 15), hi=1 << 15):
        g = torch.Generator().manual_seed(seed)
        actor = torch.randint(0, n + 3000, (M,), generator=g, dtype=torch.int32).to(DEV)
        a0 = torch.randint(lo, hi, (M,), generator=g, dtype=torch.int64).to(DEV)
        a1 = torch.randint(lo, hi, (M,), generator=g, dtype=torch.int64).to(DEV)
        return B.MsgBatch(actor, a0, a1, None, METHOD_CALC_MULTIPLY)

    vals, sts, rec_bytes, all_stats = [], [], [], []
    STAT_KEYS = ("enqueued", "processed", "spilled", "overflow", "no_actor", "holes")

    def check(req, val, st, mb, keep=True):
        known = known_of(req.actor)
        assert torch.equal(st, torch.where(known, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
        assert torch.equal(val[known], (req.a0 * req.a1)[known])
        if not keep:
            return
        vals.append(val.cpu())  # (an unanswered message's value is written too: 0 beside its status)
        sts.append(st.cpu())
        rec_bytes.append(int(mb.last_record_bytes))

    def send(mb, req, route4=True, keep=True):
        val, st = mb.send(req, t, None, ordered=False)
        torch.cuda.synchronize()
        if route4:
            assert mb.last_route == 4, mb.last_route
        check(req, val, st, mb, keep)

    def finish(mb):  # every ring drained (head == tail), no hole; the mailboxes' statistics kept
        ctr = mb.shard_counters()
        assert (ctr[:, 0] == ctr[:, 2]).all(), ctr
        s = mb.stats()
        assert s["holes"] == 0, s
        all_stats.append({k: s[k] for k in STAT_KEYS})
        return s

    def dealt_tiles(T):
        """The tiles of block 0 of the persistent grid, by the rule in the kernel's comment."""
        G = min(2 * torch.cuda.get_device_properties(0).multi_processor_count, T)
        if G >= 8:
            G -= G % 8
        if G >= 8 and T % 8 == 0:
            return list(range(0, T // 8, G // 8)), G
        return list(range(0, T, G)), G

    if case.startswith("m"):  # m<M>x<sends>: plain Sends of M messages on one Mailboxes
        M, sends = (int(x) for x in case[1:].split("x"))
        mb = Mailboxes(DEV, shards=256, slots=1 << 16)
        for k in range(sends):
            send(mb, batch(M, 32 + k))
        finish(mb)
    elif case.startswith("vote"):  # vote<M>: wide messages in block 0's first and last (or its middle) tile
        M = int(case[4:])
        T = (M + TILE - 1) // TILE
        mine, G = dealt_tiles(T)
        assert len(mine) >= 2, (mine, G)  # (more tiles than resident blocks)
        picks = [mine[0], mine[-1]] if len(mine) == 2 else [mine[len(mine) // 2]]
        req = batch(M, 70)
        for k, tile in enumerate(picks):
            other = mine[-1] + 1 if k == 0 else mine[0] + 1  # a tile of another block
            q = B.MsgBatch(req.actor.clone(), req.a0.clone(), req.a1, None, METHOD_CALC_MULTIPLY)
            q.actor[tile * TILE + 5] = 17  # (registered ids: the wide messages are delivered, not missed)
            q.a0[tile * TILE + 5] = (1 << 40) + 3
            q.actor[other * TILE + 7 * 512] = 18  # lane 0 of wave 7
            q.a0[other * TILE + 7 * 512] = (1 << 40) + 3
            mb = Mailboxes(DEV, shards=256, slots=1 << 16)
            send(mb, req, keep=False)  # (sets the 8-B widths in force: 2^40 does not fit them)
            assert mb.stats()["spilled"] == 0
            send(mb, q)
            s = finish(mb)
            assert s["spilled"] > 0 and s["overflow"] == 0, s
        assert rec_bytes == [8] * len(picks), rec_bytes
    elif case == "graph":
        # the bench's step at the whole-tile shape: requests regenerated from a device seed, two steps per replay
        M, U = 520 * TILE, 2
        ex = ActorExchange(t, M, chunks=1, delivery="mailbox", mailbox_shards=256, mailbox_slots=1 << 16)
        rq = B.MsgBatch(torch.empty(M, dtype=torch.int32, device=DEV), torch.empty(M, dtype=torch.int64, device=DEV),
                        torch.empty(M, dtype=torch.int64, device=DEV), None, METHOD_CALC_MULTIPLY)
        val = torch.empty(M, dtype=torch.int64, device=DEV)
        st = torch.empty(M, dtype=torch.int32, device=DEV)
        seed_t = torch.tensor([7 + j * 0x1000193 for j in range(U)], dtype=torch.int64, device=DEV)

        def prologue(j=0):
            B.gen_requests(M, n + 3000, METHOD_CALC_MULTIPLY, device=DEV, out=rq, seed_tensor=seed_t[j:j + 1])
            if j == U - 1:
                seed_t.add_(U * 0x1000193)

        graph = ex.capture(rq, val, st, prologue=prologue, repeat=U)
        mb = ex.mailboxes  # (built by the capture's warm-up Send)
        for k in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert mb.last_route == 4, mb.last_route
            check(rq, val, st, mb)
        finish(mb)
    elif case == "fused":  # the fused sort + drain shares drain_ring_tile
        mb = Mailboxes(DEV, shards=256, slots=1 << 16)
        for k in range(2):
            send(mb, batch(3 * TILE + 5, 90 + k), route4=False)
        finish(mb)
    else:
        raise SystemExit("unknown case " + case)
    torch.save({"val": vals, "st": sts}, out_path)
    print("RESULT " + json.dumps({"stats": all_stats, "rec_bytes": rec_bytes}))
''')


def _run(case, tune, tmp_path, tag):
    out = tmp_path / f"{case}_{tag}.pt"
    env = dict(os.environ, PTYPE_TUNE=tune, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", CHILD, case, str(out)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and "RESULT " in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    return res, torch.load(out)


def _same(new, new_t, ref, ref_t):
    assert new["stats"] == ref["stats"], (new["stats"], ref["stats"])
    assert all(s["holes"] == 0 for s in new["stats"])
    assert new["rec_bytes"] == ref["rec_bytes"], (new["rec_bytes"], ref["rec_bytes"])
    assert len(new_t["val"]) == len(ref_t["val"]) > 0
    for k, (a, b) in enumerate(zip(new_t["val"], ref_t["val"])):
        assert torch.equal(a, b), k
    for k, (a, b) in enumerate(zip(new_t["st"], ref_t["st"])):
        assert torch.equal(a, b), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", [f"m{M_FULL}x1", f"m{M_LAST1}x1", f"m{M_SHORT}x1", f"m{M_LAST1}x2",
                                  f"vote{M_FULL}", f"vote{M_SHORT}", "graph"])
def test_sort_waits_persistent_matches_one_block_per_tile(case, tmp_path):
    new, new_t = _run(case, "mbox_fused=0,mbox_rec8=1,mbox_persist=1", tmp_path, "p1")
    ref, ref_t = _run(case, "mbox_fused=0,mbox_rec8=1,mbox_persist=0", tmp_path, "p0")
    _same(new, new_t, ref, ref_t)
    if case.startswith("vote"):
        assert all(s["spilled"] > 0 for s in new["stats"]), new["stats"]


@pytest.mark.gpu
def test_sort_waits_fused_kernel_matches_separate_kernels(tmp_path):
    new, new_t = _run("fused", "mbox_fused=1,mbox_rec8=1", tmp_path, "f1")
    ref, ref_t = _run("fused", "mbox_fused=0,mbox_rec8=1,mbox_persist=0", tmp_path, "f0")
    _same(new, new_t, ref, ref_t)


# Occupancy [waves/SIMD] of every instantiation at the parent commit (the same compiler, gfx950), keyed by the
# kernel's template arguments: mbx_drain_ring_kernel<FIXED, NARROW, RF, SK> and
# mbx_sortdrain_kernel<MODE, A2, MC, FIXED, RF, SK>.
PARENT_OCCUPANCY = {
    "mbx_drain_ring_kernel": {
        (0, 1, 0, 8): 6, (0, 1, 1, 8): 7, (0, 1, 2, 8): 7,
        (1, 1, 0, 8): 8, (1, 1, 1, 8): 8, (1, 1, 2, 8): 8,
    },
    "mbx_sortdrain_kernel": {
        **{(mode, 0, 0, fixed, rf, 8): 4 for mode in (0, 1, 2, 3) for fixed in (0, 1) for rf in (0, 1)},
        (3, 0, 0, 0, 2, 8): 4, (3, 0, 0, 1, 2, 8): 4,
        **{(mode, 0, 1, 0, 0, 8): 4 for mode in (0, 1, 2)},
        **{(mode, 1, 0, fixed, 0, 8): 4 for mode in (0, 1, 2) for fixed in (0, 1)},
        **{(mode, 1, 1, 0, 0, 8): 3 for mode in (0, 1, 2)},
    },
}


def test_sort_waits_drain_kernel_resources():
    """No drain or fused kernel took scratch or lost occupancy to the staged write-out, and the
    NARROW && FIXED ring drains still fit their launch bounds (64 VGPRs, 8 waves per SIMD)."""
    import re

    from ptype_amd import _build

    _build.build_hip()
    seen = {k: set() for k in PARENT_OCCUPANCY}
    for name, r in _build.kernel_resources().items():
        m = re.search(r"(mbx_drain_ring_kernel|mbx_sortdrain_kernel)I((?:L[ib]\d+E)+)E", name)
        if not m:
            continue
        args = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2)))
        seen[m.group(1)].add(args)
        assert r["ScratchSize"] == 0, (name, r)
        assert args in PARENT_OCCUPANCY[m.group(1)], f"{name}: no parent figure in the table"
        assert r["Occupancy"] >= PARENT_OCCUPANCY[m.group(1)][args], (name, r)
        if m.group(1) == "mbx_drain_ring_kernel" and args[0] and args[1]:
            assert r["VGPRs"] <= 64, (name, r)
    for kernel, table in PARENT_OCCUPANCY.items():
        assert seen[kernel] == set(table), (kernel, sorted(set(table) ^ seen[kernel]))
