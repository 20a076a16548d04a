"""The persistent reserving sort (tune mbox_persist) against the one-block-per-tile
kernel it replaces for presence-map Sends (route mode 4): the same inputs through
``mbox_persist=1`` and ``mbox_persist=0``, each in a child process (the switches
are part of the child's environment), must give the same replies, statuses and
mailbox statistics.  The shapes are the smallest at which the tile loop can go
wrong: less than a tile, one message past a tile, more tiles than resident
blocks (not a multiple of the grid nor of 8, partial last tile), rings the runs
overrun, records that change width from Send to Send, and replays of a captured
step.

The table is the one of test_arrival_fused_big_batch_presence_map: a directory
of n + 50 ids, n of them registered, 1000 more registered past the directory
(hash probes), and actors drawn from [0, n + 3000) -- unregistered, probed and
unknown ids all occur."""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import ROOT

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

    def check(req, val, st, mb):
        known = known_of(req.actor)
        assert torch.equal(st, torch.where(known, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
        assert torch.equal(val[known], (req.a0 * req.a1)[known])
        vals.append(val.cpu())  # (an unanswered message's value is written too: 0 beside its status)
        sts.append(st.cpu())
        rec_bytes.append(int(mb.last_record_bytes))

    def send(mb, req):
        val, st = mb.send(req, t, None, ordered=False)
        torch.cuda.synchronize()
        assert mb.last_route == 4, mb.last_route
        check(req, val, st, mb)

    def finish(mb):  # every ring drained (head == tail), no hole; the mailboxes' statistics kept
        ctr = mb.shard_counters()
        assert (ctr[:, 0] == ctr[:, 2]).all(), ctr
        s = mb.stats()
        assert s["holes"] == 0, s
        all_stats.append({k: s[k] for k in STAT_KEYS})
        return s

    if case.startswith("m"):  # m<M>x<sends>: plain Sends of M messages
        M, sends = (int(x) for x in case[1:].split("x"))
        mb = Mailboxes(DEV, shards=256, slots=1 << 16)
        for k in range(sends):
            send(mb, batch(M, 32 + k))
    elif case == "spill":
        # runs that overrun their rings (4 x 1024 slots for 600 000 messages), then, on roomy
        # rings, records whose fields outgrow the 8-B widths for one Send: both spill
        M = 600_000
        mb = Mailboxes(DEV, shards=4, slots=1024)
        for k in range(3):
            send(mb, batch(M, 50 + k))
        s = finish(mb)
        assert s["spilled"] > 0 and s["overflow"] == 0, s
        mb = Mailboxes(DEV, shards=256, slots=16384)
        for k in range(3):
            req = batch(M, 60 + k)
            if k == 1:
                req.a0[::97] = (1 << 40) + 3
                req.a1[::89] = -(1 << 38)
            send(mb, req)
        s = mb.stats()
        assert s["spilled"] > 0 and s["overflow"] == 0, s
    elif case == "widths":
        M = 600_000
        mb = Mailboxes(DEV, shards=256, slots=16384)
        for k, wide in enumerate([False, True, True, True, False, False]):
            lo, hi = (-(1 << 63), (1 << 63) - 1) if wide else (-(1 << 15), 1 << 15)
            send(mb, batch(M, 40 + k, lo, hi))
        assert rec_bytes == [8, 8, 18, 18, 18, 8], rec_bytes
    elif case == "graph":
        # the bench's step: requests regenerated from a device seed, then the Send, two steps per replay
        M, U = (5 << 20) + 1000, 2
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
    else:
        raise SystemExit("unknown case " + case)
    finish(mb)
    torch.save({"val": vals, "st": sts}, out_path)
    print("RESULT " + json.dumps({"stats": all_stats, "rec_bytes": rec_bytes}))
''')


def _run(case, persist, tmp_path):
    out = tmp_path / f"{case}_{persist}.pt"
    env = dict(os.environ, PTYPE_TUNE=f"mbox_fused=0,mbox_rec8=1,mbox_persist={persist}",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", CHILD, case, str(out)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and "RESULT " in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    return res, torch.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["m1x1", "m4095x1", "m4097x1", f"m{(5 << 20) + 1000}x2", "spill", "widths", "graph"])
def test_persistent_sort_matches_one_block_per_tile(case, tmp_path):
    new, new_t = _run(case, 1, tmp_path)
    ref, ref_t = _run(case, 0, tmp_path)
    assert new["stats"] == ref["stats"], (new["stats"], ref["stats"])
    assert all(s["holes"] == 0 for s in new["stats"])
    assert new["rec_bytes"] == ref["rec_bytes"], (new["rec_bytes"], ref["rec_bytes"])
    assert len(new_t["val"]) == len(ref_t["val"]) > 0
    for k, (a, b) in enumerate(zip(new_t["val"], ref_t["val"])):
        assert torch.equal(a, b), k
    for k, (a, b) in enumerate(zip(new_t["st"], ref_t["st"])):
        assert torch.equal(a, b), k


def test_persistent_sort_kernel_resources():
    """Four waves per SIMD and no scratch: the register budget the kernel is built around."""
    from ptype_amd import _build

    _build.build_hip()
    res = {k: v for k, v in _build.kernel_resources().items() if "mbx_persist_sort_kernel" in k}
    assert res, "mbx_persist_sort_kernel missing from the build's resource remarks"
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["Occupancy"] >= 4 and r["VGPRs"] <= 128, (name, r)
