#!/usr/bin/env python3
"""A pool of worker actors behind a topic: queue subscriptions, keyed publications.

    python examples/actors/work_queue.py            # one GPU
    python examples/actors/work_queue.py --cpu      # the same calls on the CPU runtime

The process joins a one-member cluster with a ``gpu:`` section and hosts counter actors.
``--workers`` of them subscribe to topic 0 as ONE queue subscription (``Subscribe(queue=True)``:
competing consumers, a NATS queue group, a Kafka consumer group), a second pool subscribes to
the same topic under another name, and one auditor actor subscribes the ordinary way.  Every
publication -- ``CounterAdd(amount)`` keyed by a user id -- then reaches the auditor, exactly
one worker of the first pool and exactly one of the second, and every publication of one user
reaches the same worker: per-key ordering.  Every actor's counter is checked against the numpy
prediction (``ops.scatter.queue_pick``), then the same publications go round robin
(``by="index"``).
"""
import argparse
import os
import socket
import sys
import tempfile

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ptype_amd import cluster as C  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_COUNTER_ADD, STATUS_OK  # noqa: E402
from ptype_amd.ops.scatter import queue_pick  # noqa: E402


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--workers", type=int, default=1000, help="members of the first pool")
    p.add_argument("--publications", type=int, default=1 << 16)
    p.add_argument("--users", type=int, default=5000, help="distinct keys")
    p.add_argument("--cpu", action="store_true")
    a = p.parse_args()
    os.environ.setdefault("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    W, W2, Q = a.workers, max(a.workers // 3, 1), a.publications
    n = 1 + W + 2 * W2  # actor 0 audits, then the first pool, then the second on every other id
    with tempfile.TemporaryDirectory() as tmp:
        pp, pc = free_port(), free_port()
        cfg = C.Config()
        cfg.service_name, cfg.node_name, cfg.port = "counters", "node0", free_port()
        cfg.member = C.member_config(name="m0", dir=os.path.join(tmp, "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                     apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                     acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                     heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
        cfg.has_gpu = True
        cfg.gpu.cpu, cfg.gpu.actors, cfg.gpu.max_batch = a.cpu, n, 4 * Q
        cluster = C.Join(C.background(), cfg)
        server = C.Server()  # NewClient dials the registered node
        server.RegisterFunc("Counters.Ping", lambda args: 0)
        server.Listen(cfg.port, "127.0.0.1")
        client = cluster.NewClient("counters", C.ConnConfig())
        try:
            rt = cluster.runtime
            dev = rt.device
            client.Subscribe(0, actors=[0], name="audit")
            client.Subscribe(0, segments=[[1, W, 1]], name="pool", queue=True)
            client.Subscribe(0, segments=[[1 + W, W2, 2]], name="pool2", queue=True)
            print("topic 0:", [(name, segs, "queue" if q else "all") for name, segs, q in client.Topics(queues=True)[0]])
            gen = torch.Generator().manual_seed(1)
            user = torch.randint(0, a.users, (Q,), generator=gen)
            amount = torch.randint(1, 1000, (Q,), generator=gen)
            pubs = MsgBatch(torch.zeros(Q, dtype=torch.int32, device=dev), amount.to(dev), None, None, METHOD_COUNTER_ADD)
            ans = client.Publish(pubs, key=user.to(dev), op="sum")
            if dev.type == "cuda":
                torch.cuda.synchronize()
            # the prediction: the auditor gets everything, a pool's member m what its users published
            want = np.zeros(rt.total_actors, dtype=np.int64)
            want[0] = int(amount.sum())
            np.add.at(want, 1 + queue_pick(W, key=user.numpy()).astype(np.int64), amount.numpy())
            np.add.at(want, 1 + W + 2 * queue_pick(W2, key=user.numpy()).astype(np.int64), amount.numpy())
            ok = (torch.equal(rt.state[:rt.total_actors].cpu(), torch.from_numpy(want)) and ans.count.cpu().tolist() == [3] * Q
                  and bool((ans.status == STATUS_OK).all()))
            busy = int((want[1:1 + W] > 0).sum())
            print(f"{Q} publications of {a.users} users -> {ans.val.numel()} deliveries (3 each); {busy} of {W} workers of the "
                  f"first pool got work; every counter as predicted: {ok}")
            # round robin instead: publication q of the batch goes to member (seq + q) % c
            seq = rt.topics().scatter.seq
            client.Publish(pubs, by="index")
            if dev.type == "cuda":
                torch.cuda.synchronize()
            q = (np.arange(Q, dtype=np.uint64) + np.uint64(seq))
            want[0] += int(amount.sum())
            np.add.at(want, 1 + queue_pick(W, index=q).astype(np.int64), amount.numpy())
            np.add.at(want, 1 + W + 2 * queue_pick(W2, index=q).astype(np.int64), amount.numpy())
            ok = ok and torch.equal(rt.state[:rt.total_actors].cpu(), torch.from_numpy(want))
            print(f"round robin: every counter as predicted: {ok}")
            print("stats:", cluster.Stats()["runtime"]["queues"])
        finally:
            client.Close()
            server.Close()
            cluster.Close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
