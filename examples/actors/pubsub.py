#!/usr/bin/env python3
"""Publish/subscribe over GPU actors: topics kept in the replicated store, expanded on the device.

    python examples/actors/pubsub.py            # one GPU
    python examples/actors/pubsub.py --cpu      # the same calls on the CPU runtime

The process joins a one-member cluster with a ``gpu:`` section and hosts ``--actors``
counter actors.  It subscribes them to topics as strided segments -- topic ``r`` is "every
actor of shard r" (``r + shards * k``: one segment, whatever the number of actors), topic
``shards`` is "every actor" -- then publishes ``CounterAdd`` to the topics.  One publication
becomes one call per subscriber on the device (no per-subscriber table exists anywhere), the
replies are folded per publication, and the counters are checked against what the
subscriptions say.  A second subscription that names some actors again delivers to them
twice: nothing is de-duplicated across subscriptions.
"""
import argparse
import os
import socket
import sys
import tempfile

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

import torch  # noqa: E402

from ptype_amd import cluster as C  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_COUNTER_ADD, STATUS_OK  # noqa: E402


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--actors", type=int, default=65536)
    p.add_argument("--shards", type=int, default=4, help="topics 0 .. shards - 1: the actors a % shards == r")
    p.add_argument("--cpu", action="store_true")
    a = p.parse_args()
    os.environ.setdefault("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    with tempfile.TemporaryDirectory() as tmp:
        pp, pc = free_port(), free_port()
        cfg = C.Config()
        cfg.service_name, cfg.node_name, cfg.port = "counters", "node0", free_port()
        cfg.member = C.member_config(name="m0", dir=os.path.join(tmp, "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                     apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                     acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                     heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
        cfg.has_gpu = True
        cfg.gpu.cpu, cfg.gpu.actors, cfg.gpu.max_batch = a.cpu, a.actors, 4 * a.actors
        cluster = C.Join(C.background(), cfg)
        server = C.Server()  # NewClient dials the registered node
        server.RegisterFunc("Counters.Ping", lambda args: 0)
        server.Listen(cfg.port, "127.0.0.1")
        client = cluster.NewClient("counters", C.ConnConfig())
        try:
            rt = cluster.runtime
            n, W, dev = rt.total_actors, a.shards, rt.device
            for r in range(W):  # "every actor of shard r": one strided segment
                client.Subscribe(r, segments=[[r, len(range(r, n, W)), W]], name=f"shard{r}")
            client.Subscribe(W, segments=[[0, n, 1]], name="everyone")
            client.Subscribe(W, actors=range(0, min(n, 10)), name="the-first-ten-again")  # duplicates: delivered twice
            print("topics:", {g: [(name, segs) for name, segs in subs] for g, subs in client.Topics().items()})
            # publication q: CounterAdd(q + 1) to topic q; then +100 to everyone
            topics = torch.arange(W + 1, dtype=torch.int32, device=dev)
            add = torch.cat([torch.arange(1, W + 1), torch.tensor([100])]).to(dev)
            ans = client.Publish(MsgBatch(topics, add, None, None, METHOD_COUNTER_ADD), op="sum")
            if dev.type == "cuda":
                torch.cuda.synchronize()
            ids = torch.arange(n)
            want = ids % W + 1 + 100 + 100 * (ids < 10)
            counts = [len(range(r, n, W)) for r in range(W)] + [n + min(n, 10)]
            ok = (torch.equal(rt.state[:n].cpu(), want) and ans.count.cpu().tolist() == counts
                  and ans.n_ok.cpu().tolist() == counts and bool((ans.status == STATUS_OK).all()))
            print(f"{W + 1} publications -> {ans.val.numel()} deliveries; subscribers addressed {ans.count.cpu().tolist()}, "
                  f"answered OK {ans.n_ok.cpu().tolist()}; every counter as subscribed: {ok}")
            for r in range(W):
                client.Unsubscribe(r, name=f"shard{r}")
            again = client.Publish(MsgBatch(topics, add, None, None, METHOD_COUNTER_ADD))
            left = again.count.cpu().tolist()
            print("after Unsubscribe of the shard topics, subscribers addressed:", left)
            ok = ok and left == [0] * W + [n + min(n, 10)]
            print("stats:", cluster.Stats()["runtime"]["topics"])
        finally:
            client.Close()
            server.Close()
            cluster.Close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
