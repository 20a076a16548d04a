"""Per-process GPU actor runtime: the device side of a cluster member.

One process per GPU.  A ``DeviceRuntime`` owns, on its GPU:

* the actor mailboxes' state (``int64`` per actor, random-init optional),
* the persistent dispatcher (host-visible request/reply rings) for the
  single-call latency path -- ``Call`` on a GPU actor needs no kernel launch,
* the GPU registry mirror (``ops.RegistryTable``) mapping every actor id of a
  service to (rank, mailbox), kept in step with the authoritative control-plane
  store, and
* the exchange engine (``parallel.ActorExchange``) for batched ``Send`` across
  the GPUs of the node over RCCL.

Actor placement is published in the replicated KV store, one key per rank and
service (``store/_ptype/actors/<service>/<node>`` -> ``{"rank","world","count"}``,
strided ids: actor ``a`` lives on rank ``a % world`` in mailbox ``a // world``),
attached to a lease this process keeps alive, so the Raft log carries one
entry per shard, not one per actor, while the GPU table holds every actor (1M
actors = 2M slots = 32 MB of HBM).  ``mirror.RegistryMirror`` follows those
records (watch + lease expiry) into the table; with ``gpu.world > 1`` Join
forms the data-plane group through the store first (parallel/bootstrap.py).

Rank failures.  A runtime whose group Join formed is elastic.  On
a GPU the group is the compiled DataPlane (``NativeGroup``: RCCL, or IpcComm
between the processes of one GPU) and the whole lifecycle is its: the Send
watchdog (a C++ thread) fails a generation whose Send is overdue, ``recover``
is one call -- abort, lease-driven settle, generation g + 1 through the store,
ring adoption of the lost ranks' blocks -- and ``replicate`` moves buddy
replicas; this module only applies the DataPlane's plan to its tensors (the
state blocks, the registry table, the dispatcher).  A CPU runtime (gloo)
re-forms its torch group the same way (bootstrap.form_group, elastic.py
helpers).  Either way the dead rank's actors move to their ring successor
(state from the buddy replica, else zero), the shard record is republished and
the Send is re-sent:
``send_all`` re-sends the whole batch (at-least-once, like the reference
client's retries, cluster/rpc.go:107-116); ``send(..., resend_overflow=False)``
answers the messages whose actor lived on the lost rank with
``STATUS_RANK_LOST`` and delivers the rest.  The reference's client survives a
dead node the same way: lease lapse (cluster/registry.go:51-86), watch re-list
(:119-150), balancer re-selection (cluster/rpc.go:197-244).

Reference: the reference has no device side; this realises SURVEY C9/C10/C14
under the API of cluster/cluster.go and cluster/rpc.go.
"""
from __future__ import annotations

import json
import logging
import os
import time

import torch

from .ops import batch as B
from .ops import hip
from .ops.records import STATUS_OK, STATUS_RANK_LOST
from .ops.table import RegistryTable, actor_keys
from .utils import trace

ACTORS_PREFIX = "_ptype/actors"
_log = logging.getLogger("ptype.runtime")


def _dist():
    import torch.distributed as dist

    return dist if dist.is_available() and dist.is_initialized() else None


class DeviceRuntime:
    def __init__(self, device=None, actors: int = 1024, ring: int = 4096, idle_ms: float = 200.0,
                 delay_us: int = 0, max_batch: int = 1 << 20, chunks: int = 0, random_state: bool = False,
                 group=None, shm: bool = True, service: str = "", mailbox_shards: int = 256,
                 mailbox_slots: int = 0, delivery: str = "auto", comm: str = "rccl", comm_timeout_s: float = 30.0,
                 ledger: bool = False, coalesce: bool = False, cache: bool = False, cache_entries: int = 1 << 20,
                 breaker: bool = False, breaker_threshold: int = 5, breaker_cooldown: int = 8,
                 breaker_actors: int = 0, breaker_trip_on=None, limit: bool = False, limit_rate: int = 1,
                 limit_burst: int = 1, limit_actors: int = 0, dead_letters: bool = False,
                 dead_letter_entries: int = 1 << 16, dead_letter_mask=None, max_topics: int = 1024,
                 timers: bool = False, timer_entries: int = 1 << 20, timer_horizon: int = 256,
                 timer_runs: int = 256):
        if device is None:
            device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        self.device = torch.device(device)
        # a CPU runtime runs the handler table's host reference (tests, GPU-less hosts):
        # no persistent dispatcher, no HBM mailboxes, gloo collectives
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu:
            torch.cuda.set_device(self.device)
        d = _dist()
        self.group = group
        if group is not None and hasattr(group, "comm_ptr"):  # NativeGroup: the compiled DataPlane
            self.rank, self.world = group.rank, group.size
        else:
            self.rank = d.get_rank(group) if d else 0
            self.world = d.get_world_size(group) if d else 1
        self.service = service
        # services whose actors are this runtime's actors: the one it joined as, plus
        # any co-hosted through host()/serve() (one actor id space per runtime)
        self.hosted: set[str] = {service} if service else set()
        self.actors = int(actors)
        if random_state:
            g = torch.Generator(device=self.device).manual_seed(1234 + self.rank)
            self.state = torch.randint(0, 1 << 20, (self.actors,), dtype=torch.int64, device=self.device, generator=g)
        else:
            self.state = torch.zeros(self.actors, dtype=torch.int64, device=self.device)
        self.delay_us = int(delay_us)
        self.server = None
        if self.on_gpu:
            # dispatcher rings in shared memory: same-node client processes call these
            # GPU actors without a socket (shmring.hpp)
            self.server = hip().DeviceServer(self.device.index or 0, int(ring), self.state.data_ptr(), self.actors,
                                             self.delay_us, float(idle_ms), 60.0,
                                             f"ptype-{os.getpid()}-{self.device.index or 0}" if shm else "")
        self._ring, self._idle_ms = int(ring), float(idle_ms)
        self.table = RegistryTable(2 * self.actors * self.world, device=self.device)
        # dense actor ids [0, actors*world): route through the compiled directory (K5b)
        self.table.enable_directory(self.actors * self.world, affine_world=self.world)
        self.max_batch = int(max_batch)
        # 2 pipeline chunks at N > 1: the measured optimum at R = 2, 4 and 8 (profiles/r2_chunk_model)
        self.chunks = chunks or (1 if self.world == 1 else 2)
        # elasticity (set by for_cluster when Join formed the group)
        self.world0 = self.world    # the original world: actor a belongs to original rank a % world0
        self.blocks = [self.rank]   # original ranks whose actors this process hosts (mailbox-block order)
        self.membership = None      # {"me", "nodes0", "members", "gen"} of the group Join formed
        self._elastic_cfg = None
        self.replicas: dict[int, torch.Tensor] = {}  # original rank -> its block as of the last replicate()
        self.restored: list[int] = []
        self.recoveries = 0
        self.replicate_every = 0
        self._sends = 0
        self._cpu_failed = None  # a CPU runtime's failed generation (fail_generation)
        self.mailbox_shards, self.mailbox_slots = int(mailbox_shards), int(mailbox_slots)
        self.delivery = delivery or "auto"  # "mailbox": every Send through the HBM mailboxes (ActorExchange)
        # N > 1 collectives: the group's RCCL communicator, or IpcComm ("ipc": shared-memory
        # segments every rank maps, over a gloo group -- several ranks may share one GPU)
        self.comm, self.comm_timeout_s = comm or "rccl", float(comm_timeout_s)
        self._exchange = None
        # Send ledger (ops/ledger.py, opt-in): per-method counts, a digest of every reply and
        # per-actor load of the batches this rank sent, kept in HBM and read by stats()
        self.ledger = None
        if ledger:
            from .ops.ledger import Ledger

            self.ledger = Ledger(self.device, actors=self.total_actors)
        # Send coalescing (ops/coalesce.py): the default of send(coalesce=None), the grouping
        # workspace with its host counters (created by the first coalesced Send)
        self.coalesce = bool(coalesce)
        self._coalescer = None
        # Reply cache (ops/reply_cache.py): the default of send(cache=None), the table with its
        # host counters (created by the first cached Send), and the registry change counter --
        # bumped by everything that can change which actors answer; a cached Send that sees it
        # (or its router's record counter) moved clears the cache first
        self.cache, self.cache_entries = bool(cache), int(cache_entries)
        self._cache = None
        self._registry_changes = 0
        self._cache_seen = None
        # Circuit breaker (ops/breaker.py): the default of send(breaker=None), its settings, the
        # state table with its host counters (created by the first guarded Send; breaker_actors 0:
        # one word per actor of the service) and what the last guarded Send saw of the registry
        from .ops.breaker import BreakerRef

        self.breaker = bool(breaker)
        self.breaker_threshold, self.breaker_cooldown = int(breaker_threshold), int(breaker_cooldown)
        self.breaker_actors, self.breaker_trip_on = int(breaker_actors), breaker_trip_on
        if self.breaker_actors < 0:
            raise ValueError("breaker_actors must be >= 0 (0: every actor of the service)")
        BreakerRef("cpu", 1, self.breaker_threshold, self.breaker_cooldown, breaker_trip_on)  # (validates the settings)
        self._breaker = None
        self._breaker_seen = None
        # Rate limiter (ops/limit.py): the default of send(limit=None), its settings and the
        # bucket table with its host counters (created by the first limited Send; limit_actors 0:
        # one word per actor of the service)
        from .ops.limit import LimiterRef

        self.limit = bool(limit)
        self.limit_rate, self.limit_burst, self.limit_actors = int(limit_rate), int(limit_burst), int(limit_actors)
        if self.limit_actors < 0:
            raise ValueError("limit_actors must be >= 0 (0: every actor of the service)")
        LimiterRef("cpu", 1, self.limit_rate, self.limit_burst)  # (validates the settings)
        self._limiter = None
        # Dead-letter queue (ops/dead_letters.py, opt-in): the default of send(dead_letter=None);
        # the calls whose final status is in the mask, kept whole in an HBM ring until they are
        # looked at (dead_letters()) or re-sent (redrive())
        from .ops import dead_letters as DL

        self.dead_letter_entries = DL.check_entries(dead_letter_entries)
        self.dead_letter_mask = DL.dead_letter_mask(dead_letter_mask)
        self._dlq = None
        if dead_letters:
            self._dlq = DL.DeadLetters(self.device, self.dead_letter_entries, self.dead_letter_mask,
                                       max_rows=self.max_batch)
        # Timer queue (ops/timers.py, opt-in): delayed messages kept whole in an HBM ring until
        # their tick (schedule(), tick()); the clock counts ticks, there is no wall clock
        from .ops import timers as TM

        self.timer_entries, self.timer_horizon = TM.check_entries(timer_entries), TM.check_horizon(timer_horizon)
        self.timer_runs = TM.check_runs(timer_runs)
        self._timers = None
        if timers:
            self._timers = TM.TimerQueue(self.device, self.timer_entries, self.timer_horizon, self.timer_runs,
                                         max_rows=self.max_batch)
        # Scatter-gather (ask, ops/scatter.py): host counters, from what every expansion read
        self._scatter_counters = {"asks": 0, "questions": 0, "rows": 0, "oob": 0}
        # Pub/sub topics (publish, ops/topics.py): per service the follower-fed table and its scatter,
        # created by the first Subscribe or Publish (nothing is watched before); host counters
        self.max_topics = int(max_topics)
        if not 1 <= self.max_topics <= 1 << 20:
            raise ValueError("max_topics must be in [1, 2**20]")
        self._topics: dict = {}
        self._topic_counters = {"publishes": 0, "publications": 0, "rows": 0, "oob": 0}
        self._queue_rows = 0  # the queue-subscription rows published (Stats()["runtime"]["queues"])
        self.shards: dict[str, list[dict]] = {}
        self.mirror = None  # RegistryMirror (watch-driven) once attached to a control plane
        self.shard_lease = None
        self._tcp_store = None  # rendezvous store of a group this runtime formed (kept alive)
        self._owns_group = False
        self._closed = False

    # ------------------------------------------------------------------ setup
    @classmethod
    def for_cluster(cls, core_cluster, cfg) -> "DeviceRuntime":
        """The device side of ``Join``: form the service's data plane through the
        store when ``gpu.world > 1`` (parallel/bootstrap.py), start the runtime on
        this rank's device, publish the actor shard under a lease and mirror every
        shard of the service into the registry table (mirror.py)."""
        import torch.distributed as dist

        from .cluster import KVStore, Registry

        g = cfg.gpu
        owns = False
        tcp = None
        ndev = 0 if g.cpu else torch.cuda.device_count()

        def device_for_rank(r: int):
            if g.cpu:
                return torch.device("cpu")
            if g.device >= 0:
                return torch.device("cuda", g.device)
            lr = os.environ.get("LOCAL_RANK")
            return torch.device("cuda", int(lr) if lr is not None else r % max(ndev, 1))

        members = None
        native = None
        if (g.world > 1 or g.form_group) and not (dist.is_available() and dist.is_initialized()):
            from .parallel.bootstrap import form_group, node_id, wait_nodes

            me = node_id(core_cluster.local_addr, cfg.port)
            registry = Registry(core_cluster.registry)
            store = KVStore(core_cluster.store)
            if not g.cpu:
                # the group's whole lifecycle in the control plane (csrc/core/dataplane.hpp): store
                # rendezvous, RCCL init (or IpcComm segments: gpu.comm ipc), abort, next generation
                from .parallel.exchange import ipc_cap_for
                from .parallel.native_group import NativeGroup

                world = max(g.world, 1)
                chunks = 1 if world == 1 else 2
                native = NativeGroup.join(core_cluster, cfg.service_name, me, device_for_rank, world,
                                          timeout_s=max(30.0, g.group_timeout_s), transport=g.comm,
                                          cap_bytes=ipc_cap_for(g.max_batch, chunks, world) if g.comm == "ipc" else 0)
                members = native.members
                backend = "native"
            else:
                backend = g.backend or "gloo"
                nodes = wait_nodes(registry, cfg.service_name, max(g.world, 1))
                members, tcp = form_group(store, core_cluster.local_addr, me, cfg.service_name, 0, nodes, backend,
                                          device_for_rank, timeout_s=g.group_timeout_s)
            owns = True
        d = _dist()
        rank = native.rank if native is not None else (d.get_rank() if d else 0)
        rt = cls(device_for_rank(rank), actors=g.actors, ring=g.ring, idle_ms=g.idle_ms, delay_us=g.delay_us,
                 max_batch=g.max_batch, service=cfg.service_name, mailbox_shards=g.mailbox_shards,
                 mailbox_slots=g.mailbox_slots, delivery=g.delivery, comm=g.comm,
                 comm_timeout_s=g.group_timeout_s, group=native, ledger=g.ledger, coalesce=g.coalesce,
                 cache=g.cache, cache_entries=g.cache_entries, breaker=g.breaker,
                 breaker_threshold=g.breaker_threshold, breaker_cooldown=g.breaker_cooldown,
                 breaker_actors=g.breaker_actors, limit=g.limit, limit_rate=g.limit_rate,
                 limit_burst=g.limit_burst, limit_actors=g.limit_actors, dead_letters=g.dead_letters,
                 dead_letter_entries=g.dead_letter_entries, dead_letter_mask=g.dead_letter_mask or None,
                 max_topics=g.topics, timers=g.timers, timer_entries=g.timer_entries,
                 timer_horizon=g.timer_horizon, timer_runs=g.timer_runs)
        rt._tcp_store, rt._owns_group = tcp, owns
        rt._addr = (core_cluster.local_addr, int(cfg.port))
        if members is not None and g.elastic:
            rt.membership = {"me": me, "nodes0": list(members), "members": list(members), "gen": 0}
            rt._elastic_cfg = {"store": store, "registry": registry, "local_addr": core_cluster.local_addr,
                               "backend": backend, "timeout_s": g.group_timeout_s, "grace_s": g.grace_s,
                               "max_recoveries": 3}
            rt.replicate_every = int(g.replicate_every)
            if g.send_timeout_s > 0 and native is not None:  # the DataPlane's watchdog thread (C++)
                native.dp.set_watchdog(float(g.send_timeout_s))
        rt.attach(core_cluster.registry.kv, cfg.service_name, cfg.node_name, watch=g.watch)
        # Send needs every rank's routes: wait until all shards of the group are mirrored
        rt.mirror.wait_shards(rt.world)
        return rt

    def attach(self, kv, service: str, node: str, watch: bool = True) -> None:
        """Publish this rank's shard (lease-attached) and follow every shard of
        ``service`` into the registry table."""
        from .mirror import RegistryMirror, ShardLease

        self.service = service
        self.hosted.add(service)
        self.shard_lease = ShardLease(kv, service, node, self.rank, self.world, self.actors)
        self.table.clear()
        self.mirror = RegistryMirror(self.table, kv, service, watch=watch)
        self.mirror.apply()
        self._registry_changes += 1
        self._kv, self._node = kv, node

    def sync(self) -> int:
        """Apply pending registry changes (joins, leaves, lease expiries) now."""
        n = self.mirror.apply() if self.mirror is not None else 0
        if n:
            self._registry_changes += 1
        return n

    def publish_shard(self, store, service: str, node: str) -> None:
        """Record this rank's actor shard of `service` in the replicated store
        (without a lease; ``attach`` keeps a lease-attached record instead)."""
        from .cluster import Context

        v = json.dumps({"rank": self.rank, "world": self.world, "count": self.actors, "node": node})
        store.put(Context.background(), f"{ACTORS_PREFIX}/{service}/{node}", v)

    def sync_registry(self, store, service: str) -> int:
        """One-shot rebuild of the GPU registry mirror of `service` from the
        published shards (K5 batch upsert on the device); returns the number of actors."""
        from .cluster import Context, NoKeyError, WithPrefix

        try:
            vals = store.get(Context.background(), f"{ACTORS_PREFIX}/{service}/", WithPrefix())
        except NoKeyError:
            vals = []
        shards = [json.loads(v) for v in vals]
        self.shards[service] = shards
        self.table.clear()
        total = 0
        for s in shards:
            n, r, w = int(s["count"]), int(s["rank"]), int(s["world"])
            mbox = torch.arange(n, dtype=torch.int64, device=self.device)
            ids = r + w * mbox
            self.table.upsert(actor_keys(ids), torch.full((n,), r, dtype=torch.int32, device=self.device),
                              mbox.to(torch.int32))
            total += n
        self._registry_changes += 1
        return total

    def place_local(self, n_actors_total: int | None = None) -> None:
        """Strided placement without a control plane (single process / bench):
        every rank mirrors every rank's shard."""
        n = self.actors
        self._registry_changes += 1
        self.table.clear()
        for r in range(self.world):
            mbox = torch.arange(n, dtype=torch.int64, device=self.device)
            self.table.upsert(actor_keys(r + self.world * mbox),
                              torch.full((n,), r, dtype=torch.int32, device=self.device), mbox.to(torch.int32))

    @property
    def total_actors(self) -> int:
        return self.actors * self.world0

    @property
    def mailboxes(self) -> int:
        """Mailboxes this process hosts (``actors`` per hosted block)."""
        return self.state.numel()

    @property
    def exchange(self):
        if self._exchange is None:
            from .parallel.exchange import ActorExchange

            self._exchange = ActorExchange(self.table, self.max_batch, chunks=self.chunks, group=self.group,
                                           state=self.state, delay_us=self.delay_us, delivery=self.delivery,
                                           mailbox_shards=self.mailbox_shards, mailbox_slots=self.mailbox_slots,
                                           comm=self.comm if self.on_gpu else "rccl",
                                           comm_timeout_s=self.comm_timeout_s)
        return self._exchange

    # ------------------------------------------------------------------ data plane
    def host(self, service: str) -> None:
        """Co-host ``service`` on this runtime's actors (the reference registers
        several net/rpc services on one server; here they share the GPU actors and
        the registry mirror, and a Send names which one it addresses)."""
        self.hosted.add(service)
        self._registry_changes += 1

    def _check_service(self, service: str | None) -> None:
        if service and self.hosted and service not in self.hosted:
            raise ValueError(f"Send to {service!r}: this process's data plane hosts {sorted(self.hosted)} "
                             "(co-host more services with DeviceRuntime.host)")

    # ------------------------------------------------------------------ replicated services (parallel/replicas.py)
    def serve_replica(self, service: str, address: str | None = None, port: int | None = None) -> None:
        """Serve ``service`` as one replica of a replicated stateless service:
        its logical actors [0, actors) are this rank's mailboxes (lease-attached
        record ``_ptype/actors/<service>/<node>`` with ``"replica": true``)."""
        from .mirror import ShardLease

        if getattr(self, "_kv", None) is None:
            raise RuntimeError("serve_replica needs a control plane (Join, or attach())")
        addr, p = self._addr if getattr(self, "_addr", None) else ("", 0)
        self.host(service)
        lease = ShardLease(self._kv, service, self._node, self.blocks[0], self.world0, self.actors, replica=True,
                           address=address if address is not None else addr, port=int(port if port is not None else p))
        self._replica_leases = getattr(self, "_replica_leases", {})
        self._replica_leases[service] = lease

    def has_replicas(self, service: str) -> bool:
        """Whether ``service`` has replica records in the store."""
        from .mirror import ACTORS_PREFIX, STORE_PREFIX, _prefix_end

        kv = getattr(self, "_kv", None)
        if kv is None:
            return False
        from ._core import RangeOpts

        o = RangeOpts()
        pfx = f"{STORE_PREFIX}{ACTORS_PREFIX}/{service}/"
        o.end = _prefix_end(pfx)
        return any(json.loads(x.value).get("replica") for x in kv.get(pfx, o).kvs)

    def replica_router(self, service: str, max_connections: int = 3, local_addr: str | None = None):
        """A client's replica selection for ``service`` (follows its records)."""
        from .parallel.replicas import ReplicaRouter

        la = local_addr if local_addr is not None else (self._addr[0] if getattr(self, "_addr", None) else "")
        return ReplicaRouter(service, self.world0, la, max_connections, kv=self._kv)

    def send(self, service: str | None, batch: B.MsgBatch, resend_overflow: bool = True, router=None,
             retries: int | None = None, retry_on=None, account: bool | None = None,
             coalesce: bool | None = None, cache: bool | None = None, gather=None, breaker: bool | None = None,
             limit: bool | None = None, dead_letter: bool | None = None, dead_letter_tag: int = 0,
             dead_letter_attempts=None):
        """Batched Send (``_send``), optionally coalesced, answered from the reply cache,
        guarded by the circuit breaker and rate-limited per actor.
        ``dead_letter``: the rows whose final status is in the runtime's ``dead_letter_mask``
        (by default statuses 1 to 6) are filed, with the whole call, in the runtime's
        dead-letter queue in HBM (ops/dead_letters.py: protoactor's ``DeadLetterEvent``,
        Akka's ``deadLetters``), under the ids the caller wrote, with ``dead_letter_tag`` and
        ``dead_letter_attempts`` (an int32 column: earlier attempts of each row; None: none).
        None follows the runtime's setting (``DeviceRuntime(dead_letters=...)``,
        ``gpu.dead_letters``), False skips this Send, True without a queue raises.  It runs
        once per Send, on the full batch's final replies, where the ledger and the gather
        do: after coalescing's fan-out (a failed leader's followers each get a letter), the
        cache hits, the breaker's and the limiter's answers, the retries and the overflow
        re-sends.  Like an accounted Send it never defers its overflow re-sends.  It is the
        caller's view (no collective), reads nothing on the host and allocates nothing, so
        it does not by itself forbid graph capture; every replay files its letters again.
        ``dead_letters()`` looks at the queue, ``redrive()`` re-sends it.  Without it a Send
        creates, launches and reads nothing new.
        ``gather``: an ``ops.gather.Gather`` over this batch -- the replies are folded
        into its groups on the device (sum / min / max / first_ne per group, the first
        error per group), once per Send, on the full batch's final replies in the
        caller's order: after coalescing's fan-out, the cache hits, the retries and the
        overflow re-sends.  The return value stays ``(value, status)`` per message; the
        results are the object's output tensors, valid in stream order after the Send.
        Like an accounted Send, a gathered Send never defers its overflow re-sends;
        with ``resend_overflow=False`` the ``STATUS_OVERFLOW`` / ``STATUS_RANK_LOST`` rows are
        simply non-OK rows.  It is the caller's view (each rank gathers the batch it
        sent, no collective), reads nothing on the host and allocates nothing, so it
        does not by itself forbid graph capture.  Without it a Send creates, launches
        and reads nothing new.
        ``coalesce``: duplicate calls of a pure method (``records.PURE_METHODS``) in
        this batch -- equal ``(logical actor id, method, a0, a1, a2)`` -- are sent once
        and every duplicate gets the reply of the group's first message
        (ops/coalesce.py: Go's ``singleflight`` per Send).  None follows the runtime's
        setting (``DeviceRuntime(coalesce=...)``, ``gpu.coalesce``), False skips this
        Send.  The batch is grouped on the ids its caller wrote, before any ``router``;
        the leaders go through the whole Send below as one sub-batch in message order
        (one collective Send per rank whatever its K; retries, the router, the elastic
        loop and the overflow re-sends apply to the leaders, and a follower inherits its
        leader's final status, whatever it is); the Send ledger accounts the full batch
        once, on the fanned-out replies.  A batch without duplicates is sent as it is.
        A coalesced Send reads K on the host, so it is refused under graph capture, and
        it never defers its overflow re-sends.  The result equals, element for element,
        what the same Send returns without ``coalesce``.
        ``cache``: a call of a pure method whose ``STATUS_OK`` reply an earlier cached
        Send of this runtime stored -- same key as above -- is answered from the HBM
        reply cache and not sent (ops/reply_cache.py).  None follows the runtime's
        setting (``DeviceRuntime(cache=...)``, ``gpu.cache``), False skips this Send.
        The order is fixed: coalesce, then cache, then the Send below -- the cache sees
        coalescing's leaders, and retries, the router, the elastic loop and the overflow
        re-sends see the misses only, as one sub-batch in message order (a non-pure
        message is always a miss, so an ordered method keeps its per-actor FIFO).  The
        inner Send runs exactly once per cached Send (a rank whose batch was all hits
        joins with an empty batch); at world 1 with no miss it is skipped.  A non-OK
        reply is never stored.  The registry is synced first and the cache cleared when
        anything that decides whether an actor exists has changed since the last
        cached Send (``sync`` applying changes, ``recover``, ``restore_from``, ``host``,
        the router's record set); ``cache_clear()`` does it by hand.  A Send with another
        ``router`` than the last cached Send's (or with none after one, or the reverse)
        counts as such a change: clients with different routers that alternate on one
        runtime clear the cache on every Send and get nothing from it.  Like a coalesced
        Send it reads K on the host, is refused under graph capture and never defers;
        the ledger accounts the full batch once, hits included.  The table is state
        that outlives the Send and stream order is its only protection: every cached
        Send of a runtime must be issued on the same stream (or on streams the caller
        orders after one another).
        ``breaker``: a circuit breaker per logical actor id (ops/breaker.py: gobreaker, Akka's
        ``CircuitBreaker``).  An actor whose messages failed ``breaker_threshold`` times in a
        row -- a final status in ``breaker_trip_on``, by default ``STATUS_FAILED``,
        ``STATUS_NO_ACTOR`` or ``STATUS_NOT_DELIVERED``, with no ``STATUS_OK`` in between -- is
        open for the next ``breaker_cooldown`` guarded Sends: its messages are answered
        ``(0, STATUS_BREAKER_OPEN)`` and not sent.  After that the lowest message of a batch
        that addresses it travels as the probe (every other one is still rejected): OK closes
        the actor, a failure opens it for another cooldown.  None follows the runtime's
        setting (``DeviceRuntime(breaker=...)``, ``gpu.breaker``), False skips this Send.  The
        order is fixed: coalesce, cache, breaker, then the Send below -- a breaker wraps the
        retried call, so retries, the router, the elastic loop and the overflow re-sends see
        only the admitted rows, as one sub-batch in message order (an ordered method keeps
        its per-actor FIFO), and the final status after the retries is what the breaker
        observes.  A coalesced follower inherits its leader's ``STATUS_BREAKER_OPEN``; the
        cache never stores it (and a cached hit is never sent, so it passes an open breaker);
        the ledger counts it under "other"; a gather sees a non-OK row.  The inner Send runs
        exactly once per guarded Send at world > 1 (a rank whose batch was all rejected joins
        with an empty batch); at world 1 with nothing admitted it is skipped.  Time is
        counted in guarded Sends.  Every actor closes (``breaker_reset()`` does it by hand)
        when anything that decides whether an actor exists has changed since the last
        guarded Send, or when the same router's record set has; another router object alone
        does not reset.  A guarded Send reads the number of open actors on the host (and K
        when there are any), so it is refused under graph capture and never defers; with
        nothing open the batch is sent untouched and only the observation kernels follow.
        Like the cache's, its tables outlive the Send: all guarded Sends of a runtime go on
        one stream.
        ``limit``: a token bucket per logical actor id (ops/limit.py: ``golang.org/x/time/rate``,
        Akka's ``throttle``).  An actor gains ``limit_rate`` tokens per limited Send and holds at
        most ``limit_burst``; every message that travels costs one.  Of an actor whose rows
        exceed its tokens the first ones in message order travel, the others are answered
        ``(0, STATUS_THROTTLED)`` and not sent.  None follows the runtime's setting
        (``DeviceRuntime(limit=...)``, ``gpu.limit``), False skips this Send.  The order is
        fixed: coalesce, cache, breaker, limit, then the Send below -- the limiter is the
        innermost wrapper, so a token is spent only by a row that actually travels: followers,
        cache hits and breaker-rejected rows cost nothing, and a row that is retried or re-sent
        after an overflow costs one token for all its attempts.  The admitted rows go on as one
        sub-batch in message order (an ordered method keeps its per-actor FIFO).  A coalesced
        follower inherits its leader's ``STATUS_THROTTLED``; the cache never stores it; the
        breaker's ``trip_on`` cannot name it, so a throttled row counts as neither OK nor bad
        there and a throttled probe leaves its actor half-open; the ledger counts it under
        "other"; a gather sees a non-OK row.  The inner Send runs exactly once per limited Send
        at world > 1 (a rank whose batch was all throttled joins with an empty batch); at
        world 1 with nothing admitted it is skipped.  Time is counted in limited Sends.  The
        buckets do not depend on whether an actor exists: registry or router changes reset
        nothing, ``limit_reset()`` fills every bucket by hand.  A limited Send reads the number
        of actors over their quota on the host (and K when there are any), so it is refused
        under graph capture and never defers; with nothing over quota the batch is sent
        untouched after two launches.  Its tables outlive the Send: all limited Sends of a
        runtime go on one stream."""
        if coalesce is None:
            coalesce = self.coalesce
        if cache is None:
            cache = self.cache
        if breaker is None:
            breaker = self.breaker
        if limit is None:
            limit = self.limit
        if gather is not None:
            gather.check_batch(batch.M)
        dlq = self._dead_letter_sink(dead_letter, dead_letter_attempts, dead_letter_tag)
        if not coalesce and not cache and not breaker and not limit:
            return self._send(service, batch, resend_overflow, router, retries, retry_on, account, gather=gather,
                              dead_letters=dlq)
        if account and self.ledger is None:
            raise ValueError("send(account=True): this runtime keeps no Send ledger (DeviceRuntime(ledger=True), "
                             "gpu.ledger)")
        if (self._exchange is not None and self._exchange._capturing) or (
                self.on_gpu and torch.cuda.is_current_stream_capturing()):
            for on, name, why in ((coalesce, "coalesce", "selecting the leaders needs a host read"),
                                  (cache, "cache", "selecting the misses needs a host read"),
                                  (breaker, "breaker", "the count of open actors is read on the host"),
                                  (limit, "limit", "the count of actors over their quota is read on the host")):
                if on:
                    raise ValueError(f"send({name}=True) inside a captured Send: {why}")
        ledger = self.ledger if account is None or account else None
        # the inner Send accounts nothing: the full batch is accounted below, on the replies it returns
        inner = (lambda sub: self._send(service, sub, resend_overflow, router, retries, retry_on, False, final=True))

        def wrap(w, inner):
            return lambda sub: w.send(sub, inner, collective=self.world > 1)

        if limit:
            if self._limiter is None:
                from .ops.limit import Limiter

                self._limiter = Limiter(self.device, self.limit_actors or self.total_actors, self.limit_rate,
                                        self.limit_burst)
            if router is None:
                self._check_service(service)  # (an all-throttled Send never reaches _send's check)
            inner = wrap(self._limiter, inner)
        if breaker:
            if self._breaker is None:
                from .ops.breaker import Breaker

                self._breaker = Breaker(self.device, self.breaker_actors or self.total_actors, self.breaker_threshold,
                                        self.breaker_cooldown, self.breaker_trip_on)
            seen, last = self._existence_stamp(service, router), self._breaker_seen
            if last is not None and (seen[0] != last[0] or (seen[1] is last[1] and seen[2] != last[2])):
                self._breaker.reset()
            self._breaker_seen = seen
            inner = wrap(self._breaker, inner)
        if cache:
            if self._cache is None:
                from .ops.reply_cache import ReplyCache

                self._cache = ReplyCache(self.device, self.cache_entries)
            seen, last = self._existence_stamp(service, router), self._cache_seen
            if last is None or seen[0] != last[0] or seen[1] is not last[1] or seen[2] != last[2]:
                if last is not None:
                    self._cache.clear()
                self._cache_seen = seen
            inner = wrap(self._cache, inner)
        if not coalesce:
            return self._settle(batch, inner(batch), ledger, gather, dead_letters=dlq)
        if self._coalescer is None:
            from .ops.coalesce import Coalescer

            self._coalescer = Coalescer(self.device, self.max_batch)
        return self._settle(batch, self._coalescer.send(batch, inner)[0], ledger, gather, dead_letters=dlq)

    def _dead_letter_sink(self, dead_letter: bool | None, attempts=None, tag: int = 0):
        """The dead-letter queue with one Send's ``attempts`` and ``tag`` bound, or None."""
        if dead_letter is None:
            dead_letter = self._dlq is not None
        if not dead_letter:
            return None
        if self._dlq is None:
            raise ValueError("send(dead_letter=True): this runtime keeps no dead-letter queue "
                             "(DeviceRuntime(dead_letters=True), gpu.dead_letters)")
        return self._dlq.bound(attempts, tag)

    def _existence_stamp(self, service: str | None, router):
        """What decides whether an actor exists, brought up to date: the registry change
        counter, the router (itself, not its id(): a collected router's id can be reused)
        and its record counter.  A Send whose wrappers answer every row never reaches
        ``_send``'s service check, so it is made here."""
        self.sync()
        if router is not None:
            router.refresh()
        else:
            self._check_service(service)
        return self._registry_changes, router, None if router is None else router.changes

    def _settle(self, batch: B.MsgBatch, out, ledger, gather, logical=None, dead_letters=None):
        """A Send's final replies into the ledger (``batch`` under its ``logical`` actor
        ids, when a router rewrote them), the gather and the dead-letter queue (under the
        logical ids too); returns ``out``."""
        if ledger is not None:
            ledger.account(batch if logical is None else self._logical_batch(batch, logical), out[0], out[1])
        if gather is not None:
            gather.reduce(out[0], out[1])
        if dead_letters is not None:
            dead_letters.append(batch if logical is None else self._logical_batch(batch, logical), out[1])
        return out

    def dead_letters(self, max_letters: int | None = None, drain: bool = False):
        """The unread letters of the dead-letter queue (at most ``max_letters``), oldest
        first, as an ``ops.dead_letters.Letters``: SoA columns on the device (``seq``, ``row``,
        ``status``, ``actor``, ``method``, ``attempts``, ``a0``, ``a1``, ``a2``, ``tag``) with ``n``
        and ``torn``.  ``drain``: they leave the queue.  Reads the queue's head and tail on
        the host."""
        if self._dlq is None:
            raise ValueError("dead_letters(): this runtime keeps no dead-letter queue "
                             "(DeviceRuntime(dead_letters=True), gpu.dead_letters)")
        return self._dlq.take(max_letters, drain)

    def redrive(self, service: str | None, max_letters: int | None = None, router=None, **send_kw):
        """Re-send the dead letters: up to ``min(unread, max_letters, max_batch)`` of them are
        taken out of the queue, oldest first, and sent as one batch of the logical ids their
        callers wrote -- through ``send`` with every keyword it takes (``send_kw``), and with
        dead-lettering on, the letters' ``attempts`` and the caller's ``dead_letter_tag``: a
        letter that fails again is back in the queue with ``attempts + 1``, one that succeeds
        has left it.  Returns an ``ops.dead_letters.Redrive``: the taken ``letters`` and the
        re-send's ``(value, status)``, row for row.  It reads the queue on the host, so it is
        refused under graph capture.  At world > 1 it is a collective Send like any other (a
        rank without letters joins with an empty batch); at world 1 without letters the Send
        is skipped.  The keywords are checked before a letter is taken -- an unknown one,
        ``account=True`` without a ledger, a ``gather`` of another size than the letters to
        take, ``retries`` with ``resend_overflow=False`` or a bad ``retry_on``, a service this
        runtime does not host -- so such a call leaves the queue as it was.  An error the
        Send raises later than that (letters of an ordered method re-sent with ``retries``,
        a rank failure that is not recovered) finds the letters already taken: they are not
        put back."""
        from .ops.dead_letters import Redrive

        if self._dlq is None:
            raise ValueError("redrive(): this runtime keeps no dead-letter queue "
                             "(DeviceRuntime(dead_letters=True), gpu.dead_letters)")
        if "dead_letter" in send_kw or "dead_letter_attempts" in send_kw:
            raise ValueError("redrive: dead-lettering of the re-send is its own (attempts, dead_letter=True)")
        if (self._exchange is not None and self._exchange._capturing) or (
                self.on_gpu and torch.cuda.is_current_stream_capturing()):
            raise ValueError("redrive inside a captured Send: the queue's head and tail are read on the host")
        # what send would refuse, before a letter leaves the queue
        self._check_send_keywords("redrive", service, router, send_kw)
        ex = self.exchange
        n = min(self._dlq.read()["unread"], ex.max_chunk * ex.chunks)
        if max_letters is not None:
            n = min(n, max(0, int(max_letters)))
        if send_kw.get("gather") is not None:
            send_kw["gather"].check_batch(n)
        letters = self._dlq.take(n, drain=True)
        self._dlq.counters["redrives"] += 1
        self._dlq.counters["redriven"] += letters.n
        if letters.n or self.world > 1:
            out = self.send(service, letters.batch(), router=router, dead_letter=True,
                            dead_letter_attempts=letters.attempts, **send_kw)
        else:
            out = (torch.empty(0, dtype=torch.int64, device=self.device),
                   torch.empty(0, dtype=torch.int32, device=self.device))
        return Redrive(letters, out[0], out[1])

    def _check_send_keywords(self, who: str, service: str | None, router, send_kw: dict) -> None:
        """What ``send`` would refuse whatever the batch, raised before ``who`` (redrive, tick)
        takes anything out of its queue: an unknown keyword (TypeError), ``account=True``
        without a ledger, ``retries`` with ``resend_overflow=False`` or a bad ``retry_on``, a
        service this runtime does not host."""
        import inspect

        from .ops.retry import retry_mask

        inspect.signature(self.send).bind(service, None, router=router, **send_kw)  # (an unknown keyword: TypeError)
        if send_kw.get("account") and self.ledger is None:
            raise ValueError(f"{who}(account=True): this runtime keeps no Send ledger (DeviceRuntime(ledger=True), "
                             "gpu.ledger)")
        if send_kw.get("retries"):
            if int(send_kw["retries"]) < 0:
                raise ValueError("retries >= 0")
            if not send_kw.get("resend_overflow", True):
                raise ValueError(f"{who}(retries > 0) runs after the overflow re-sends: resend_overflow=False "
                                 "excludes it")
            if send_kw.get("retry_on") is not None:
                retry_mask(send_kw["retry_on"])
        if router is None:
            self._check_service(service)

    def _timer_queue(self, who: str):
        if self._timers is None:
            raise ValueError(f"{who}: this runtime keeps no timer queue (DeviceRuntime(timers=True), gpu.timers)")
        if (self._exchange is not None and self._exchange._capturing) or (
                self.on_gpu and torch.cuda.is_current_stream_capturing()):
            raise ValueError(f"{who} inside a captured Send: the timer queue's counts are read on the host")
        return self._timers

    def schedule(self, batch: B.MsgBatch, delay, tag: int = 0):
        """Delayed messages (Akka's ``scheduleOnce``, protoactor's ``SendOnce``, SQS
        ``DelaySeconds``): row ``i`` of ``batch`` is filed in the runtime's timer queue in HBM
        (ops/timers.py), with its whole call under the id its caller wrote and ``tag``, to be
        sent by the ``tick()`` ``delay[i]`` ticks from now.  ``delay``: an int, or an int32[M]
        column on the batch's device; a row whose delay is outside ``[1, timer_horizon]`` is
        not filed and counted in ``refused``.  Nothing is routed now: the replica round robin
        and a re-homed actor are resolved when the message is due.  Returns an
        ``ops.timers.Scheduled`` (``n``, ``refused``, ``first_ticket``, ``now``); raises
        ``ops.timers.TimerQueueFull``, with nothing filed, when the ring or the run table lacks
        room.  It reads its counts on the host, so it is refused under graph capture; it is
        the caller's view (no collective)."""
        return self._timer_queue("schedule").schedule(batch, delay, tag)

    def tick(self, service: str | None, router=None, ticks: int | None = None, **send_kw):
        """Advance the runtime's clock by one tick and send what is due: the due records of
        every pending Schedule, in ticket order (per Schedule by ``(delay, row)``, Schedules in
        call order -- two messages for one actor due at the same tick are in that order in the
        batch, so with ``delivery="mailbox"`` an ordered method keeps its per-actor FIFO; the due
        batch carries a method column, and on the direct path an ordered method's updates are
        serialised per actor but not in batch order), go through ``send`` as one batch of the
        logical ids their callers wrote, with every keyword it takes (``send_kw``).  Returns an
        ``ops.timers.Ticked``: the ``due`` records (``ops.timers.Timers``) and the Send's ``(value,
        status)``, row for row.  More due rows than one Send holds are sent as consecutive
        slices in ticket order and the replies concatenated (a ``gather`` spans the whole tick
        and refuses that).  At world > 1 a tick is a collective Send like any other: a rank
        with nothing due joins with an empty batch, and every rank must send the same number
        of slices; at world 1 with nothing due the Send is skipped.  ``ticks=n`` is a host loop
        of ``n`` single ticks and returns their list.  The keywords are checked before the
        clock moves -- an unknown one, ``account=True`` without a ledger, ``dead_letter=True``
        without a queue, a ``gather`` of another size than what is due, ``retries`` with
        ``resend_overflow=False`` or a bad ``retry_on``, a service this runtime does not host
        -- so such a call leaves the clock and the queue as they were.  An error the Send
        raises later than that finds the records taken: they are not put back.  It reads
        ``n_due`` on the host, so it is refused under graph capture."""
        from .ops.timers import Ticked

        tq = self._timer_queue("tick")
        if "dead_letter_attempts" in send_kw:
            raise ValueError("tick: the rows that will be due are not the caller's to count attempts for")
        self._check_send_keywords("tick", service, router, send_kw)
        self._dead_letter_sink(send_kw.get("dead_letter"))  # (dead_letter=True without a queue: ValueError)
        if ticks is not None:
            if int(ticks) < 0 or send_kw.get("gather") is not None:
                raise ValueError("tick(ticks=n): n >= 0, and a gather belongs to one tick")
            return [self.tick(service, router=router, **send_kw) for _ in range(int(ticks))]
        ex = self.exchange
        cap = ex.max_chunk * ex.chunks
        if send_kw.get("gather") is not None:
            n = tq.peek()
            send_kw["gather"].check_batch(n)
            if n > cap:
                raise ValueError(f"tick(gather=): {n} rows are due, more than one Send holds ({cap})")
        due = tq.tick()
        outs = [self.send(service, self._timer_slice(due, lo, min(lo + cap, due.n)), router=router, **send_kw)
                for lo in range(0, due.n, cap)]
        if not outs and self.world > 1:
            outs = [self.send(service, due.batch(), router=router, **send_kw)]
        if len(outs) == 1:
            return Ticked(due, outs[0][0], outs[0][1])
        if not outs:
            return Ticked(due, torch.empty(0, dtype=torch.int64, device=self.device),
                          torch.empty(0, dtype=torch.int32, device=self.device))
        return Ticked(due, torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))

    @staticmethod
    def _timer_slice(due, lo: int, hi: int) -> B.MsgBatch:
        if lo == 0 and hi == due.n:
            return due.batch()
        # (copies: a Send's kernels load their columns from allocation-aligned tensors)
        return B.MsgBatch(*(c[lo:hi].clone() for c in (due.actor, due.a0, due.a1, due.a2, due.method)))

    def timers(self) -> dict:
        """The timer queue's counters (one host read of its control line): ``now``, ``head``,
        ``tail``, ``live`` (records filed and not yet due), ``runs`` (pending Schedules),
        ``refused``, ``delivered``, ``full`` (Schedules refused with ``TimerQueueFull``), ``torn`` and
        the sizes ``entries``, ``horizon``, ``max_runs``."""
        if self._timers is None:
            raise ValueError("timers(): this runtime keeps no timer queue (DeviceRuntime(timers=True), gpu.timers)")
        return self._timers.read()

    def ask(self, service: str | None, questions: B.MsgBatch, scatter, op: str = "sum", sentinel=None, key=None,
            **send_kw):
        """Scatter-gather in one call (the optimus coordinator's ``splitWork`` ..
        ``watchReplies``, coordinator.go:67-98): ``scatter`` (an ``ops.scatter.Scatter``)
        expands the Q ``questions`` into T calls on the device, the calls go through
        ``send`` -- ``send_kw`` is its keywords, so ``retries``, ``coalesce``, ``cache``,
        ``breaker``, ``limit``, ``dead_letter``, ``account``, ``router`` and ``resend_overflow`` apply
        to the expanded calls exactly as to any batch -- and the expansion's ``Gather`` folds the
        replies with ``op`` (``sentinel`` for ``first_ne``) into one answer per question.
        Returns an ``ops.scatter.Answer``.  The expansion reads its total on the host, so
        an Ask is refused under graph capture; more calls than a Send takes raise the
        Send's error before anything travels.  Each rank expands its own questions, there
        is no new collective: a rank whose expansion is empty joins the Send with an
        empty batch, and at world 1 an empty expansion skips the Send.  ``key``: the key column
        of a topics rule's queue subscriptions (``publish``); any other rule refuses one."""
        from .ops.scatter import Answer

        if "gather" in send_kw:
            raise ValueError("ask: the gather is the expansion's own (op=, sentinel=)")
        if self._exchange is not None and self._exchange._capturing:
            raise ValueError("ask inside a captured Send: the total of the expansion is read on the host")
        exp = scatter.expand(questions) if key is None else scatter.expand(questions, key=key)
        c = self._scatter_counters
        c["asks"] += 1
        c["questions"] += exp.Q
        c["rows"] += exp.total
        c["oob"] += exp.oob
        ex = self.exchange
        if exp.total > ex.max_chunk * ex.chunks:
            raise ValueError(f"batch of {exp.total} exceeds max_batch {ex.max_chunk * ex.chunks}")
        g = exp.gather(op, sentinel) if exp.Q else None
        if exp.total or self.world > 1:
            out = self.send(service, exp.batch, gather=g, **send_kw)
        else:
            out = (torch.empty(0, dtype=torch.int64, device=self.device),
                   torch.empty(0, dtype=torch.int32, device=self.device))
            if g is not None:
                g.reduce(out[0], out[1])
        if g is None:
            e64, e32 = exp.first, exp.n  # (no questions: empty int64 and int32 tensors)
            return Answer(e64, e32, e32, e32, e32, exp.first, exp.n, exp.oob, out[0], out[1])
        return Answer(g.value, g.status, g.n_ok, g.count, g.bad_row, exp.first, exp.n, exp.oob, out[0], out[1])

    def topics(self, service: str | None = None, table=None):
        """The ``ops.topics.TopicTable`` of ``service`` (default: the runtime's), created with its
        follower on first use; its scatter is ``topics(service).scatter``.  ``table``: install
        this table instead (one that follows no store: a runtime without a control plane)."""
        from .ops.scatter import Scatter
        from .ops.topics import TopicTable

        service = self.service if service is None else service
        t = self._topics.get(service)
        if table is not None:
            if t is not None:
                t.close()
            t = None
        if t is None:
            kv = getattr(self, "_kv", None)
            if table is None and kv is None:
                raise RuntimeError("topics need the cluster's control plane: this runtime is not attached to a store "
                                   "(Join with a gpu: section, or DeviceRuntime.attach)")
            ex = self.exchange
            t = table if table is not None else TopicTable(self.device, self.max_topics, kv=kv, service=service)
            t.scatter = Scatter.topics(t, capacity=ex.max_chunk * ex.chunks)
            self._topics[service] = t
        return t

    def publish(self, service: str | None, publications: B.MsgBatch, op: str = "sum", sentinel=None, key=None,
                by: str | None = None, **send_kw):
        """Publish/subscribe in one call (Akka's ``DistributedPubSub`` ``Publish``): publication
        q -- its ``actor`` column names a topic -- becomes one call to every subscriber of the
        topic, expanded on the device from the store's subscriptions (``ops/topics.py``), sent,
        and folded per publication.  ``topics(service).apply()`` followed by ``ask`` with the
        table's scatter: everything ``ask`` documents holds unchanged (the Send keywords, the
        refusal under capture, each rank expanding its own publications, no new collective).
        A subscription is visible to a Publish once ``TopicTable.wait`` of its revision returned
        (``Client.Subscribe`` waits for its own).

        Queue subscriptions (``Client.Subscribe(queue=True)``): after the calls to its topic's
        ordinary subscribers a publication makes ONE call per queue subscription of the topic,
        to the member picked ``by="key"`` (default: the hash of ``key[q]``, an int64[Q] column
        that defaults to the publication's ``a0`` -- one key always reaches one member while the
        membership stands) or ``by="index"`` (round robin over the table scatter's ``seq``
        counter); ``ops/scatter.py`` has the arithmetic.  Over a table without a queue
        subscription ``key`` and ``by`` change nothing."""
        if by not in (None, "key", "index"):
            raise ValueError('publish: by must be "key" or "index"')
        t = self._topics.get(self.service if service is None else service) or self.topics(service)
        if self._exchange is not None and self._exchange._capturing:
            raise ValueError("publish inside a captured Send: the total of the expansion is read on the host")
        t.apply()
        t.scatter.by = by or "key"
        if t.n_queues and publications.actor.numel():
            # the queue rows of these publications, from the host's table: 4 bytes per publication read
            g = publications.actor.detach().cpu().numpy().astype("int64")
            q_off = t.host["q_off"]
            g = g[(g >= 0) & (g < q_off.size - 1)]
            queue_rows = int((q_off[g + 1] - q_off[g]).sum())
        else:
            queue_rows = 0
        a = self._scatter_counters
        questions, rows, oob = a["questions"], a["rows"], a["oob"]
        out = self.ask(service, publications, t.scatter, op=op, sentinel=sentinel, key=key, **send_kw)
        self._queue_rows += queue_rows
        c = self._topic_counters
        c["publishes"] += 1
        c["publications"] += a["questions"] - questions
        c["rows"] += a["rows"] - rows
        c["oob"] += a["oob"] - oob
        return out

    def cache_clear(self) -> None:
        """Drop every entry of the reply cache (O(1): the cache's epoch moves on)."""
        if self._cache is not None:
            self._cache.clear()

    def breaker_reset(self) -> None:
        """Close every actor's circuit breaker (the breaker's tick goes on)."""
        if self._breaker is not None:
            self._breaker.reset()

    def limit_reset(self) -> None:
        """Fill every actor's token bucket (the limiter's tick goes on)."""
        if self._limiter is not None:
            self._limiter.reset()

    def _send(self, service: str | None, batch: B.MsgBatch, resend_overflow: bool = True, router=None,
              retries: int | None = None, retry_on=None, account: bool | None = None, final: bool = False,
              gather=None, dead_letters=None):
        """Batched Send: every message to its actor anywhere in the node and the
        replies back in message order.  Collective across the process group.
        Registry changes seen since the last Send are applied first.  With an
        elastic group a rank failure is recovered here (module docstring).
        ``router``: a replicated service's ReplicaRouter -- the batch's logical
        actor ids are routed to the selected replicas, round robin.
        ``retries``: up to that many further attempts of every message whose status
        is in ``retry_on`` (default STATUS_FAILED), each through ``router`` again --
        the reference's ``withRetry`` (``ActorExchange.send_all``).  None or 0: one
        attempt, no retry work at all.
        ``account``: whether the Send ledger (``DeviceRuntime(ledger=True)``,
        ``gpu.ledger``) accounts this Send -- once, on its final replies, under the
        batch's logical actor ids.  None follows the runtime's setting, False skips
        this Send, True without a ledger raises.  An accounted Send does not defer
        its overflow re-sends.
        ``final``: the replies must be final on return (a coalesced Send fans them
        out): the overflow re-sends are not deferred.
        ``gather``: an ``ops.gather.Gather`` that folds the final replies into its groups
        (``send``); a gathered Send does not defer its overflow re-sends either.
        ``dead_letters``: the dead-letter queue's sink of this Send (``send(dead_letter=)``): the
        final replies' failed rows are filed there, at the same point, never deferred."""
        if account and self.ledger is None:
            raise ValueError("send(account=True): this runtime keeps no Send ledger (DeviceRuntime(ledger=True), "
                             "gpu.ledger)")
        ledger = self.ledger if account is None or account else None
        rkw = {}
        if retries:
            if not resend_overflow:
                raise ValueError("send(retries > 0) runs after the overflow re-sends: resend_overflow=False excludes it")
            rkw = {"retries": int(retries), "reroute": None if router is None else router.route}
            if retry_on is not None:
                rkw["retry_on"] = retry_on
        logical = batch.actor
        if router is not None:
            batch = B.MsgBatch(router.route(batch.actor), batch.a0, batch.a1, batch.a2, batch.method)
        else:
            self._check_service(service)
        self.sync()
        if self.membership is None:
            ex = self.exchange
            if ledger is not None or gather is not None or dead_letters is not None:
                # on its final replies: never deferred
                if resend_overflow:
                    return ex.send_all(batch, logical=logical, ledger=ledger, gather=gather,
                                       dead_letters=dead_letters, **rkw)
                return self._settle(batch, ex.send(batch), ledger, gather, logical, dead_letters)
            # more than one rank: no host wait on this Send (its overflow, if any, is
            # re-sent just before Send + 2 or at flush(): ActorExchange.send_all)
            if rkw:
                return ex.send_all(batch, logical=logical, **rkw)
            return ex.send_all(batch, defer=self.world > 1 and not final) if resend_overflow else ex.send(batch)
        from .parallel.elastic import RankFailure, is_rank_failure

        dp = self.group.dp if self._native else None  # the compiled lifecycle (watchdog, recovery)
        lost_before: list[int] = []
        todo = None  # after a recovery without re-sends: the indices still to deliver
        for attempt in range(self._elastic_cfg["max_recoveries"] + 1):
            try:
                if self._failed():
                    raise RankFailure(self._failed())
                sub = batch if todo is None else batch.index_select(todo)
                if dp is not None:
                    dp.begin_send()  # the host part of the Send is bounded too
                try:
                    if rkw:  # the retry rounds are part of the Send: a rank failure in one is recovered alike
                        out = self.exchange.send_all(
                            sub, logical=logical if todo is None else logical.index_select(0, todo), **rkw)
                    else:
                        out = self.exchange.send_all(sub) if resend_overflow else self.exchange.send(sub)
                finally:
                    if dp is not None:
                        dp.end_send()
                if dp is not None and dp.watchdog_failed:  # aborted mid-Send: its replies are void
                    raise RankFailure(dp.watchdog_failed)
                ipc = self.exchange.ipc
                if ipc is not None:  # IpcComm: a peer that missed a collective is seen once the Send's waits end
                    torch.cuda.current_stream(self.device).synchronize()
                    ipc.check()
            except RuntimeError as e:
                # only a peer's failure re-forms the group; a local error (OOM, a launch
                # failure, a stalled look-back) propagates unchanged -- recovering from it
                # would abort every rank and re-run delivered, non-commutative messages
                if not is_rank_failure(e) or attempt == self._elastic_cfg["max_recoveries"]:
                    raise
                _log.warning("data-plane generation %d failed: %s", self.membership["gen"], str(e)[:300])
                trace.mark("ptype.rank_failure")
                lost_before += self.recover()
                if not resend_overflow and lost_before:
                    # messages whose actor lived on a lost rank: STATUS_RANK_LOST, not re-run
                    a = batch.actor.to(torch.int64)
                    lost = torch.zeros(a.numel(), dtype=torch.bool, device=a.device)
                    for r in lost_before:
                        lost |= (a % self.world0) == r
                    todo = torch.nonzero(~lost).flatten()
                continue
            self._sends += 1
            if dp is not None and self.on_gpu:  # the Send's device work must finish in time
                dp.arm(torch.cuda.current_stream(self.device).cuda_stream)
            if self.replicate_every and self._sends % self.replicate_every == 0:
                try:
                    self.replicate()
                except RuntimeError as e:
                    if not is_rank_failure(e):
                        raise
                    self.recover()  # the batch WAS delivered: recover, never re-send it
            if todo is None:
                return self._settle(batch, out, ledger, gather, logical, dead_letters)
            val = torch.zeros(batch.M, dtype=out[0].dtype, device=out[0].device)
            st = torch.full((batch.M,), STATUS_RANK_LOST, dtype=out[1].dtype, device=out[1].device)
            val[todo] = out[0]
            st[todo] = out[1]
            # the whole batch, the STATUS_RANK_LOST rows included
            return self._settle(batch, (val, st) + tuple(out[2:]), ledger, gather, logical, dead_letters)
        raise AssertionError("unreachable")

    @staticmethod
    def _logical_batch(batch: B.MsgBatch, logical: torch.Tensor) -> B.MsgBatch:
        """``batch`` as its caller addressed it (a replica router rewrote the actor
        column): what the Send ledger accounts."""
        if logical is batch.actor:
            return batch
        return B.MsgBatch(logical.to(torch.int32), batch.a0, batch.a1, batch.a2, batch.method)

    def _failed(self) -> str:
        """Why the current generation was failed ("" while fine)."""
        return self.group.dp.watchdog_failed if self._native else (self._cpu_failed or "")

    def fail_generation(self, why: str) -> None:
        """Mark the current generation failed, as the Send watchdog does: the next
        Send recovers (fault injection of the tests)."""
        if self._native:
            self.group.dp.fail_generation(why)
        else:
            self._cpu_failed = why

    def flush(self) -> None:
        """Every earlier Send's replies final (deferred re-sends run now).  Collective."""
        if getattr(self, "_exchange", None) is not None:
            self._exchange.flush()

    # ------------------------------------------------------------------ rank failures
    def replicate(self) -> None:
        """Collective over the current generation: every rank ships the blocks it
        hosts to its buddy (the node that would adopt them) and keeps the blocks it
        is buddy of, resident in HBM.  Point-to-point only.  On a GPU the DataPlane
        picks the buddies and moves the bytes (csrc/core/dataplane.cpp replicate)."""
        import torch.distributed as dist

        from .parallel.elastic import buddy, ring_placement

        m = self.membership
        if m is None:
            return
        P = self.actors
        if self._native:
            dp = self.group.dp
            src_blocks = list(dp.replica_blocks())
            recv = torch.empty(max(1, P * len(src_blocks)), dtype=torch.int64, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()  # the state's producers are done
            st = self.state.contiguous()
            got = list(dp.replicate(st.data_ptr(), st.numel() * 8, recv.data_ptr(), P * len(src_blocks) * 8))
            self.replicas = {r: recv[j * P:(j + 1) * P] for j, r in enumerate(got)}
            return
        own = ring_placement(m["nodes0"], m["members"])
        dst = buddy(m["nodes0"], m["members"], m["me"])
        if dst == m["me"]:
            return
        src = next(n for n in m["members"] if buddy(m["nodes0"], m["members"], n) == m["me"])
        # a gloo group (CPU runtimes) moves host tensors
        recv = torch.empty(P * len(own[src]), dtype=torch.int64, device=self.device)
        ops = [dist.P2POp(dist.isend, self.state, m["members"].index(dst)),
               dist.P2POp(dist.irecv, recv, m["members"].index(src))]
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        self.replicas = {r: recv[j * P:(j + 1) * P] for j, r in enumerate(own[src])}

    def recover(self) -> list[int]:
        """Abort the failed generation, let the lease-based membership settle,
        form the next generation through the store and re-home the lost ranks'
        actors.  Returns the original ranks that were lost."""
        from .parallel.bootstrap import alive_nodes, form_group
        from .parallel.elastic import Excluded, lost_blocks, ring_placement, settle_membership

        m, c = self.membership, self._elastic_cfg
        if m is None:
            raise RuntimeError("recover(): this runtime's group was not formed by Join")
        self._abort_generation()
        if self._exchange is not None and self._exchange.pending():
            # (elastic Sends never defer; a deferred Send of the failed generation keeps
            # STATUS_OVERFLOW on its pending messages -- say so instead of dropping it silently)
            _log.warning("recover: %d deferred Send(s) of generation %d left unresolved (STATUS_OVERFLOW)",
                         self._exchange.drop_pending(), m["gen"])
        self._exchange = None
        if self._native:
            # the compiled lifecycle: abort, lease-driven settle, the first current record in
            # the store wins, the next generation's communicator, ring adoption
            dp = self.group.dp
            try:
                plan = self.group.recover(float(c["grace_s"]))
            except RuntimeError as e:
                if "excluded" in str(e):
                    raise Excluded(str(e)) from e
                raise
            dp.reset_watchdog()
            lost = list(plan["lost"])
            m["members"], m["gen"] = list(plan["members"]), m["gen"] + 1
            self.rank, self.world = self.group.rank, self.group.size
            own = {n: list(rs) for n, rs in dict(dp.placement(m["members"])).items()}
            self._rehome(own, list(plan["blocks"]), list(plan["kept_from"]), list(plan["from_replica"]))
        else:
            proposal = settle_membership(lambda: alive_nodes(c["registry"], self.service), m["members"], m["me"],
                                         c["grace_s"])
            members, tcp = form_group(c["store"], c["local_addr"], m["me"], self.service, m["gen"] + 1, proposal,
                                      c["backend"], lambda r: None, timeout_s=c["timeout_s"])
            self._tcp_store = tcp
            self._cpu_failed = None
            lost = lost_blocks(m["nodes0"], m["members"], members)
            m["members"], m["gen"] = list(members), m["gen"] + 1
            self.rank, self.world = members.index(m["me"]), len(members)
            own = ring_placement(m["nodes0"], m["members"])
            nb = own[m["me"]]
            kept = [self.blocks.index(r) if r in self.blocks else -1 for r in nb]
            self._rehome(own, nb, kept, [k < 0 and r in self.replicas for r, k in zip(nb, kept)])
        self.recoveries += 1
        self._registry_changes += 1
        _log.warning("data-plane generation %d formed: world %d, lost original ranks %s, hosting %s", m["gen"],
                     self.world, lost, self.blocks)
        trace.mark("ptype.regenerated")
        return lost

    @property
    def _native(self) -> bool:
        """Whether the group is the compiled DataPlane (parallel/native_group.py)."""
        return self.group is not None and hasattr(self.group, "comm_ptr")

    def _abort_generation(self) -> None:
        """Abort the current data-plane generation (never raises)."""
        if self._native:
            try:
                self.group.abort()
            except Exception:
                pass
        else:
            from .parallel.elastic import abort_group

            abort_group()

    def _rehome(self, own: dict, new_blocks: list, kept_from: list, from_replica: list) -> None:
        """Apply a placement: keep the state of blocks that stay, adopt lost blocks
        from their replicas (else zero), rebuild the registry table and the
        dispatcher, republish this rank's record.  ``own``: node -> original ranks."""
        m = self.membership
        P, W0 = self.actors, self.world0
        state = torch.zeros(P * len(new_blocks), dtype=torch.int64, device=self.device)
        self.restored = []
        for j, (r, k, rep) in enumerate(zip(new_blocks, kept_from, from_replica)):
            if k >= 0:
                state[j * P:(j + 1) * P] = self.state[k * P:(k + 1) * P]
            elif rep and r in self.replicas:
                state[j * P:(j + 1) * P] = self.replicas[r]
                self.restored.append(r)
        self.blocks, self.state, self.replicas = list(new_blocks), state, {}
        self.table.clear()
        k = torch.arange(P, dtype=torch.int64)
        for node, rs in own.items():
            rank = m["members"].index(node)
            for j, r in enumerate(rs):
                self.table.upsert(actor_keys(r + W0 * k), torch.full((P,), rank, dtype=torch.int32),
                                  (j * P + k).to(torch.int32))
        self.table.enable_directory(W0 * P, affine_world=W0)
        self._ltable = None
        if self.server is not None:  # the dispatcher serves the new state tensor
            name = self.server.shm_name
            self.server.close()
            self.server = hip().DeviceServer(self.device.index or 0, self._ring, self.state.data_ptr(),
                                             self.mailboxes, self.delay_us, self._idle_ms, 60.0, name)
        for _, b in getattr(self, "_bridges", []):  # the net/rpc server keeps their handles: retarget in place
            b.retarget(self.table.table.data_ptr(), self.table.cap, self.state.data_ptr(), self.state.numel())
        if self.mirror is not None:
            self.mirror.set_generation(m["gen"])
        if self.shard_lease is not None:
            self.shard_lease.update(rank=self.rank, world=W0, count=P, gen=m["gen"], blocks=list(new_blocks))

    def tell(self, batch: B.MsgBatch, outbox_capacity: int | None = None):
        """Fire-and-forget delivery that lets GPU handlers send on: ``batch`` is
        delivered, and whatever the handlers emit (actor-to-actor ``Forward``
        tells) is routed epoch after epoch until every outbox of the group is
        empty.  Collective.  Returns ``(epochs, messages delivered here)``."""
        from .ops.outbox import DeviceOutbox

        cap = int(outbox_capacity or self.max_batch)
        if getattr(self, "_outbox", None) is None or self._outbox.cap < cap:
            self._outbox = DeviceOutbox(cap, device=self.device)
        return self.exchange.pump(self._outbox, initial=batch)

    def call(self, method: int, actor: int, a0: int = 0, a1: int = 0, a2: int = 0, timeout: float = 30.0):
        """Single synchronous call to a local actor.  Through the persistent
        dispatcher (no kernel launch) -- except ordered methods, which must queue
        behind the actor's other messages: those go through its HBM mailbox."""
        from .ops.records import method_ordered

        if not self.on_gpu or method_ordered(method):
            b = B.MsgBatch(torch.tensor([actor], dtype=torch.int32, device=self.device),
                           torch.tensor([a0], dtype=torch.int64, device=self.device),
                           torch.tensor([a1], dtype=torch.int64, device=self.device),
                           torch.tensor([a2], dtype=torch.int64, device=self.device), int(method))
            if self.on_gpu:
                mb = self.exchange._mailboxes()
                v, st = mb.send(b, self._local_table(), self.state, rank_self=0, delay_us=self.delay_us, ordered=True)
                return int(v.item()), int(st.item())
            v, st = B._handler_ref(torch.tensor([int(method)]), torch.tensor([actor]), b.a0, b.a1, b.a2, self.state)
            return int(v[0]), int(st[0])
        with trace.range("ptype.call"):
            v, st, _ = self.server.call(int(method), int(actor), int(a0), int(a1), int(a2), float(timeout))
        return v, st

    def _local_table(self):
        """Identity table of this rank's mailboxes (a local call names the mailbox)."""
        if getattr(self, "_ltable", None) is None:
            t = RegistryTable(2 * self.actors, device=self.device)
            ids = torch.arange(self.actors, dtype=torch.int64)
            t.upsert(actor_keys(ids), torch.zeros(self.actors, dtype=torch.int32), ids.to(torch.int32))
            t.enable_directory(self.actors)
            self._ltable = t
        return self._ltable

    def serve(self, server, service: str, methods: dict, batch: bool = False) -> None:
        """Expose GPU handlers over net/rpc: ``methods`` maps a Go method name to
        ``(method_id, [arg field names])`` -- e.g. ``{"Multiply": (1, ["A", "B"])}``.
        ``batch``: also serve each method in batches through the GPU gob bridge
        (K4: a connection's pipelined requests decoded on the GPU into mailbox
        columns, ``gob_bridge``)."""
        self.host(service)
        if batch and self.world0 > 1:
            # the bridge routes with mailbox = actor id on this GPU: right only when
            # this rank hosts every actor
            raise ValueError("serve(batch=True): the GPU gob bridge serves single-rank runtimes only")
        for name, (mid, fields) in methods.items():
            server.RegisterDevice(f"{service}.{name}", self.server, mid, fields)
            if batch:
                server.RegisterDeviceBatch(f"{service}.{name}", self.gob_bridge(mid).handle(), fields)

    def gob_bridge(self, method_id: int, actor: int = 0):
        """The GPU gob bridge of ``method_id`` (csrc/hip/gob_bridge.hpp): batches
        of gob argument messages decoded on this GPU and sent through mailboxes of
        their own (separate rings: the bridge runs on its own stream), answering
        actor ``actor`` (or the request's actor field).  Kept alive by the runtime."""
        from .ops.mailbox import Mailboxes

        if not self.on_gpu:
            raise RuntimeError("gob_bridge needs a GPU runtime (use _core.host_batch_multiply() on the host)")
        self._bridges = getattr(self, "_bridges", [])
        mb = Mailboxes(self.device, shards=64, slots=1 << 12)
        # ordered after the runtime's stream both ways: a bridge batch and a Send never
        # update actor state concurrently
        b = hip().GobBridge(self.device.index or 0, mb._m, int(method_id), int(actor), self.table.table.data_ptr(),
                            self.table.cap, self.state.data_ptr(), self.state.numel(), self.delay_us,
                            torch.cuda.current_stream(self.device).cuda_stream)
        self._bridges.append((mb, b))
        return b

    # ------------------------------------------------------------------ snapshots (C14)
    def snapshot_to_host(self) -> dict:
        """Actor state + packed registry mirror in pinned host DRAM, on a side
        stream (the routing stream keeps running): the state by one DMA copy, the
        mirror by K7 writing straight into its pinned buffers.  The pinned
        buffers are allocated once and reused; the returned tensors are views
        valid until the next snapshot."""
        side = torch.cuda.Stream(self.device) if self.on_gpu else None
        if self.on_gpu:
            side.wait_stream(torch.cuda.current_stream(self.device))
            if getattr(self, "_snap_state", None) is None or self._snap_state.numel() != self.state.numel():
                self._snap_state = torch.empty(self.state.shape, dtype=self.state.dtype, pin_memory=True)
            with torch.cuda.stream(side):
                self._snap_state.copy_(self.state, non_blocking=True)
            h_state = self._snap_state
        else:
            h_state = self.state.clone()
        ent, exp = self.table.snapshot_to_host(side)
        return {"state": h_state, "table": ent, "expiry": exp,
                "meta": torch.tensor([self.rank, self.world, self.actors], dtype=torch.int64)}

    def save(self, path: str) -> dict:
        from safetensors.torch import save_file

        t0 = time.perf_counter()
        snap = self.snapshot_to_host()
        nbytes = sum(v.numel() * v.element_size() for v in snap.values())
        save_file({k: v.contiguous() for k, v in snap.items()}, path)
        return {"bytes": nbytes, "seconds": time.perf_counter() - t0}

    def restore(self, path: str) -> None:
        from safetensors.torch import load_file

        snap = load_file(path)
        if int(snap["meta"][2]) != self.actors:
            raise ValueError("snapshot actor count does not match this runtime")
        self.restore_from(snap)

    def restore_from(self, snap: dict) -> None:
        """Actor state and registry mirror from a snapshot dict (``snapshot_to_host``
        output): one host->device copy each, the mirror re-inserted by one packed
        upsert kernel."""
        pin = self.on_gpu and not snap["state"].is_pinned()
        st = snap["state"].pin_memory() if pin else snap["state"]
        self.state.copy_(st, non_blocking=self.on_gpu)
        self.table.clear()
        if snap["table"].numel():
            ent, exp = snap["table"], snap["expiry"]
            if self.on_gpu and not ent.is_pinned():
                ent, exp = ent.pin_memory(), exp.pin_memory()
            self.table.load_packed(ent, exp)
        self._registry_changes += 1

    # ------------------------------------------------------------------ stats / teardown
    def stats(self) -> dict:
        from dataclasses import asdict

        from .utils.trace import hist_percentile

        out = {"rank": self.rank, "world": self.world, "actors": self.actors, "device": str(self.device)}
        if self.server is not None:
            h = self.server.rtt_histogram()
            out["dispatcher"] = {"processed": self.server.processed, "launches": self.server.launches,
                                 "exits_idle": self.server.exits_idle, "exits_lifetime": self.server.exits_lifetime,
                                 "running": self.server.running, "calls": int(sum(h)),
                                 "rtt_p50_ns_le": hist_percentile(h, 50), "rtt_p99_ns_le": hist_percentile(h, 99),
                                 "rtt_log2ns_hist": h}
        out["registry"] = {"live": self.table.live, "tombstones": self.table.tombstones,
                           "generation": self.table.generation, "capacity": self.table.cap,
                           "directory_ids": self.table.dir_n}
        out["shards"] = ({k: v["record"] for k, v in self.mirror.shards.items()} if self.mirror is not None
                         else self.shards)
        if self.mirror is not None:
            out["mirror"] = {"applies": self.mirror.applies, "actors": self.mirror.actors}
        if self._exchange is not None:
            out["exchange"] = asdict(self._exchange.stats())
        if self.ledger is not None:
            out["ledger"] = self.ledger.read()
        out["coalesce"] = (dict(self._coalescer.counters) if self._coalescer is not None
                           else {"sends": 0, "messages": 0, "executed": 0})
        out["cache"] = (dict(self._cache.counters, entries=self._cache.entries) if self._cache is not None
                        else {"sends": 0, "messages": 0, "hits": 0, "sent": 0, "clears": 0, "entries": 0})
        if self._breaker is not None:
            b, r = self._breaker, self._breaker.read()  # (one host read of the device counters)
            out["breaker"] = dict(b.counters, open=r["open"], trips=r["trips"], closes=r["closes"], oob=r["oob"],
                                  actors=b.n, threshold=b.threshold, cooldown=b.cooldown)
        else:
            out["breaker"] = {"sends": 0, "messages": 0, "rejected": 0, "sent": 0, "open": 0, "trips": 0, "closes": 0,
                              "oob": 0, "actors": 0, "threshold": 0, "cooldown": 0}
        if self._limiter is not None:
            lim, r = self._limiter, self._limiter.read()  # (one host read of the device counters)
            out["limit"] = dict(lim.counters, throttled=r["throttled"], oob=r["oob"], actors=lim.n, rate=lim.rate,
                                burst=lim.burst)
        else:
            out["limit"] = {"sends": 0, "messages": 0, "rejected": 0, "sent": 0, "throttled": 0, "oob": 0, "actors": 0,
                            "rate": 0, "burst": 0}
        out["scatter"] = dict(self._scatter_counters)
        t = self._topics.get(self.service)
        out["topics"] = dict(t.stats() if t is not None else {"topics": 0, "segments": 0, "subscribers": 0, "records": 0,
                                                              "bad_records": 0, "applied_rev": 0},
                             **self._topic_counters)
        out["queues"] = dict(t.queue_stats() if t is not None else {"queues": 0, "members": 0, "segments": 0},
                             rows=self._queue_rows)
        out["dead_letters"] = (self._dlq.read() if self._dlq is not None  # (one host read of the control line)
                               else {"entries": 0, "appended": 0, "unread": 0, "dropped": 0, "sends": 0, "torn": 0,
                                     "redrives": 0, "redriven": 0})
        out["timers"] = (self._timers.read() if self._timers is not None  # (one host read of the control line)
                         else {"now": 0, "head": 0, "tail": 0, "live": 0, "runs": 0, "refused": 0, "delivered": 0,
                               "full": 0, "torn": 0, "entries": 0, "horizon": 0, "max_runs": 0})
        return out

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        if self._exchange is not None and self._exchange.pending():
            # deferred re-sends (world > 1) resolve before the group goes away (collective:
            # every rank closes); a failure here is reported, the teardown goes on
            try:
                self._exchange.flush()
            except Exception as e:  # noqa: BLE001
                _log.warning("close: deferred re-sends not resolved: %s", str(e)[:300])
        for lease in getattr(self, "_replica_leases", {}).values():
            lease.close()
        for t in self._topics.values():
            t.close()
        if self.mirror is not None:
            self.mirror.close()
        if self.shard_lease is not None:
            self.shard_lease.close()
        if self.server is not None:
            self.server.close()
        if self._owns_group and self._native:
            self.group.close()  # abort: never waits on a member that may be gone
        elif self._owns_group:
            import torch.distributed as dist

            if dist.is_initialized():
                try:
                    dist.destroy_process_group()
                except Exception:
                    pass
            self._tcp_store = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_ok(status: torch.Tensor) -> bool:
    return bool((status == STATUS_OK).all())
