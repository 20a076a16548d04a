"""The ptype ``cluster`` API for Python, backed by the C++ control plane.

Names follow the reference package (``cluster.Join``, ``ConfigFromFile``,
``Cluster.Registry`` / ``Store`` / ``MemberList`` / ``NewClient`` / ``Close``,
``Client.Call`` / ``Go`` / ``Close`` / ``ConnectionErrs``, ``Registry.Register`` /
``Services`` / ``WatchService``, ``KVStore.Get`` / ``Put`` / ``Delete``, the
``With*`` option helpers, ``ErrNoKey``, ``ErrNoClientAvailable``,
``DefaultConnConfig``), plus the north-star entry points ``New`` (= ``Join``),
``Client.Send`` (batched device-native submit) and ``Serve`` (server-side
registration, which the reference leaves to stdlib net/rpc).

Reference: cluster/cluster.go, cluster/config.go, cluster/registry.go,
cluster/store.go, cluster/store_config.go, cluster/rpc.go.
"""
from __future__ import annotations

import inspect
import json
from typing import Any, Callable, Iterable

from . import _core
from ._core import (  # noqa: F401  (re-exported API surface)
    CallChannel,
    ConfigError,
    ConnConfig,
    Context,
    ErrChannel,
    IntChannel,
    KvClient,
    LearnerNotReadyError,
    MemberConfig,
    MemberError,
    NoClientAvailableError,
    NoKeyError,
    Node,
    NodesChannel,
    PtypeError,
    RpcError,
    RpcServer,
    ShutdownError,
    TimeoutError,
    UnavailableError,
)
from .gobtypes import GoSlice, GoStruct, GoUint  # noqa: F401

# ---------------------------------------------------------------- sentinels
ErrNoKey = NoKeyError                       # cluster/store.go:15
ErrNoClientAvailable = NoClientAvailableError  # cluster/rpc.go:16
ErrLearnerNotReady = LearnerNotReadyError

# ---------------------------------------------------------------- options (store_config.go)
SortByKey, SortByVersion, SortByCreateRevision, SortByModRevision, SortByValue = range(5)
SortNone, SortAscend, SortDescend = range(3)

WithPrefix = _core.with_prefix
WithLimit = _core.with_limit
WithRev = _core.with_rev
WithRange = _core.with_range
WithFromKey = _core.with_from_key
WithSerializable = _core.with_serializable
WithKeysOnly = _core.with_keys_only
WithCountOnly = _core.with_count_only
WithLease = _core.with_lease


def WithSort(target: int, order: int):
    return _core.with_sort(int(target), int(order))


def GetPrefixRangeEnd(prefix: str | bytes) -> str | bytes:
    """Range end of a prefix on its bytes (store_config.go:41-58); returns str
    when the result is valid UTF-8, else bytes ("\\x00" when no end exists)."""
    b = bytearray(prefix.encode() if isinstance(prefix, str) else prefix)
    for i in range(len(b) - 1, -1, -1):
        if b[i] < 0xFF:
            b[i] += 1
            out = bytes(b[: i + 1])
            break
    else:
        out = b"\x00"
    if isinstance(prefix, str):
        try:
            return out.decode()
        except UnicodeDecodeError:
            return out
    return out


def DefaultConnConfig() -> ConnConfig:
    """{MaxConnections 3, InitialNodeTimeout 5 s, DebounceTime 3 s, Retries 2} (rpc.go:33-38)."""
    return _core.default_conn_config()


def background() -> Context:
    return Context.background()


def _ctx(ctx) -> Context:
    return ctx if ctx is not None else Context.background()


# ---------------------------------------------------------------- config
Config = _core.Config


def ConfigFromFile(path: str) -> Config:
    """Load the ptype YAML and its member (etcd) YAML (cluster/config.go:23-46)."""
    return _core.config_from_file(path)


config_from_file = ConfigFromFile


# ---------------------------------------------------------------- registry
class Registry:
    """Service registry over the Raft-replicated store (cluster/registry.go)."""

    def __init__(self, core):
        self._r = core

    def Register(self, ctx, serviceName: str, nodeName: str, host: str, port: int) -> None:
        self._r.register(_ctx(ctx), serviceName, nodeName, host, int(port))

    def Services(self, ctx=None) -> dict:
        return self._r.services(_ctx(ctx))

    def WatchService(self, ctx, serviceName: str) -> NodesChannel:
        return self._r.watch_service(_ctx(ctx), serviceName)

    def nodes(self, ctx, serviceName: str):
        return self._r.nodes(_ctx(ctx), serviceName)

    register = Register
    services = Services
    watch_service = WatchService

    @property
    def kv(self):
        return self._r.kv

    def close(self):
        self._r.close()


def new_etcd_registry(endpoints: list[str]) -> Registry:
    return Registry(_core.EtcdRegistry(list(endpoints)))


class KVStore:
    """Shared KV store under the ``store/`` prefix (cluster/store.go)."""

    def __init__(self, core):
        self._s = core

    def Get(self, ctx, key: str, *opts) -> list[str]:
        return self._s.get(_ctx(ctx), key, *opts)

    def Put(self, ctx, key: str, value: str, *opts) -> None:
        self._s.put(_ctx(ctx), key, value, *opts)

    def Delete(self, ctx, key: str, *opts) -> None:
        self._s.delete(_ctx(ctx), key, *opts)

    get, put, delete = Get, Put, Delete

    def close(self):
        self._s.close()


def new_kv_store(endpoints: list[str]) -> KVStore:
    return KVStore(_core.KVStore(list(endpoints)))


# ---------------------------------------------------------------- client
class Client:
    """RPC client with the reference's balancer semantics (cluster/rpc.go).

    ``Call`` returns the reply (Go writes it through a pointer); ``Go`` returns
    a call handle whose ``done`` channel later delivers it; ``Send`` is the
    batched device-native path (see ``ptype_amd.runtime``).
    """

    def __init__(self, core: _core.RpcClient, runtime=None, service: str = "", local_addr: str = "",
                 max_connections: int = 3):
        self._c = core
        self._rt = runtime
        self.service = service
        self._local_addr, self._max_connections = local_addr, int(max_connections)
        self._router = None  # replica routing of Send (parallel/replicas.py), when the service is replicated
        self._router_checked = False
        self._tag = None  # FNV-1a64 of the service name: what this client's dead letters are filed under
        self._topic_leases: dict = {}  # (topic, name) -> the kept-alive lease of an ephemeral subscription

    def _replica_router(self):
        if not self._router_checked:
            self._router_checked = True
            if self._rt.has_replicas(self.service):
                self._router = self._rt.replica_router(self.service, self._max_connections, self._local_addr)
        return self._router

    def Call(self, serviceMethod: str, args: Any) -> Any:
        return self._c.call(serviceMethod, args)

    def Go(self, serviceMethod: str, args: Any, done: CallChannel | None = None):
        return self._c.go(serviceMethod, args, done)

    def Send(self, batch, retries: int | None = None, retry_on=None, coalesce: bool | None = None,
             cache: bool | None = None, gather=None, breaker: bool | None = None, limit: bool | None = None,
             dead_letter: bool | None = None, **kw):
        """Batched submit of a ``MsgBatch`` to GPU actors of this service:
        RCCL epoch exchange across ranks, device dispatch, replies in order.

        Asynchronous like ``Go`` (cluster/rpc.go:69-105): it returns device tensors
        ``(value, status)`` as soon as the Send is enqueued, with no host wait on
        it.  With more than one rank, a message that overflowed its region (skewed
        traffic beyond the agreed capacity) reads STATUS_OVERFLOW until its re-send
        -- at most two Sends later, or at ``Flush()`` -- writes its reply into the
        same tensors; keep ``batch`` unchanged until then.

        ``retries``: the reference's ``withRetry`` (cluster/rpc.go:107-116) on the
        batch -- every message whose status is in ``retry_on`` (default
        ``STATUS_FAILED``) is sent again, up to ``retries`` times, each time to the
        next replica of the round robin, and its reply replaces the failed one.
        Opt-in (``retries=client.cfg.retries`` for the reference's behaviour): it
        costs a host read per Send, and a retried message runs after the rest of
        its batch, so a batch with an ordered method is refused.  ``None``: one
        attempt, exactly the Send above.

        ``account=`` (keyword, forwarded to ``DeviceRuntime.send``): whether the
        Send ledger (``gpu.ledger: true``; ``Stats()["runtime"]["ledger"]``)
        accounts this Send -- per-method call counts, a digest of every reply, an
        audit of the pure methods and per-actor load, folded in on the device once
        the replies are final.  ``None`` follows the runtime's setting, ``False``
        skips this Send, ``True`` without a ledger raises.  An accounted Send does
        not defer its overflow re-sends, and the ledger is the caller's view: each
        rank accounts the batches it sent.

        ``coalesce``: Go's ``singleflight`` on the batch -- messages of a pure method
        (``Calculator.Multiply``, ``Prime.Check``, ``Echo``) with equal ``(actor,
        method, a0, a1, a2)`` are sent once and every duplicate gets that reply, so
        the result equals the plain Send's element for element (ops/coalesce.py).
        ``None`` follows ``gpu.coalesce``, ``False`` skips this Send.  It costs a
        hash pass over the batch and one host read per Send, is refused under graph
        capture and never defers its overflow re-sends;
        ``Stats()["runtime"]["coalesce"]`` counts messages and executed leaders.

        ``cache``: the cache a Go service keeps next to ``singleflight`` -- a call of a
        pure method whose ``STATUS_OK`` reply an earlier cached Send of this process
        stored (same key) is answered from the HBM reply cache and not sent
        (ops/reply_cache.py); only the misses travel, after coalescing if both are
        on.  The result equals the plain Send's element for element: a non-OK reply
        is never stored, any other method runs as often as it appears, and the
        cache is cleared whenever the registry (or this client's replica set)
        changed since the last cached Send.  ``None`` follows ``gpu.cache``, ``False``
        skips this Send; ``gpu.cache_entries`` sizes the direct-mapped table (64 B
        per entry, default ``1 << 20``).  It costs one read-only probe per message
        and one host read per Send, is refused under graph capture and never defers;
        ``Stats()["runtime"]["cache"]`` counts messages, hits and misses sent.  The
        cache belongs to the process's runtime: cached Sends must all be issued on one
        stream, and clients of different replicated services (different routers)
        that alternate on it clear it on every Send.

        ``gather``: the gather half of a scatter-gather (the optimus coordinator's
        ``watchReplies``) -- an ``ops.gather.Gather(group, groups, op, sentinel)`` over
        this batch folds the replies into one result per group on the device: ``sum``,
        ``min``, ``max`` or ``first_ne`` over the ``STATUS_OK`` replies of each group, with
        the group's first error in message order (ops/gather.py).  The return value
        stays ``(value, status)`` per message; the results are the object's tensors
        (``value``, ``status``, ``n_ok``, ``count``, ``bad_row``, ``oob``), valid in stream
        order after the Send and overwritten by the next Send that carries it.  It
        runs once, on the full batch's final replies (after coalescing, the cache,
        retries and overflow re-sends), costs two kernel launches and no host read,
        and like an accounted Send never defers its overflow re-sends.

        ``breaker``: the circuit breaker a Go service puts around a flaky dependency
        (``sony/gobreaker``), per actor -- an actor whose messages failed
        ``gpu.breaker_threshold`` times in a row (``STATUS_FAILED``, ``STATUS_NO_ACTOR`` or
        ``STATUS_NOT_DELIVERED`` after the retries, no ``STATUS_OK`` in between) is not sent
        to for the next ``gpu.breaker_cooldown`` guarded Sends: its messages come back
        ``(0, STATUS_BREAKER_OPEN)`` at once.  Then one probe message per Send -- the lowest
        of the batch that addresses it -- decides: OK closes the actor, a failure opens
        it again (ops/breaker.py).  It wraps the retried call: the order is coalesce,
        cache, breaker, retries.  A batch that trips nothing returns exactly what the
        plain Send returns.  ``None`` follows ``gpu.breaker``, ``False`` skips this Send;
        ``gpu.breaker_actors`` sizes the dense state table (8 B per actor id, default
        every actor of the service; ids past it are never guarded).  It costs one pass
        over the statuses and one host read per Send (a second one while any actor is
        open), is refused under graph capture and never defers;
        ``Stats()["runtime"]["breaker"]`` counts messages, rejected and sent ones, open
        actors, trips and closes.  Every actor closes when the registry (or this
        client's replica set) changed, and guarded Sends must all be issued on one
        stream.

        ``limit``: the rate limiter a Go service puts in front of a dependency
        (``golang.org/x/time/rate``), per actor -- a token bucket that gains ``gpu.limit_rate``
        tokens per limited Send and holds at most ``gpu.limit_burst``.  Every message that
        travels costs one token; of an actor whose messages in this batch exceed its tokens
        the first ones in message order travel and the others come back
        ``(0, STATUS_THROTTLED)`` at once (ops/limit.py).  It is the innermost wrapper: the
        order is coalesce, cache, breaker, limit, retries, so followers, cached hits and
        breaker-rejected messages cost nothing and a retried message costs one token.
        ``None`` follows ``gpu.limit``, ``False`` skips this Send; ``gpu.limit_actors`` sizes
        the dense bucket table (8 B per actor id, default every actor of the service; ids
        past it are never limited).  It costs one pass over the actor ids and one host read
        per Send (more passes and a second read only while some actor is over its quota), is
        refused under graph capture and never defers; ``Stats()["runtime"]["limit"]`` counts
        messages, throttled and sent ones.  Registry changes reset nothing, and limited
        Sends must all be issued on one stream.

        ``dead_letter``: the dead-letter queue of an actor runtime (protoactor's
        ``DeadLetterEvent``, Akka's ``deadLetters``) -- the messages that still failed after all
        of the above (a final status in ``gpu.dead_letter_mask``, by default every failure
        status 1 to 6) are filed with their whole call in a ring of ``gpu.dead_letter_entries``
        64-byte records in HBM (ops/dead_letters.py), because ``batch`` is the caller's and
        may be gone when anyone asks.  ``None`` follows ``gpu.dead_letters``, ``False`` skips
        this Send, ``True`` without a queue raises.  It runs once, on the full batch's final
        replies (a coalesced follower of a failed leader gets its own letter), costs two
        kernel launches and no host read, is legal under graph capture and like an accounted
        Send never defers its overflow re-sends.  The newest letters win: a ring that
        overflows counts what it overwrote in ``dropped``.  ``DeadLetters()`` looks at the
        queue, ``Redrive()`` re-sends it; ``Stats()["runtime"]["dead_letters"]`` counts.  The
        queue belongs to the process's runtime, not to this client: letters are filed under
        ``tag`` = FNV-1a64 of the client's service name, which is reported and not filtered
        on."""
        if self._rt is None:
            raise RuntimeError("Client.Send needs the cluster's device runtime (Join with a gpu: section)")
        if retries:
            kw.update(retries=int(retries), retry_on=retry_on)
        if coalesce is not None:
            kw.update(coalesce=bool(coalesce))
        if cache is not None:
            kw.update(cache=bool(cache))
        if gather is not None:
            kw.update(gather=gather)
        if breaker is not None:
            kw.update(breaker=bool(breaker))
        if limit is not None:
            kw.update(limit=bool(limit))
        if dead_letter is not None:
            kw.update(dead_letter=bool(dead_letter))
        if dead_letter is not False:  # (the tag of a Send that files nothing is not looked at)
            kw.setdefault("dead_letter_tag", self._dead_letter_tag())
        return self._rt.send(self.service, batch, router=self._replica_router(), **kw)

    def _dead_letter_tag(self) -> int:
        if self._tag is None:
            from .ops.dead_letters import fnv1a64

            self._tag = fnv1a64(self.service)
        return self._tag

    def DeadLetters(self, max_letters: int | None = None, drain: bool = False):
        """The unread letters of the runtime's dead-letter queue (at most ``max_letters``),
        oldest first: an ``ops.dead_letters.Letters`` with the columns ``seq``, ``row``,
        ``status``, ``actor``, ``method``, ``attempts``, ``a0``, ``a1``, ``a2`` and ``tag`` on the
        device, ``n`` and ``torn``.  ``drain``: they leave the queue.  The queue is per runtime:
        letters of every client of this process are in it, told apart by ``tag``."""
        if self._rt is None:
            raise RuntimeError("Client.DeadLetters needs the cluster's device runtime (Join with a gpu: section)")
        return self._rt.dead_letters(max_letters, drain)

    def Redrive(self, max_letters: int | None = None, **kw):
        """The redrive of a message queue's dead-letter queue: up to ``max_letters`` letters
        (and at most one Send's worth) are taken out of the runtime's queue and sent again
        as one batch, through ``Send`` with every keyword it takes (``retries``, ``coalesce``,
        ``cache``, ``breaker``, ``limit``, ``account``).  A letter that fails again is filed
        again with ``attempts + 1`` and this client's tag, one that succeeds has left the
        queue.  Returns an ``ops.dead_letters.Redrive``: ``letters``, ``value``, ``status``.
        The queue is per runtime and the tag is not filtered on: ``Redrive`` sends whatever
        it takes -- other clients' letters included -- to this client's own service.  The
        keywords are checked before a letter is taken; an error the Send raises later than
        that finds the letters taken, they are not put back.  It
        reads the queue on the host (refused under graph capture) and is a collective Send
        at world > 1."""
        if self._rt is None:
            raise RuntimeError("Client.Redrive needs the cluster's device runtime (Join with a gpu: section)")
        kw.setdefault("dead_letter_tag", self._dead_letter_tag())
        return self._rt.redrive(self.service, max_letters, router=self._replica_router(), **kw)

    def Schedule(self, batch, delay, tag: int | None = None):
        """Delayed messages, the ``scheduleOnce`` / ``SendOnce`` / ``DelaySeconds`` of the batched
        path: row ``i`` of ``batch`` is kept, with its whole call, in the runtime's timer queue
        in HBM (ops/timers.py) and sent by the ``Tick()`` ``delay[i]`` ticks from now.  ``delay``
        is an int or an int32 column; a row whose delay is outside ``[1, gpu.timer_horizon]`` is
        not filed and counted in ``refused``.  ``tag`` defaults to this client's (FNV-1a64 of its
        service, as for dead letters).  Returns an ``ops.timers.Scheduled``: ``n``, ``refused``,
        ``first_ticket``, ``now``; raises ``ops.timers.TimerQueueFull``, with nothing filed, when the
        ring (``gpu.timer_entries``) or the run table (``gpu.timer_runs`` pending Schedules) lacks
        room.  Time is explicit: the clock counts ticks and only ``Tick()`` moves it.  Routing
        happens when a message is due, not now.  It reads its counts on the host (refused
        under graph capture).  The queue is per runtime, like the dead-letter queue."""
        if self._rt is None:
            raise RuntimeError("Client.Schedule needs the cluster's device runtime (Join with a gpu: section)")
        return self._rt.schedule(batch, delay, self._dead_letter_tag() if tag is None else int(tag))

    def Tick(self, ticks: int | None = None, **kw):
        """Advance the runtime's clock by one tick and send the messages that are due, in
        ticket order, as one batch through ``Send`` with every keyword it takes (``retries``,
        ``coalesce``, ``cache``, ``breaker``, ``limit``, ``dead_letter``, ``gather``, ``account``).
        Returns an ``ops.timers.Ticked``: ``due`` (the records: ``ticket``, ``row``, ``actor``,
        ``method``, ``delay``, ``t0``, ``a0``, ``a1``, ``a2``, ``tag``, ``n``, ``torn``), ``value``,
        ``status``.  The queue is per runtime and the tag is not filtered on: ``Tick`` sends
        whatever is due -- other clients' messages included -- to this client's own service.
        The keywords are checked before the clock moves.  ``ticks=n``: ``n`` single ticks, a
        list.  It reads ``n_due`` on the host (refused under graph capture) and is a collective
        Send at world > 1."""
        if self._rt is None:
            raise RuntimeError("Client.Tick needs the cluster's device runtime (Join with a gpu: section)")
        if kw.get("dead_letter") is not False:
            kw.setdefault("dead_letter_tag", self._dead_letter_tag())
        return self._rt.tick(self.service, router=self._replica_router(), ticks=ticks, **kw)

    def Timers(self) -> dict:
        """The timer queue's counters: ``now``, ``head``, ``tail``, ``live``, ``runs``, ``refused``,
        ``delivered``, ``full``, ``torn`` and its sizes (one host read);
        ``Stats()["runtime"]["timers"]`` has the same."""
        if self._rt is None:
            raise RuntimeError("Client.Timers needs the cluster's device runtime (Join with a gpu: section)")
        return self._rt.timers()

    def Ask(self, questions, scatter, op: str = "sum", sentinel=None, **kw):
        """Scatter-gather on the device: the optimus coordinator's ``splitWork`` ..
        ``watchReplies`` (coordinator.go:67-98) for any rule and op.  ``scatter`` -- an
        ``ops.scatter.Scatter``: ``Scatter.ranges(step, n_actors, first_lo)`` is
        ``splitWork``, ``Scatter.members(offsets, members)`` one call to every member of a
        group -- expands the Q ``questions`` (a short ``MsgBatch``) into T calls with HIP
        kernels, the calls go through ``Send`` with every keyword it takes (``retries``,
        ``coalesce``, ``cache``, ``breaker``, ``limit``, ``dead_letter``, ``account``) and the replies are folded
        per question with ``op`` (``sum``, ``min``, ``max`` or ``first_ne`` against
        ``sentinel``).  Returns an ``ops.scatter.Answer``: ``value``, ``status``, ``n_ok``,
        ``count`` and ``bad_row`` per question, the expansion's ``first``, ``n`` and ``oob``,
        and the per-call ``(val, st)``.  It costs four launches and one 16-byte host read
        on top of the Send, so it is refused under graph capture (expand first and capture
        ``Send(exp.batch, gather=exp.gather(op))`` instead);
        ``Stats()["runtime"]["scatter"]`` counts asks, questions, rows and oob."""
        if self._rt is None:
            raise RuntimeError("Client.Ask needs the cluster's device runtime (Join with a gpu: section)")
        if kw.get("dead_letter") is not False:  # (as in Send: an Ask's letters carry this client's tag)
            kw.setdefault("dead_letter_tag", self._dead_letter_tag())
        return self._rt.ask(self.service, questions, scatter, op=op, sentinel=sentinel, router=self._replica_router(),
                            **kw)

    # ------------------------------------------------------------------ publish / subscribe
    def _topics(self):
        if self._rt is None:
            raise RuntimeError("topics need the cluster's device runtime (Join with a gpu: section)")
        return self._rt.topics(self.service)

    def _topic_name(self, name) -> str:
        name = self._rt._node if name is None else str(name)
        if not name or "/" in name:
            raise ValueError("a subscription's name is a non-empty string without '/'")
        return name

    def Subscribe(self, topic: int, actors=None, segments=None, name: str | None = None,
                  ephemeral: bool = False, queue: bool = False) -> int:
        """Subscribe actors of this service to ``topic`` (an int in ``[0, gpu.topics)``): the
        record ``store/_ptype/topics/<service>/<topic>/<name>`` (ops/topics.py has the schema)
        is put in the replicated store, so every client of the cluster sees it.  Exactly one
        of ``actors`` (ids: sorted, de-duplicated and cut into strided segments by
        ``ops.topics.segments_of``) and ``segments`` (``[[start, count, stride], ...]``, kept as
        given) names the subscribers; ``name`` (default: the node's name) identifies the
        subscription -- the same name replaces it.  Nothing is de-duplicated across
        subscriptions: an actor named by two of them gets every publication twice.
        Persistent by default (actors are re-homed when a rank fails, so a subscription
        outlives the node that made it); ``ephemeral=True`` attaches the record to a 2 s lease
        this client keeps alive, as the service registry does, so it lapses with its owner
        (or at ``Unsubscribe`` / ``Close``).  Returns the store revision of the put, after
        waiting until this process's topic table reflects it: a ``Publish`` issued after
        ``Subscribe`` returned sees the subscription; another process sees it once its own
        table caught up (a watch event; at the latest its next re-list, 0.5 s).

        ``queue=True`` makes it a **queue subscription** (competing consumers: Akka's
        ``sendOneMessageToEachGroup``, a NATS queue group, a Kafka consumer group): a publication
        to the topic reaches exactly ONE of the subscription's members -- the ids of its segments
        in order, at most ``2**31 - 1`` of them -- instead of all of them: a pool of workers
        behind a topic.  ``Publish`` picks the member (``key=``, ``by=``).  Re-subscribing under
        the same name replaces the subscription, whichever kind it was."""
        from .ops import topics as T

        if (actors is None) == (segments is None):
            raise ValueError("Subscribe: exactly one of actors= and segments=")
        table = self._topics()
        topic = int(topic)
        if not 0 <= topic < table.max_topics:
            raise ValueError(f"Subscribe: topic must be in [0, {table.max_topics}) (gpu.topics)")
        name = self._topic_name(name)
        segs = T.check_segments(T.segments_of(actors) if segments is None else segments)
        if not isinstance(queue, bool):
            raise ValueError("Subscribe: queue is True or False")
        if queue and sum(s[1] for s in segs) > T.MAX_QUEUE_MEMBERS:
            raise ValueError(f"Subscribe: a queue subscription holds at most {T.MAX_QUEUE_MEMBERS} members")
        record = {"segments": segs, "queue": True} if queue else {"segments": segs}
        key, value = T.topic_key(self.service, topic, name), json.dumps(record)
        kv = self._rt._kv
        old = self._topic_leases.pop((topic, name), None)
        if old is not None:
            old.close()
        if ephemeral:
            lease = _core.ShardLease(kv, key, value, T.LEASE_TTL_S)
            self._topic_leases[(topic, name)] = lease
            found = kv.get(key).kvs
            rev = int(found[0].mod_revision) if found else 0
        else:
            rev = int(kv.put(key, value.encode()))
        table.wait(rev)
        return rev

    def Unsubscribe(self, topic: int, name: str | None = None) -> int:
        """Delete the subscription ``name`` (default: the node's) of ``topic`` and close its
        lease if it was ephemeral.  Returns the store revision, after this process's topic
        table reflects it; a subscription that does not exist is not an error."""
        from .ops import topics as T

        table = self._topics()
        topic, name = int(topic), self._topic_name(name)
        lease = self._topic_leases.pop((topic, name), None)
        if lease is not None:
            lease.close()  # (revokes: the store deletes the record)
        _, rev = self._rt._kv.delete_rev(T.topic_key(self.service, topic, name))
        table.wait(int(rev))
        return int(rev)

    def Topics(self, queues: bool = False) -> dict:
        """The ordinary subscriptions this process's topic table holds, after applying what is
        pending: ``{topic: [(name, [[start, count, stride], ...])]}``, names in key order.
        ``queues=True``: every subscription as ``(name, segments, queue)``, a topic's ordinary
        ones (``queue`` False) before its queue subscriptions (True)."""
        table = self._topics()
        table.apply()
        return table.view(queues=True) if queues else table.view()

    def Publish(self, publications, op: str = "sum", sentinel=None, key=None, by=None, **kw):
        """Publish to topics: publication q of the ``MsgBatch`` -- its ``actor`` column names the
        topic, ``a0`` .. ``a2`` and the method are the payload -- becomes one call to every
        subscriber of the topic (``DistributedPubSub``'s ``Publish``, protoactor's cluster
        pub/sub), expanded on the device from strided segments without a per-subscriber table,
        sent with every keyword ``Send`` takes and folded per publication with ``op``, exactly
        as ``Ask`` does.  Returns an ``ops.scatter.Answer``: ``count[q]`` subscribers addressed,
        ``n_ok[q]`` deliveries that answered OK, ``value[q]`` the fold.  A topic outside ``[0,
        gpu.topics)`` addresses nobody and is counted in ``oob``; one without subscribers
        addresses nobody.  Refused under graph capture, like ``Ask``;
        ``Stats()["runtime"]["topics"]`` has the table's and the publishes' counters.

        After them a publication makes one call per **queue subscription** of its topic
        (``Subscribe(queue=True)``), in key order, to one member: ``by="key"`` (default) picks it
        from the hash of ``key[q]`` -- ``key`` an int64[Q] column, by default the publication's
        ``a0`` -- so every publication of one key reaches the same member while the membership
        stands (per-key ordering: Kafka's keyed records); ``by="index"`` walks the members round
        robin (publication ``q`` of the batch takes ``(seq + q) mod c``; ``seq`` advances by Q).
        ``count[q]`` is then the ordinary subscribers plus the queue subscriptions of the topic.
        ``Stats()["runtime"]["queues"]`` counts the queue subscriptions, their members and
        segments, and the queue rows published."""
        if self._rt is None:
            raise RuntimeError("Client.Publish needs the cluster's device runtime (Join with a gpu: section)")
        if kw.get("dead_letter") is not False:
            kw.setdefault("dead_letter_tag", self._dead_letter_tag())
        return self._rt.publish(self.service, publications, op=op, sentinel=sentinel, key=key, by=by,
                                router=self._replica_router(), **kw)

    def Flush(self) -> None:
        """Every earlier ``Send``'s replies final (pending re-sends run now)."""
        if self._rt is not None:
            self._rt.flush()

    def Tell(self, batch, **kw):
        """Batched fire-and-forget to GPU actors of this service; handlers may send
        on to other actors (device outbox), which is pumped until quiescent."""
        if self._rt is None:
            raise RuntimeError("Client.Tell needs the cluster's device runtime (Join with a gpu: section)")
        return self._rt.tell(batch, **kw)

    def Close(self) -> None:
        for lease in self._topic_leases.values():
            lease.close()
        self._topic_leases.clear()
        if self._router is not None:
            self._router.close()
        self._c.close()

    def ConnectionErrs(self) -> ErrChannel:
        return self._c.connection_errs()

    call, go, send, tell, close, flush, ask = Call, Go, Send, Tell, Close, Flush, Ask
    dead_letters, redrive = DeadLetters, Redrive
    schedule, tick, timers = Schedule, Tick, Timers
    subscribe, unsubscribe, topics, publish = Subscribe, Unsubscribe, Topics, Publish

    @property
    def conns_updated(self) -> IntChannel:
        return self._c.conns_updated

    def selected_nodes(self):
        return self._c.selected_nodes()

    @property
    def cfg(self) -> ConnConfig:
        return self._c.cfg


def new_client(host: str, serviceName: str, nodes: NodesChannel, cfg: ConnConfig | None = None) -> Client:
    """newClient(host, serviceName, registry, cfg) taking the WatchService channel."""
    return Client(_core.RpcClient(host, serviceName, nodes, cfg if cfg is not None else DefaultConnConfig()),
                  service=serviceName)


# ---------------------------------------------------------------- server side
def _exported_methods(receiver) -> list[tuple[str, Callable]]:
    out = []
    for name, fn in inspect.getmembers(receiver, predicate=callable):
        if name[:1].isupper() and not name.startswith("_"):
            out.append((name, fn))
    return out


class Server:
    """net/rpc-compatible server (HTTP CONNECT + gob) for host and GPU actors.

    ``Register(receiver)`` mirrors ``rpc.Register``: every exported (capitalised)
    method of the receiver becomes ``"<TypeName>.<Method>"``; a method takes the
    decoded args and returns the reply, raising to return an RPC error.
    ``RegisterDevice`` binds a method to a compiled-in GPU handler through the
    persistent dispatcher.
    """

    def __init__(self):
        self._s = RpcServer()

    def Register(self, receiver, name: str | None = None) -> None:
        tname = name or type(receiver).__name__
        methods = _exported_methods(receiver)
        if not methods:
            raise ValueError(f"rpc.Register: type {tname} has no exported methods of suitable type")
        for mname, fn in methods:
            self._s.register_method(f"{tname}.{mname}", fn)

    def RegisterFunc(self, service_method: str, fn: Callable) -> None:
        self._s.register_method(service_method, fn)

    def RegisterDevice(self, service_method: str, device_server, method_id: int, fields: Iterable[str] = (),
                       actor: int = 0, actor_field: str = "") -> None:
        fn, ctx = device_server.submit_handle()
        self._s.register_device_method(service_method, fn, ctx, int(method_id), int(actor), list(fields), actor_field)
        if getattr(device_server, "shm_name", ""):  # same-node processes call it through shared memory
            device_server.export_method(service_method, int(method_id), int(actor), list(fields), actor_field)
            self._s.set_shm_segment(device_server.shm_name)

    def RegisterDeviceBatch(self, service_method: str, batch_handle, fields: Iterable[str] = (), actor_field: str = "",
                            max_batch: int = 1 << 16) -> None:
        """Serve ``service_method`` (registered for single calls first) in
        batches: the pipelined requests a connection has buffered are decoded
        together -- on the GPU with ``batch_handle = DeviceRuntime.gob_bridge(...).handle()``
        (K4, csrc/hip/gob_bridge.hpp), or on the host with ``_core.host_batch_multiply()``."""
        fn, ctx = batch_handle
        self._s.register_device_batch(service_method, fn, ctx, list(fields), actor_field, int(max_batch))

    @property
    def batches(self) -> int:
        return self._s.batches

    @property
    def batched_calls(self) -> int:
        return self._s.batched_calls

    def Listen(self, port: int = 0, host: str = "0.0.0.0", local: bool = True) -> int:
        return self._s.listen(host, int(port), local)

    def Close(self) -> None:
        self._s.close()

    def Dispatch(self, service_method: str, args: Any) -> Any:
        return self._s.dispatch(service_method, args)

    @property
    def port(self) -> int:
        return self._s.port

    def call_counts(self) -> dict:
        return self._s.call_counts()

    def debug_page(self) -> str:
        return self._s.debug_page()

    def ServeDebug(self, stats: Callable[[], dict], path: str = "/debug/ptype") -> None:
        """``GET <path>`` on this server's port answers ``json.dumps(stats())``
        (next to net/rpc's ``/debug/rpc``); e.g. ``server.ServeDebug(cluster.Stats)``."""
        import json

        self._s.set_debug_handler(path, lambda: json.dumps(stats(), default=str))

    register, register_func, register_device, listen, close = Register, RegisterFunc, RegisterDevice, Listen, Close
    serve_debug = ServeDebug


def Serve(port: int, *receivers, host: str = "0.0.0.0") -> Server:
    """rpc.Register(each receiver) + rpc.HandleHTTP + ListenAndServe(":port")
    (example/calculator/server/server.go:16-20, :38), non-blocking."""
    s = Server()
    for r in receivers:
        s.Register(r)
    s.Listen(port, host)
    return s


# ---------------------------------------------------------------- cluster
class Cluster:
    """Handle returned by ``Join`` (cluster/cluster.go:20-26)."""

    def __init__(self, core: _core.Cluster, cfg: Config, runtime=None):
        self._c = core
        self.cfg = cfg
        self.Registry = Registry(core.registry)
        self.Store = KVStore(core.store)
        self.runtime = runtime
        self._clients: list[Client] = []

    def MemberList(self, ctx=None):
        return self._c.member_list(_ctx(ctx))

    def NewClient(self, serviceName: str, cfg: ConnConfig | None = None) -> Client:
        mc = cfg.max_connections if cfg is not None else _core.default_conn_config().max_connections
        c = Client(self._c.new_client(serviceName, cfg), self.runtime, serviceName, self.local_addr, mc)
        self._clients.append(c)
        return c

    def Stats(self) -> dict:
        """Observability snapshot: control-plane member status, the
        clients' call/attempt counters and selected nodes, and -- with a GPU
        runtime -- dispatcher, registry-mirror and exchange counters plus the
        single-call round-trip histogram.  Served as JSON by ``Server.ServeDebug``."""
        st = self._c.member_status()
        out = {
            "service": self.cfg.service_name, "node": self.cfg.node_name, "local_addr": self.local_addr,
            "member": {"id": st.id, "leader": st.leader, "term": st.term, "commit": st.commit,
                       "applied": st.applied, "revision": st.revision, "is_learner": st.is_learner},
            "clients": [{"service": c.service, "calls": c._c.calls, "attempts": c._c.attempts,
                         "nodes": [f"{n.address}:{n.port}" for n in c.selected_nodes()]} for c in self._clients],
        }
        if self.runtime is not None:
            out["runtime"] = self.runtime.stats()
        return out

    def Close(self) -> None:
        if self.runtime is not None:
            self.runtime.close()
        self._c.close()

    @property
    def local_addr(self) -> str:
        return self._c.local_addr

    @property
    def member_id(self) -> int:
        return self._c.member_id

    def status(self):
        return self._c.member_status()

    registry = property(lambda self: self.Registry)
    store = property(lambda self: self.Store)
    member_list, new_client, close, stats = MemberList, NewClient, Close, Stats

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Close()


def Join(ctx, cfg: Config, runtime: bool | None = None) -> Cluster:
    """Join the cluster: start the local control-plane member (as a learner via
    ``initial_cluster_client_urls`` when ``initial-cluster-state: existing``,
    promoted once caught up), then register ``services/<service>/<node>/`` with
    a 2 s lease.  With a ``gpu:`` section (or ``runtime=True``) the process also
    brings up its GPU actor runtime (persistent dispatcher, registry mirror)."""
    core = _core.Cluster.join(_ctx(ctx), cfg)
    rt = None
    want = cfg.has_gpu if runtime is None else runtime
    if want:
        from .runtime import DeviceRuntime

        try:
            if cfg.gpu.tune:  # the config's path switches (ops/tune.py, csrc/hip/tune.hpp)
                from .ops import tune

                tune.set(cfg.gpu.tune)
            rt = DeviceRuntime.for_cluster(core, cfg)
        except Exception:
            core.close()
            raise
    return Cluster(core, cfg, rt)


def New(cfg: Config, ctx=None, runtime: bool | None = None) -> Cluster:
    """North-star entry point: ``cluster.New(cfg)`` == ``Join(ctx, cfg)``."""
    return Join(ctx, cfg, runtime)


join = Join
new = New


def member_config(**kw) -> MemberConfig:
    """Programmatic member config (the reference's tests set the unexported
    etcdConfig fields directly, cluster/cluster_test.go:73-87)."""
    m = MemberConfig()
    for k, v in kw.items():
        if not hasattr(m, k):
            raise AttributeError(f"MemberConfig has no field {k}")
        setattr(m, k, v)
    return m
