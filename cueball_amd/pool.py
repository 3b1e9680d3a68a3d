"""ConnectionPool: claim/release pooling over resolver-discovered backends.

Re-design of reference lib/pool.js.  The pool owns one ConnectionSlotFSM
per connection, keeps idle/init/waiter queues (intrusive, O(1) unlink),
and continuously rebalances towards `spares` idle connections spread
evenly over the live backends, clamped by an EMA low-pass filter so the
pool does not shrink against recent load transients
(lib/pool.js:37-100), rate-limited by `maxChurnRate`, and periodically
"decoherence-shuffled" so that many clients don't converge on the same
backend ordering (lib/pool.js:501-519, docs/internals.adoc:276-386).

States: starting -> running <-> failed ; stopping -> stopping.backends
-> stopped (lib/pool.js:315-487).
"""

from __future__ import annotations

import functools
import math
import os as _os
import random
import time as mod_time
import uuid as mod_uuid
from typing import Any, Callable, Dict, List, Mapping, Optional

from . import affinity as mod_affinity
from . import balance as mod_balance
from . import codel as mod_codel
from . import errors as mod_errors
from . import latency as mod_latency
from . import limit as mod_limit
from . import utils as mod_utils
from .connection_fsm import ClaimHandle, ConnectionSlotFSM
from .events import EventEmitter
from .fsm import FSM, StateScope, get_loop
from .logutil import CueballLogger, default_logger
from .pool_monitor import monitor as global_monitor
from .queue import Queue

__all__ = ["ConnectionPool", "FIRFilter", "gen_taps"]

# EMA/low-pass filter parameters (lib/pool.js:37-62): 5 Hz sampling,
# 128-tap EMA with time constant -0.2 => pass band ~0.25 Hz.
LP_RATE = 5
LP_INT_MS = round(1000.0 / LP_RATE)


def gen_taps(count: int, tc: float) -> List[float]:
    taps = [math.exp(tc * i) for i in range(count)]
    s = sum(taps)
    return [t / s for t in taps]


LP_TAPS = gen_taps(128, -0.2)


class FIRFilter:
    """Simple FIR filter over a circular buffer (lib/pool.js:77-100)."""

    __slots__ = ("f_taps", "f_buf", "f_ptr")

    def __init__(self, taps: List[float]) -> None:
        self.f_taps = taps
        self.f_buf = [0.0] * len(taps)
        self.f_ptr = 0

    def put(self, v: float) -> None:
        self.f_buf[self.f_ptr] = v
        self.f_ptr += 1
        if self.f_ptr == len(self.f_taps):
            self.f_ptr = 0

    def get(self) -> float:
        i = self.f_ptr - 1
        n = len(self.f_taps)
        if i < 0:
            i += n
        acc = 0.0
        buf = self.f_buf
        for tap in self.f_taps:
            acc += buf[i] * tap
            i -= 1
            if i < 0:
                i += n
        return acc


class _ClaimTicket:
    """Per-claim driver: retries the claim whenever the handle returns
    to 'waiting' (registered as the handle's stateChanged listener; the
    closure-free form of lib/pool.js:922-968, on the claim hot path).

    When the native core is loaded, its own ticket replaces this class
    on the claim path: a hook of the native handle, not a registered
    listener, that performs the idle-queue handoff entirely in C and
    delegates everything else to the same ``pool._ticket_slow`` this
    class uses (``_speed.ClaimTicket`` is that code as a listener)."""

    __slots__ = ("pool", "handle", "err_on_empty")

    #: lets the handle's terminal cleanup unregister us (see
    #: ClaimHandle._fsm_terminal_settled)
    _cueball_ticket = True

    def __init__(self, pool: "ConnectionPool", handle: ClaimHandle,
                 err_on_empty: bool) -> None:
        self.pool = pool
        self.handle = handle
        self.err_on_empty = err_on_empty

    def __call__(self, st: str) -> None:
        if st == "waiting":
            self.pool._ticket_slow(self.handle, self.err_on_empty)


class _AvoidClaimTicket:
    """The ticket of a claim that carries ``avoidBackends``: always the
    Python slow path, with the set handed along, on either runtime.  It
    unregisters itself when the handle settles (the native handle's
    terminal cleanup knows only its own ticket type)."""

    __slots__ = ("pool", "handle", "err_on_empty", "avoid")

    _cueball_ticket = True

    def __init__(self, pool: "ConnectionPool", handle: ClaimHandle,
                 err_on_empty: bool, avoid: frozenset) -> None:
        self.pool = pool
        self.handle = handle
        self.err_on_empty = err_on_empty
        self.avoid = avoid

    def __call__(self, st: str) -> None:
        handle = self.handle
        if handle is None:
            return
        if st == "waiting":
            self.pool._ticket_slow(handle, self.err_on_empty, self.avoid)
        elif st in ("released", "closed", "cancelled", "failed"):
            self.handle = None
            handle.remove_listener("stateChanged", self)


class _BalancedClaimTicket:
    """The ticket of every claim on a pool with ``claimBalancing``: the
    Python path once more, on either runtime, with the balancer choosing
    among the idle slots (``pool._ticket_balanced``).  The handle and the
    slot's busy/idle cycle stay what they are."""

    __slots__ = ("pool", "handle", "err_on_empty", "avoid")

    _cueball_ticket = True

    def __init__(self, pool: "ConnectionPool", handle: ClaimHandle,
                 err_on_empty: bool, avoid: Optional[frozenset]) -> None:
        self.pool = pool
        self.handle = handle
        self.err_on_empty = err_on_empty
        self.avoid = avoid

    def __call__(self, st: str) -> None:
        handle = self.handle
        if handle is None:
            return
        if st == "waiting":
            self.pool._ticket_balanced(handle, self.err_on_empty,
                                       self.avoid)
        elif st in ("released", "closed", "cancelled", "failed"):
            self.handle = None
            handle.remove_listener("stateChanged", self)


class _AffinityClaimTicket:
    """The ticket of a claim that carries ``affinityKey``, on a pool with
    ``claimAffinity``: the Python path, on either runtime, with the key's
    rendezvous order choosing among the idle slots
    (``pool._ticket_affine``).  ``counted`` is set once the claim's
    outcome has been counted: a claim is counted once, however often it
    returns to 'waiting'."""

    __slots__ = ("pool", "handle", "err_on_empty", "avoid", "key",
                 "counted")

    _cueball_ticket = True

    def __init__(self, pool: "ConnectionPool", handle: ClaimHandle,
                 err_on_empty: bool, avoid: Optional[frozenset],
                 key: bytes) -> None:
        self.pool = pool
        self.handle = handle
        self.err_on_empty = err_on_empty
        self.avoid = avoid
        self.key = key
        self.counted = False

    def __call__(self, st: str) -> None:
        handle = self.handle
        if handle is None:
            return
        if st == "waiting":
            self.pool._ticket_affine(handle, self)
        elif st in ("released", "closed", "cancelled", "failed"):
            self.handle = None
            handle.remove_listener("stateChanged", self)


#: what _ticket_slow sees in place of the idle queue while the pool's
#: concurrency limit holds claims back
_NO_IDLE = Queue()

_NativeClaimTicket = None
_native_claim_fast = None
_native_pool_claim = None
_NativeSlotDispatch = None
if not _os.environ.get("CUEBALL_PURE"):
    try:
        from ._speed import ClaimTicket as _NativeClaimTicket  # noqa: F811
        from ._speed import claim_fast as _native_claim_fast
        from ._speed import pool_claim as _native_pool_claim
        from ._speed import SlotDispatch as _NativeSlotDispatch
    except ImportError:
        pass


class _CancelStub:
    """claim() return value when the pool is stopping/failed: supports
    only .cancel() (lib/pool.js:895-897)."""

    __slots__ = ("_state",)

    def __init__(self, state):
        self._state = state

    def cancel(self) -> None:
        self._state["done"] = True


class _IntervalTimer(EventEmitter):
    """An EventEmitter that fires 'timeout' every `ms` (the pool's FSM
    states subscribe/unsubscribe to these with their state scope, like
    the reference's unref()'d setInterval wrappers, lib/pool.js:228-263).
    """

    def __init__(self, loop, ms: float) -> None:
        super().__init__()
        self._loop = loop
        self._ms = ms
        self._handle = None
        self._stopped = False
        self._schedule()

    def _schedule(self) -> None:
        self._handle = self._loop.call_later(self._ms / 1000.0, self._fire)

    def _fire(self) -> None:
        if self._stopped:
            return
        self._schedule()
        self.emit("timeout")

    def cancel(self) -> None:
        self._stopped = True
        if self._handle is not None:
            self._handle.cancel()


class ConnectionPool(FSM):
    # SRV ranking state.  Class-level defaults, so that a pool without
    # srvRanking carries no extra instance attribute: native code looks
    # attributes up in the instance dict on every claim, and that dict
    # stays exactly what it was.
    p_ranks: Optional[Dict[str, tuple]] = None
    p_rank_gen = 0
    p_active_priority: Optional[int] = None
    _prio_gauge = None

    # Connection age / recycle() state, class-level for the same
    # reason: a pool without maxConnectionAge that never called
    # recycle() has none of these in its instance dict.
    p_age_max: Optional[float] = None      # maxConnectionAge, ms
    p_age_spread: Optional[float] = None
    #: slot -> [deadline (loop seconds), reason] for connected sockets
    #: that have a deadline; None until the feature is in use
    p_age_slots: Optional[Dict[Any, list]] = None
    #: slot -> reason for slots retired or marked, until they stop
    p_age_retiring: Optional[Dict[Any, str]] = None
    #: retired slots that stopped whose replacement is not planned yet
    p_age_settling = 0
    p_age_timer = None
    p_age_timer_at: Optional[float] = None
    _age_gauge = None

    # Outlier detection / eject_backend() state, class-level once more:
    # a pool without outlierDetection that never called eject_backend()
    # has none of these in its instance dict.
    #: the validated outlierDetection option, defaults filled in
    p_od: Optional[Dict[str, Any]] = None
    #: key -> per-backend record (see _od_record); None until in use
    p_od_backends: Optional[Dict[str, Dict[str, Any]]] = None
    #: key -> ejection entry {"reason", "at", "until", "durationMs",
    #: "timer"} for the backends that are ejected right now
    p_od_ejected: Optional[Dict[str, Dict[str, Any]]] = None
    #: slot -> claim handle of the lease seen to begin on it
    p_od_open: Optional[Dict[Any, Any]] = None
    #: slot -> last handle attributed to it (a handle has one lease)
    p_od_last: Optional[Dict[Any, Any]] = None
    #: slot -> "error" | "closed": how its current socket ended
    p_od_sock: Optional[Dict[Any, str]] = None
    _od_gauge = None

    # Claim balancing state, class-level like the rest: a pool without
    # claimBalancing has none of these in its instance dict, and its
    # claim() is the class's.
    #: the validated claimBalancing option, defaults filled in
    p_lb: Optional[Dict[str, Any]] = None
    #: key -> balance.BackendLoad; dropped when the resolver removes it
    p_lb_backends: Optional[Dict[str, Any]] = None
    #: slot -> (handle, load) of a slot the ticket handed over, until
    #: the slot's 'busy' is heard
    p_lb_handed: Optional[Dict[Any, tuple]] = None
    #: slot -> (handle, load, start in loop seconds) of the lease seen
    #: to begin on it
    p_lb_open: Optional[Dict[Any, tuple]] = None
    #: slot -> last handle attributed to it (a handle has one lease)
    p_lb_last: Optional[Dict[Any, Any]] = None
    _lb_gauges: Optional[tuple] = None

    # Claim queue state, class-level like the rest: a pool without
    # claimQueue has none of these in its instance dict, and its
    # claim() is the class's.
    #: the validated claimQueue option, defaults filled in
    p_cq: Optional[Dict[str, Any]] = None
    #: per class, the node of its last waiter as far as the pool knows
    #: (it may have left the queue since); None with a single class
    p_cq_last: Optional[List[Any]] = None
    #: when the waiter queue last went from empty to non-empty, loop ms
    p_cq_since = 0.0
    _cq_gauge = None

    # Key affinity state, class-level like the rest: a pool without
    # claimAffinity has none of these in its instance dict, and its
    # claim() is the class's.
    #: the validated claimAffinity option, defaults filled in
    p_af: Optional[Dict[str, Any]] = None
    #: key -> affinity.backend_hash(key), for the backends the resolver
    #: lists: set when one is added, dropped when it is removed
    p_af_hashes: Optional[Dict[str, int]] = None
    #: (backend keys sorted, their hashes in that order), what
    #: affinity.rank reads; None after the resolver changed the set
    p_af_ranked: Optional[tuple] = None
    #: key -> [keyed claims that had it as first choice, keyed claims
    #: placed on it]
    p_af_placed: Optional[Dict[str, List[int]]] = None
    _af_gauge = None

    # Concurrency limit state, class-level like the rest: a pool without
    # concurrencyLimit has none of these in its instance dict, its
    # claim() is the class's and its slots keep the native dispatcher.
    #: the validated concurrencyLimit option, defaults filled in
    p_cl: Optional[Dict[str, Any]] = None
    #: the limit.ConcurrencyLimiter
    p_cl_lim: Any = None
    #: leases in flight, and limiter.allowed() as last published
    p_cl_inflight = 0
    p_cl_allowed = 0
    #: floor(limit) as the last rebalance was asked to size for
    p_cl_floor = 0
    #: slot -> (handle, limiter token) of a slot handed to a claim,
    #: until the slot's 'busy' is heard
    p_cl_handed: Optional[Dict[Any, tuple]] = None
    #: slot -> (handle, token) of the lease seen to begin on it
    p_cl_open: Optional[Dict[Any, tuple]] = None
    #: slot -> last handle attributed to it (a handle has one lease)
    p_cl_last: Optional[Dict[Any, Any]] = None
    _cl_gauges: Optional[tuple] = None

    def __init__(self, options: Dict[str, Any]) -> None:
        if not callable(options.get("constructor")):
            raise TypeError("options.constructor (callable) is required")

        loop_opt = options.get("loop")
        self.p_uuid = str(mod_uuid.uuid4())
        self.p_constructor = options["constructor"]

        if not isinstance(options.get("domain"), str):
            raise TypeError("options.domain (string) is required")
        self.p_domain = options["domain"]
        mod_utils.assert_claim_delay(options.get("targetClaimDelay"))

        recovery = options.get("recovery")
        mod_utils.assert_recovery_set(recovery)
        self.p_recovery = recovery

        log: CueballLogger = options.get("log") or default_logger()
        self.p_log = log.child(
            component="ConnectionPool",
            domain=options.get("domain"),
            service=options.get("service"),
            pool=self.p_uuid,
        )
        # shared child logger for claim handles (hot path)
        self.p_claim_log = self.p_log.child(component="ClaimHandle")

        self.p_collector = mod_utils.create_error_metrics(options)
        try:
            self._gauge = self.p_collector.gauge(
                name="cueball_pool_connections",
                help="Live connection counts per pool and state")
            self._gauge_labels = {"pool": self.p_uuid.split("-")[0],
                                  "domain": options["domain"]}
        except (AttributeError, ValueError):
            self._gauge = None  # foreign collector without gauges
            self._gauge_labels = {}

        spares = options.get("spares")
        maximum = options.get("maximum")
        if not isinstance(spares, int) or not isinstance(maximum, int):
            raise TypeError("options.spares and options.maximum are required")
        self.p_spares = spares
        self.p_max = maximum

        self.p_checker = options.get("checker")
        self.p_check_timeout = options.get("checkTimeout")

        self.p_keys: List[str] = []
        self.p_backends: Dict[str, Dict[str, Any]] = {}
        self.p_connections: Dict[str, List[ConnectionSlotFSM]] = {}
        self.p_dead: Dict[str, bool] = {}
        self.p_lastrate: Dict[str, Dict[str, float]] = {}

        max_churn = options.get("maxChurnRate")
        self.p_maxrate = float(max_churn) if max_churn is not None else math.inf

        self.p_last_rebalance: Optional[float] = None
        self.p_in_rebalance = False
        self.p_rebal_scheduled = False
        self.p_started_resolver = False
        self.p_lpf = FIRFilter(LP_TAPS)
        self.p_last_rebal_clamped = False
        self.p_rate_delay_timer = None
        # Census signature of the last no-op rebalance: plan_rebalance
        # is a pure function of (key order, per-key counts, dead set,
        # target, max), so if none of those changed since a rebalance
        # that planned nothing, the plan is empty again and we can skip
        # building it.  Claim-heavy steady state schedules a rebalance
        # every loop turn (each idle->busy claim does), making this the
        # hot no-op path.
        self.p_noop_census: Optional[tuple] = None
        # Peak demand (busy + extras) and peak busy seen since the last
        # rebalance / LPF sample.  The reference sizes from an
        # instantaneous sample taken when its setImmediate/timer fires
        # (lib/pool.js:560-588, :251-263); with this runtime's batched
        # event dispatch those callbacks tend to run at quiescent
        # points between claim bursts, where busy == waiters == 0, so
        # an instantaneous sample would chronically under-size the
        # pool.  Tracking the high-water mark on the claim path sizes
        # for the peak concurrent demand of the interval instead,
        # which is the reference's intent.
        self.p_demand_hwm = 0
        self.p_busy_hwm = 0
        self.p_total_conns = 0

        self.p_idleq = Queue()
        self.p_initq = Queue()
        self.p_waiters = Queue()

        self.p_codel: Optional[mod_codel.ControlledDelay] = None
        tcd = options.get("targetClaimDelay")
        if tcd is not None and math.isfinite(tcd):
            self.p_codel = mod_codel.ControlledDelay(tcd, loop=loop_opt)

        # Latency histograms (claim wait, claim hold, connect).  The
        # claim handle records into p_lat directly from its state
        # entries; the collector only ever sees a snapshot, published
        # from _lp_tick.
        latency_stats = options.get("latencyStats")
        if latency_stats is None:
            latency_stats = True
        if not isinstance(latency_stats, bool):
            raise TypeError("options.latencyStats must be a bool")
        self.p_lat = None
        self._lat_metrics: List[tuple] = []
        if latency_stats:
            self.p_lat = mod_latency.PoolLatency(get_loop(loop_opt))
            self._register_latency_metrics()

        self.p_last_error: Optional[BaseException] = None
        self.p_counters: Dict[str, int] = {}

        # SRV ranking (opt-in): key -> (priority, weight), handed to the
        # rebalance planner; None when off.  p_rank_gen counts rank
        # edits for the no-op census.
        srv_ranking = options.get("srvRanking")
        if srv_ranking is None:
            srv_ranking = False
        if not isinstance(srv_ranking, bool):
            raise TypeError("options.srvRanking must be a bool")
        if srv_ranking:
            self.p_ranks = {}
        if srv_ranking and self._gauge is not None:
            try:
                self._prio_gauge = self.p_collector.gauge(
                    name="cueball_pool_active_priority",
                    help="SRV priority tier the pool is currently using")
            except (AttributeError, ValueError):
                pass

        # Connection age (opt-in): see the "connection age" section
        # below.  Off means not one attribute is set here.
        age, spread = mod_utils.assert_connection_age(options)
        if age is not None:
            self.p_age_max = age
            self.p_age_spread = spread
            self.p_age_slots = {}
            self.p_age_retiring = {}
            if self._gauge is not None:
                try:
                    self._age_gauge = self.p_collector.gauge(
                        name="cueball_pool_oldest_connection_seconds",
                        help="Age of the pool's oldest connected socket")
                except (AttributeError, ValueError):
                    pass

        # Outlier detection (opt-in): see the "outlier ejection"
        # section below.  Off means not one attribute is set here.
        od = mod_utils.assert_outlier_detection(options)
        if od is not None:
            self.p_od = od
            self._od_init()
            self.p_od_open = {}
            self.p_od_last = {}
            self.p_od_sock = {}
            if self._gauge is not None:
                try:
                    self._od_gauge = self.p_collector.gauge(
                        name="cueball_pool_ejected_backends",
                        help="Backends the pool has ejected as outliers")
                except (AttributeError, ValueError):
                    pass

        # Claim balancing (opt-in): see the "claim balancing" section
        # below.  Off means not one attribute is set here; on, claim()
        # itself is replaced on this instance alone.
        lb = mod_utils.assert_claim_balancing(options)
        if lb is not None:
            self.p_lb = lb
            self.p_lb_backends = {}
            self.p_lb_handed = {}
            self.p_lb_open = {}
            self.p_lb_last = {}
            self.claim = self._claim_balanced
            if self._gauge is not None:
                try:
                    self._lb_gauges = (
                        self.p_collector.gauge(
                            name="cueball_pool_backend_latency_seconds",
                            help="Lease latency estimate per backend, as "
                                 "claim balancing sees it"),
                        self.p_collector.gauge(
                            name="cueball_pool_backend_outstanding",
                            help="Connections per backend handed to a "
                                 "claim or serving a lease"))
                except (AttributeError, ValueError):
                    pass

        # Claim queue (opt-in): see the "claim queue" section below.
        # Off means not one attribute is set here; on, claim() is
        # replaced on this instance alone, claimBalancing or not.
        cq = mod_utils.assert_claim_queue(options)
        if cq is not None:
            self.p_cq = cq
            if cq["priorities"] > 1:
                self.p_cq_last = [None] * cq["priorities"]
            self.p_cq_since = 0.0
            self.claim = self._claim_queued
            if self._gauge is not None:
                try:
                    self._cq_gauge = self.p_collector.gauge(
                        name="cueball_pool_queued_claims",
                        help="Claims waiting in the pool's queue, by "
                             "priority class")
                except (AttributeError, ValueError):
                    pass

        # Key affinity (opt-in): see the "key affinity" section below.
        # Off means not one attribute is set here.  On, claim() is
        # replaced on this instance alone, unless claimBalancing or
        # claimQueue has done so: their claim()s know about keys.
        af = mod_utils.assert_claim_affinity(options)
        if af is not None:
            self.p_af = af
            self.p_af_hashes = {}
            self.p_af_placed = {}
            if lb is None and cq is None:
                self.claim = self._claim_affine
            if self._gauge is not None:
                try:
                    self._af_gauge = self.p_collector.gauge(
                        name="cueball_pool_affinity_hit_ratio",
                        help="Share of the claims with an affinityKey "
                             "that got the key's first choice")
                except (AttributeError, ValueError):
                    pass

        # Concurrency limit (opt-in): see the "concurrency limit"
        # section below.  Off means not one attribute is set here.  On,
        # claim() is replaced on this instance alone, unless one of the
        # three options above has done so: their tickets know the gate.
        cl = mod_utils.assert_concurrency_limit(options)
        if cl is not None:
            self.p_cl = cl
            self.p_cl_lim = mod_limit.ConcurrencyLimiter(cl)
            self.p_cl_inflight = 0
            self.p_cl_allowed = self.p_cl_lim.allowed()
            self.p_cl_floor = int(math.floor(self.p_cl_lim.limit))
            self.p_cl_handed = {}
            self.p_cl_open = {}
            self.p_cl_last = {}
            if lb is None and cq is None and af is None:
                self.claim = self._claim_limited
            if self._gauge is not None:
                try:
                    self._cl_gauges = (
                        self.p_collector.gauge(
                            name="cueball_pool_concurrency_limit",
                            help="Leases the pool may have in flight, as "
                                 "its concurrency limit stands"),
                        self.p_collector.gauge(
                            name="cueball_pool_in_flight",
                            help="Leases the pool has in flight, as its "
                                 "concurrency limit counts them"))
                except (AttributeError, ValueError):
                    pass

        if options.get("resolver") is not None:
            self.p_resolver = options["resolver"]
            self.p_resolver_custom = True
        else:
            from . import resolver as mod_resolver
            self.p_resolver = mod_resolver.Resolver({
                "resolvers": options.get("resolvers"),
                "domain": options["domain"],
                "service": options.get("service"),
                "maxDNSConcurrency": options.get("maxDNSConcurrency"),
                "defaultPort": options.get("defaultPort"),
                "log": self.p_log,
                "recovery": recovery,
                "loop": loop_opt,
                "srvRanking": srv_ranking,
            })
            self.p_resolver_custom = False

        super().__init__("starting", loop=loop_opt)

        # Periodic timers.  Created after FSM init so self._loop exists;
        # states subscribe to them scoped (lib/pool.js:228-263).
        self.p_rebal_timer = _IntervalTimer(self._loop, 10_000)
        shuffle_intvl = options.get("decoherenceInterval")
        if shuffle_intvl is None or shuffle_intvl < 60:
            shuffle_intvl = 60
        self.p_shuffle_timer = _IntervalTimer(self._loop, shuffle_intvl * 1000)
        self.p_lp_timer = _IntervalTimer(self._loop, LP_INT_MS)
        self.p_lp_timer.on("timeout", self._lp_tick)

    # -- counters -------------------------------------------------------
    def _incr_counter(self, counter: str) -> None:
        # only tracked error events reach the metrics collector; the
        # hot counters (claim, queued-claim) skip the call entirely
        if counter in mod_utils.TRACKED_ERROR_EVENTS:
            mod_utils.update_error_metrics(self.p_collector, self.p_uuid,
                                           counter)
        self.p_counters[counter] = self.p_counters.get(counter, 0) + 1

    def _hwm_counter(self, counter: str, val: int) -> None:
        if self.p_counters.get(counter, -1) < val:
            self.p_counters[counter] = val

    def _note_demand(self) -> None:
        """O(1) demand sample on the claim path: fold the current
        busy/extras into the high-water marks consumed by _rebalance
        and _lp_tick (see p_demand_hwm comment in __init__)."""
        nw = self.p_waiters._len
        ni = self.p_initq._len
        spares = self.p_idleq._len + ni - nw
        if spares < 0:
            spares = 0
        busy = self.p_total_conns - spares
        if busy < 0:
            busy = 0
        extras = nw - ni
        if extras < 0:
            extras = 0
        if busy > self.p_busy_hwm:
            self.p_busy_hwm = busy
        if busy + extras > self.p_demand_hwm:
            self.p_demand_hwm = busy + extras

    # -- latency histograms -----------------------------------------------
    _LAT_METRICS = (
        ("wait", "cueball_claim_wait_seconds",
         "Time from claim() to the claim callback, served claims only"),
        ("hold", "cueball_claim_hold_seconds",
         "Time a claimed connection was held before release/close"),
        ("connect", "cueball_connect_seconds",
         "Time from starting a connect to the connect event"),
    )

    def _register_latency_metrics(self) -> None:
        """One Prometheus histogram per pool histogram, with the same
        labels as cueball_pool_connections.  The ``le`` bounds are
        4**k us (k = 2..13) in seconds; each is an internal bucket
        boundary, so the published counts are exact.  Half-open
        convention: an observation counts under ``le=L`` when its
        value, rounded to whole microseconds, is < L."""
        bounds = [us / 1e6 for us in mod_latency.EXPOSITION_BOUNDS_US]
        try:
            for attr, name, help_ in self._LAT_METRICS:
                m = self.p_collector.histogram(name=name, help=help_,
                                               buckets=bounds)
                self._lat_metrics.append((getattr(self.p_lat, attr), m))
        except (AttributeError, ValueError, TypeError):
            # foreign collector without (compatible) histograms
            self._lat_metrics = []

    def _publish_latency(self) -> None:
        labels = self._gauge_labels or {
            "pool": self.p_uuid.split("-")[0], "domain": self.p_domain}
        for hist, metric in self._lat_metrics:
            metric.set_cumulative(
                hist.cumulative(mod_latency.EXPOSITION_BOUNDS_US),
                hist.sum_us / 1e6, hist.count, labels)

    def get_latency_stats(self) -> Optional[Dict[str, Any]]:
        """Snapshots of the pool's latency histograms, times in ms:
        ``{"claimWait": snap, "claimHold": snap, "connect": snap}`` with
        ``snap = {"count", "sumMs", "minMs", "maxMs", "p50", "p90",
        "p99", "p999"}``; None when the pool was created with
        ``latencyStats: False``."""
        lat = self.p_lat
        if lat is None:
            return None
        return {"claimWait": lat.wait.snapshot(),
                "claimHold": lat.hold.snapshot(),
                "connect": lat.connect.snapshot()}

    # -- LPF anti-shrink sampling (lib/pool.js:251-263) ------------------
    def _lp_tick(self) -> None:
        conns = sum(len(v) for v in self.p_connections.values())
        spares = len(self.p_idleq) + len(self.p_initq)
        busy = conns - spares
        if busy < self.p_busy_hwm:
            busy = self.p_busy_hwm
        self.p_busy_hwm = conns - spares if conns > spares else 0
        self.p_lpf.put(busy + self.p_spares)
        # piggyback live gauges on the 5 Hz sample (beyond the
        # reference, which exposes state through kang only)
        g = self._gauge
        if g is not None:
            labels = self._gauge_labels
            g.set(conns, {**labels, "state": "total"})
            g.set(len(self.p_idleq), {**labels, "state": "idle"})
            g.set(len(self.p_initq), {**labels, "state": "pending"})
            g.set(len(self.p_waiters), {**labels, "state": "waiting"})
        if self._lat_metrics:
            self._publish_latency()
        if self._prio_gauge is not None and \
                self.p_active_priority is not None:
            self._prio_gauge.set(self.p_active_priority, self._gauge_labels)
        if self._age_gauge is not None:
            oldest = self._age_oldest(self._loop.time())
            self._age_gauge.set(0.0 if oldest is None else oldest,
                                self._gauge_labels)
        if self._od_gauge is not None:
            self._od_gauge.set(len(self.p_od_ejected), self._gauge_labels)
        if self._lb_gauges is not None:
            self._lb_publish()
        if self._cq_gauge is not None:
            self._cq_publish()
        if self._af_gauge is not None:
            self._af_publish()
        if self._cl_gauges is not None:
            self._cl_gauges[0].set(self.p_cl_allowed, self._gauge_labels)
            self._cl_gauges[1].set(self.p_cl_inflight, self._gauge_labels)
        if self.p_last_rebal_clamped:
            self.rebalance()

    # -- resolver events ------------------------------------------------
    def _on_resolver_added(self, k: str, backend: Dict[str, Any]) -> None:
        backend["key"] = k
        idx = random.randrange(len(self.p_keys) + 1)
        self.p_keys.insert(idx, k)
        self.p_backends[k] = backend
        if self.p_ranks is not None:
            self.p_ranks[k] = (backend.get("priority", 0),
                               backend.get("weight", 0))
            self.p_rank_gen += 1
        if self.p_af_hashes is not None:
            self.p_af_hashes[k] = mod_affinity.backend_hash(k)
            self.p_af_ranked = None
        self.rebalance()

    def _on_resolver_changed(self, k: str, backend: Dict[str, Any]) -> None:
        """A known backend's SRV rank changed (srvRanking only): same
        key, so no connection is touched here; the rebalance moves the
        spread."""
        if k not in self.p_backends:
            return
        # update in place: live slots hold a reference to this dict
        self.p_backends[k].update(backend)
        self.p_backends[k]["key"] = k
        self.p_ranks[k] = (backend.get("priority", 0),
                           backend.get("weight", 0))
        self.p_rank_gen += 1
        self.rebalance()

    def _subscribe_resolver(self, S: StateScope) -> None:
        S.on(self.p_resolver, "added", self._on_resolver_added)
        S.on(self.p_resolver, "removed", self._on_resolver_removed)
        if self.p_ranks is not None:
            S.on(self.p_resolver, "changed", self._on_resolver_changed)

    def _on_resolver_removed(self, k: str) -> None:
        try:
            self.p_keys.remove(k)
        except ValueError:
            raise AssertionError("resolver key %s not found" % k)
        self.p_backends.pop(k, None)
        self.p_dead.pop(k, None)
        if self.p_ranks is not None:
            self.p_ranks.pop(k, None)
            self.p_rank_gen += 1
        if self.p_od_backends is not None:
            # gone is gone: no event, and a backend that comes back
            # under the same key starts clean
            self.p_od_backends.pop(k, None)
            ent = self.p_od_ejected.pop(k, None)
            if ent is not None:
                ent["timer"].cancel()
        if self.p_lb_backends is not None:
            # likewise; leases still open keep the record they began on
            self.p_lb_backends.pop(k, None)
        if self.p_af_hashes is not None:
            self.p_af_hashes.pop(k, None)
            self.p_af_placed.pop(k, None)
            self.p_af_ranked = None
        # Slots unlink themselves (and rebalance) from the stateChanged
        # handler in add_connection once they stop; here we only flag
        # them unwanted (lib/pool.js:300-313).
        for fsm in list(self.p_connections.get(k, ())):
            fsm.set_unwanted()
        if self.p_od_ejected:
            # the last backend that was not ejected may just have left
            self._od_panic_check()

    # -- states ----------------------------------------------------------
    def state_starting(self, S: StateScope) -> None:
        S.valid_transitions(["failed", "running", "stopping"])
        global_monitor.register_pool(self)

        self._subscribe_resolver(S)

        if self.p_resolver.is_in_state("failed"):
            self.p_log.warn('pre-provided resolver has already failed, '
                            'pool will start up in "failed" state')
            self.p_last_error = mod_errors.CueballError(
                'Pool resolver entered state "failed"',
                self.p_resolver.get_last_error())
            S.goto_state("failed")
            return

        def on_res_state(state: str) -> None:
            if state == "failed":
                self.p_log.warn('underlying resolver failed, moving pool '
                                'to "failed" state')
                self.p_last_error = mod_errors.CueballError(
                    'Pool resolver entered state "failed"',
                    self.p_resolver.get_last_error())
                S.goto_state("failed")

        S.on(self.p_resolver, "stateChanged", on_res_state)

        if self.p_resolver.is_in_state("running"):
            for k, backend in self.p_resolver.list().items():
                self._on_resolver_added(k, backend)
        elif self.p_resolver.is_in_state("stopped") and \
                not self.p_resolver_custom:
            self.p_resolver.start()
            self.p_started_resolver = True

        S.on(self, "connectedToBackend", lambda *a: S.goto_state("running"))

        def on_closed_backend(*a: Any) -> None:
            dead = len(self.p_dead)
            self._hwm_counter("max-dead-backends", dead)
            if dead >= len(self.p_keys):
                self.p_log.warn("pool has exhausted all retries, now moving "
                                'to "failed" state', dead=dead)
                S.goto_state("failed")

        S.on(self, "closedBackend", on_closed_backend)
        S.on(self, "stopAsserted", lambda: S.goto_state("stopping"))

    def state_failed(self, S: StateScope) -> None:
        S.valid_transitions(["running", "stopping"])
        self._subscribe_resolver(S)
        S.on(self.p_shuffle_timer, "timeout", self.reshuffle)

        def on_connected(*a: Any) -> None:
            if self.p_resolver.is_in_state("failed"):
                raise AssertionError("resolver failed while pool recovering")
            self.p_log.info("successfully connected to a backend, moving "
                            "back to running state")
            S.goto_state("running")

        S.on(self, "connectedToBackend", on_connected)
        S.on(self, "stopAsserted", lambda: S.goto_state("stopping"))

        self._incr_counter("failed-state")

        # Fail all outstanding claims that wait for a connection.
        while not self.p_waiters.is_empty():
            hdl = self.p_waiters.shift()
            if hdl.is_in_state("waiting"):
                hdl.fail(mod_errors.PoolFailedError(self, self.p_last_error))

    def state_running(self, S: StateScope) -> None:
        S.valid_transitions(["failed", "stopping"])
        self._subscribe_resolver(S)
        S.on(self.p_rebal_timer, "timeout", self.rebalance)
        S.on(self.p_shuffle_timer, "timeout", self.reshuffle)

        def on_closed_backend(*a: Any) -> None:
            dead = len(self.p_dead)
            self._hwm_counter("max-dead-backends", dead)
            if dead >= len(self.p_keys):
                self.p_log.warn("pool has exhausted all retries, now moving "
                                'to "failed" state', dead=dead)
                S.goto_state("failed")

        S.on(self, "closedBackend", on_closed_backend)
        S.on(self, "stopAsserted", lambda: S.goto_state("stopping"))
        if self.p_age_slots is not None:
            # deadlines that passed while the pool was not running
            self._loop.call_soon(self._age_run)

    def state_stopping(self, S: StateScope) -> None:
        S.valid_transitions(["stopping.backends"])
        if self.p_age_timer is not None:
            self.p_age_timer.cancel()
            self.p_age_timer = None
            self.p_age_timer_at = None
        if self.p_od_ejected:
            for ent in self.p_od_ejected.values():
                ent["timer"].cancel()
            self.p_od_ejected.clear()
        # Divergence from the reference (bug fix): fail queued waiters
        # with PoolStoppingError instead of leaving them pending forever
        # (the reference's state_stopping never touches p_waiters, so an
        # infinite-timeout claim outstanding at stop() hangs;
        # lib/pool.js:433-448 vs the failed-state drain at :398-405).
        while not self.p_waiters.is_empty():
            hdl = self.p_waiters.shift()
            if hdl.is_in_state("waiting"):
                hdl.fail(mod_errors.PoolStoppingError(self))
        if self.p_started_resolver:
            def on_res_state(s: str) -> None:
                if s == "stopped":
                    S.goto_state("stopping.backends")

            S.on(self.p_resolver, "stateChanged", on_res_state)
            self.p_resolver.stop()
            if self.p_resolver.is_in_state("stopped"):
                S.goto_state("stopping.backends")
        else:
            S.goto_state("stopping.backends")

    def state_stopping_backends(self, S: StateScope) -> None:
        S.valid_transitions(["stopped"])
        fsms: List[ConnectionSlotFSM] = []
        for conns in self.p_connections.values():
            fsms.extend(conns)

        remaining = {"n": len(fsms)}

        def one_done() -> None:
            remaining["n"] -= 1
            if remaining["n"] == 0:
                S.goto_state("stopped")

        if not fsms:
            S.goto_state("stopped")
            return

        for fsm in fsms:
            fsm.set_unwanted()
            if fsm.is_in_state("stopped") or fsm.is_in_state("failed"):
                one_done()
            else:
                def make_cb():
                    fired = {"done": False}

                    def cb(st: str) -> None:
                        if fired["done"]:
                            return
                        if st in ("stopped", "failed"):
                            fired["done"] = True
                            one_done()
                    return cb

                # Scoped: auto-removed from the slot FSM when the pool
                # leaves stopping.backends, so repeated stop cycles (or
                # slots that outlive the pool) cannot accumulate
                # listeners (round-1 review finding).
                S.on(fsm, "stateChanged", make_cb())

    def state_stopped(self, S: StateScope) -> None:
        S.valid_transitions([])
        global_monitor.unregister_pool(self)
        self.p_keys = []
        self.p_connections = {}
        self.p_backends = {}
        if self.p_af_hashes is not None:
            self.p_af_hashes = {}
            self.p_af_ranked = None
        self.p_rebal_timer.cancel()
        self.p_shuffle_timer.cancel()
        self.p_lp_timer.cancel()
        if self.p_rate_delay_timer is not None:
            self.p_rate_delay_timer.cancel()

    # -- public helpers --------------------------------------------------
    def should_retry_backend(self, backend: str) -> bool:
        return backend in self.p_backends

    def is_declared_dead(self, backend: str) -> bool:
        return self.p_dead.get(backend) is True

    def get_last_error(self) -> Optional[BaseException]:
        return self.p_last_error

    def stop(self) -> None:
        self.emit("stopAsserted")

    def reshuffle(self) -> None:
        """Decoherence shuffle: move the last preference-list entry to a
        random position (lib/pool.js:501-519)."""
        if len(self.p_keys) <= 1:
            return
        taken = self.p_keys.pop()
        idx = random.randrange(len(self.p_keys) + 1)
        conns = sum(len(v) for v in self.p_connections.values())
        if len(self.p_keys) > conns and idx < conns:
            self.p_log.info('random shuffle puts backend "%s" at idx %d',
                            taken, idx)
        self.p_keys.insert(idx, taken)
        self.rebalance()

    # -- rebalancing ------------------------------------------------------
    def rebalance(self) -> None:
        if len(self.p_keys) < 1:
            return
        if self.is_in_state("stopping") or self.is_in_state("stopped"):
            return
        if self.p_rebal_scheduled:
            return
        self.p_rebal_scheduled = True
        self._loop.call_soon(self._rebalance)

    def _rebalance(self) -> None:
        if self.p_in_rebalance:
            return
        self.p_in_rebalance = True
        self.p_rebal_scheduled = False

        total = 0
        counts = []
        for k in self.p_keys:
            n = len(self.p_connections.get(k, ()))
            counts.append(n)
            total += n
        spares = len(self.p_idleq) + len(self.p_initq) - len(self.p_waiters)
        if spares < 0:
            spares = 0
        busy = total - spares
        if busy < 0:
            busy = 0
        extras = len(self.p_waiters) - len(self.p_initq)
        if extras < 0:
            extras = 0

        # Size for the peak demand of the interval, not just this
        # instant (see p_demand_hwm comment in __init__).
        demand = busy + extras
        if demand < self.p_demand_hwm:
            demand = self.p_demand_hwm
        self.p_demand_hwm = busy + extras

        target = demand + self.p_spares

        # Anti-shrink clamp from the low-pass filter (lib/pool.js:579-588)
        lpf_min = math.ceil(self.p_lpf.get())
        if target < lpf_min * 1.05:
            target = lpf_min
            self.p_last_rebal_clamped = True
        else:
            self.p_last_rebal_clamped = False

        if target > self.p_max:
            target = self.p_max
        lim = self.p_cl_lim
        if lim is not None:
            # claims held by the limit wait for a lease to end, not for
            # a connection: they must not open what may not be used
            cap = int(math.floor(lim.limit)) + self.p_spares
            if target > cap:
                target = cap

        census = (target, tuple(counts), tuple(self.p_keys),
                  tuple(sorted(self.p_dead)))
        ranks = self.p_ranks
        if ranks is not None:
            # a rank edit changes the plan without changing any count
            census += (self.p_rank_gen,)
        ejected = self.p_od_ejected
        if ejected:
            # an ejection changes the plan without changing any count
            census += (tuple(sorted(ejected)),)
        if census == self.p_noop_census:
            self.p_in_rebalance = False
            self.p_last_rebalance = mod_time.time()
            return

        # An ejected backend gets no connections at all: the planner
        # never sees its key (its slots are unwanted and on their way
        # out already).
        keys = self.p_keys
        if ejected:
            keys = [k for k in keys if k not in ejected]
        conns: Dict[str, List[ConnectionSlotFSM]] = {}
        for k in keys:
            conns[k] = list(self.p_connections.get(k, ()))

        plan = mod_utils.plan_rebalance(conns, self.p_dead, target,
                                        self.p_max, ranks=ranks)
        if ranks is not None:
            self._note_active_priority(mod_utils.active_priority(
                keys, self.p_dead, ranks))
        self.p_noop_census = None if (plan["remove"] or plan["add"]) \
            else census

        if plan["remove"] or plan["add"]:
            self.p_log.trace(
                "rebalancing pool, remove %d, add %d (busy = %d, spares = "
                "%d, target = %d)", len(plan["remove"]), len(plan["add"]),
                busy, spares, target)

        now = self._loop.time()
        rate_delay: Optional[float] = None

        for fsm in plan["remove"]:
            k = fsm.get_backend()["key"]
            lastrate = self.p_lastrate.get(k)
            n = len(self.p_connections.get(k, ())) - 1
            if lastrate:
                tdelta = now - lastrate["time"]
                ndelta = n - lastrate["count"]
                rate = abs(ndelta / tdelta) if tdelta else math.inf
                if rate > self.p_maxrate:
                    tnext = lastrate["time"] + abs(ndelta) / self.p_maxrate
                    delay = tnext - now
                    if rate_delay is None or delay < rate_delay:
                        rate_delay = delay
                    continue
            self.p_lastrate[k] = {"time": now, "count": n}

            fsm.set_unwanted()
            # The slot may have gone stopped/failed synchronously; if so
            # it no longer counts against the cap (lib/pool.js:623-631).
            if fsm.is_in_state("stopped") or fsm.is_in_state("failed"):
                total -= 1

        for k in plan["add"]:
            lastrate = self.p_lastrate.get(k)
            n = len(self.p_connections.get(k, ())) + 1
            if lastrate:
                tdelta = now - lastrate["time"]
                ndelta = n - lastrate["count"]
                rate = abs(ndelta / tdelta) if tdelta else math.inf
                if rate > self.p_maxrate:
                    tnext = lastrate["time"] + abs(ndelta) / self.p_maxrate
                    delay = tnext - now
                    if rate_delay is None or delay < rate_delay:
                        rate_delay = delay
                    continue
            self.p_lastrate[k] = {"time": now, "count": n}
            total += 1
            if total > self.p_max:  # never exceed the socket limit
                continue
            self.add_connection(k)

        if rate_delay is not None:
            if self.p_rate_delay_timer is not None:
                self.p_rate_delay_timer.cancel()
            self.p_rate_delay_timer = self._loop.call_later(
                rate_delay + 0.01, self.rebalance)

        self.p_in_rebalance = False
        self.p_last_rebalance = mod_time.time()

    def _note_active_priority(self, new: Optional[int]) -> None:
        old = self.p_active_priority
        if new == old:
            return
        self.p_active_priority = new
        if old is None or new is None:
            return  # first backends seen: nothing to fail over from
        self.p_log.info("failing %s to priority %d"
                        % ("over" if new > old else "back", new))
        self._incr_counter("priority-changed")
        self.emit("priorityChanged", old, new)

    def get_ranking(self) -> Dict[str, Any]:
        """SRV ranking as the pool sees it: ``{"enabled",
        "activePriority", "tiers": [{"priority", "backends", "dead",
        "connections", "weights": {key: weight}}, ...]}``, tiers in
        ascending priority order; ``{"enabled": False}`` when the pool
        was created without ``srvRanking``."""
        return mod_utils.ranking_report(
            self.p_keys, self.p_dead, self.p_ranks,
            {k: len(v) for k, v in self.p_connections.items()})

    # -- connection age / recycle() ------------------------------------------
    #
    # Every connected socket may carry a deadline: its connect time plus
    # a lifetime drawn once per socket (maxConnectionAge), or "now"
    # (recycle()).  One call_at timer waits for the earliest deadline
    # still ahead; everything else is driven by events the pool sees
    # anyway: a socket manager connecting, a slot stopping or failing.
    # Retirement is set_unwanted() on the slot, so the replacement is
    # the ordinary rebalance's business.  None of this is reachable
    # from claim() or from the slot's busy/idle cycle.

    def _age_watch(self, fsm: ConnectionSlotFSM) -> None:
        fsm.csf_smgr.on("stateChanged",
                        functools.partial(self._age_smgr_changed, fsm))

    def _age_smgr_changed(self, fsm: ConnectionSlotFSM, st: str) -> None:
        if st == "connected":
            smgr = fsm.csf_smgr
            if smgr.is_in_state("connected") and \
                    fsm not in self.p_age_retiring:
                if self.p_age_max is not None:
                    life = self.p_age_max * \
                        (1.0 - self.p_age_spread * random.random())
                    self.p_age_slots[fsm] = [
                        smgr.sm_connected_at + life / 1000.0, "age"]
                else:
                    # a new socket: a recycle() mark was for the old one
                    self.p_age_slots.pop(fsm, None)
            # Next turn: the slot itself has not seen this event yet
            # and still counts as connecting.
            self._loop.call_soon(self._age_run)
        elif st == "error" or st == "closed":
            self.p_age_slots.pop(fsm, None)

    def _age_slot_gone(self, fsm: ConnectionSlotFSM) -> None:
        """A slot stopped or failed.  Held-back retirements are looked
        at again once the rebalance this just scheduled has run, so
        that a replacement it opens is seen as in flight."""
        self.p_age_slots.pop(fsm, None)
        self.p_age_retiring.pop(fsm, None)
        self.p_age_settling += 1
        self._loop.call_soon(self._age_settled)

    def _age_settled(self) -> None:
        self.p_age_settling -= 1
        self._age_run()

    def _age_in_flight(self) -> bool:
        if self.p_age_settling > 0:
            return True
        for fsm in self.p_age_retiring:
            # a marked lease counts once it begins stopping
            if fsm._fsm_state != "busy":
                return True
        for conns in self.p_connections.values():
            for fsm in conns:
                if not fsm.csf_monitor and fsm._fsm_state in (
                        "init", "connecting", "retrying"):
                    return True
        return False

    def _age_timer_fired(self) -> None:
        at = self.p_age_timer_at
        self.p_age_timer = None
        self.p_age_timer_at = None
        # a loop may fire a timer a clock tick early
        self._age_run(max(self._loop.time(), at))

    def _age_run(self, now: Optional[float] = None) -> None:
        """Retire what is due: every busy slot is marked, idle slots go
        oldest deadline first and one at a time.  Then re-arm the timer."""
        if self._fsm_state != "running":
            return
        if now is None:
            now = self._loop.time()
        slots = self.p_age_slots
        due = [(ent[0], i, fsm) for i, (fsm, ent) in
               enumerate(slots.items()) if ent[0] <= now]
        if due:
            due.sort()
            blocked: Optional[bool] = None
            for _, _, fsm in due:
                st = fsm._fsm_state
                if st == "busy":
                    self._age_retire(fsm, now)
                elif st == "idle":
                    if blocked is None:
                        blocked = self._age_in_flight()
                    if not blocked:
                        self._age_retire(fsm, now)
                        blocked = True
                # any other state is on its way somewhere: the event
                # that ends it brings us back here
        nxt: Optional[float] = None
        for ent in slots.values():
            if ent[0] > now and (nxt is None or ent[0] < nxt):
                nxt = ent[0]
        if nxt != self.p_age_timer_at:
            if self.p_age_timer is not None:
                self.p_age_timer.cancel()
                self.p_age_timer = None
            if nxt is not None:
                self.p_age_timer = self._loop.call_at(
                    nxt, self._age_timer_fired)
            self.p_age_timer_at = nxt

    def _age_retire(self, fsm: ConnectionSlotFSM, now: float) -> None:
        reason = self.p_age_slots.pop(fsm)[1]
        self.p_age_retiring[fsm] = reason
        key = fsm.csf_backend.get("key")
        at = fsm.csf_smgr.sm_connected_at
        fsm.csf_log.info(
            'recycling connection to backend "%s" (%s) at age %d ms',
            key, reason, round((now - at) * 1000.0) if at is not None else 0)
        self._incr_counter("recycled-" + reason)
        # idle: stops now; busy: stops when its lease is released
        fsm.set_unwanted()
        self.emit("connectionRecycled", key, reason)

    def _age_oldest(self, now: float) -> Optional[float]:
        """Age in seconds of the oldest connected socket, or None."""
        oldest: Optional[float] = None
        for conns in self.p_connections.values():
            for fsm in conns:
                smgr = fsm.csf_smgr
                if smgr._fsm_state == "connected":
                    age = now - smgr.sm_connected_at
                    if oldest is None or age > oldest:
                        oldest = age
        return oldest

    def recycle(self) -> int:
        """Treat every socket connected right now as expired: idle ones
        are retired one at a time, each after the previous one's
        replacement connected; claimed ones when their lease is
        released.  Connections opened later are unaffected.  Returns
        the number of connections marked (0 once the pool is stopping,
        stopped or failed)."""
        if self._fsm_state not in ("starting", "running"):
            return 0
        if self.p_age_slots is None:
            self.p_age_slots = {}
            self.p_age_retiring = {}
            for conns in self.p_connections.values():
                for fsm in conns:
                    self._age_watch(fsm)
        now = self._loop.time()
        marked = 0
        for conns in self.p_connections.values():
            for fsm in conns:
                if fsm in self.p_age_retiring or \
                        fsm.csf_smgr._fsm_state != "connected":
                    continue
                ent = self.p_age_slots.get(fsm)
                at = now if ent is None or ent[0] > now else ent[0]
                self.p_age_slots[fsm] = [at, "manual"]
                marked += 1
        self._age_run(now)
        return marked

    def get_connection_ages(self) -> Dict[str, Any]:
        """``{"maxAgeMs", "oldestMs", "connections": [{"backend",
        "state", "ageMs", "expiresInMs", "recycling"}, ...]}``; ages
        and expiries are None for a slot without a connected socket,
        ``expiresInMs`` also for a socket without a deadline."""
        now = self._loop.time()
        slots = self.p_age_slots or {}
        retiring = self.p_age_retiring or {}
        out = []
        for k, conns in self.p_connections.items():
            for fsm in conns:
                smgr = fsm.csf_smgr
                age = expires = None
                if smgr._fsm_state == "connected":
                    age = (now - smgr.sm_connected_at) * 1000.0
                    ent = slots.get(fsm)
                    if ent is not None:
                        expires = max(0.0, (ent[0] - now) * 1000.0)
                out.append({"backend": k, "state": fsm.get_state(),
                            "ageMs": age, "expiresInMs": expires,
                            "recycling": fsm in retiring})
        oldest = self._age_oldest(now)
        return {"maxAgeMs": self.p_age_max,
                "oldestMs": None if oldest is None else oldest * 1000.0,
                "connections": out}

    # -- outlier ejection ----------------------------------------------------
    #
    # Passive health: a backend that accepts connections but fails the
    # requests sent over them.  "Dead" (p_dead) means connects fail, and
    # a monitor slot probes until one succeeds; "ejected" means leases
    # fail, so a successful connect proves nothing: the backend gets no
    # connection at all for a fixed time and is then simply tried again.
    #
    # Leases are observed from outside the claim path.  A pool with the
    # option listens to each slot and its socket manager.  stateChanged
    # is asynchronous, so the listener never trusts the slot's present
    # state: a lease is pinned to its handle when the slot's 'busy' is
    # delivered (csf_handle, or csf_prev_handle if the slot has been
    # released to idle since; the pool cannot hand the slot out again
    # before it has seen the 'idle' that follows in the same queue), and
    # judged when the slot's next state is delivered, which says how the
    # lease left 'busy'.  By then the handle is terminal.

    def _od_init(self) -> None:
        if self.p_od_backends is None:
            self.p_od_backends = {}
            self.p_od_ejected = {}

    def _od_record(self, key: str) -> Dict[str, Any]:
        rec = self.p_od_backends.get(key)
        if rec is None:
            rec = self.p_od_backends[key] = {
                "streak": 0, "failures": 0, "successes": 0,
                # consecutive ejections; back to 0 at "cleanAt"
                "ejections": 0, "cleanAt": None}
        return rec

    def _od_ejections(self, key: str, rec: Dict[str, Any],
                      now: float) -> int:
        """The backend's count of consecutive ejections, forgotten once
        it has stayed reinstated for as long as its last ejection
        lasted."""
        clean_at = rec["cleanAt"]
        if clean_at is not None and key not in self.p_od_ejected and \
                now + 1e-9 >= clean_at:
            rec["ejections"] = 0
            rec["cleanAt"] = None
        return rec["ejections"]

    def _od_watch(self, fsm: ConnectionSlotFSM, key: str) -> None:
        fsm.on("stateChanged",
               functools.partial(self._od_slot_changed, fsm, key))
        fsm.csf_smgr.on("stateChanged",
                        functools.partial(self._od_smgr_changed, fsm))

    def _od_smgr_changed(self, fsm: ConnectionSlotFSM, st: str) -> None:
        if st == "error" or st == "closed":
            self.p_od_sock[fsm] = st
        elif st == "connected":
            self.p_od_sock.pop(fsm, None)

    def _od_slot_changed(self, fsm: ConnectionSlotFSM, key: str,
                         st: str) -> None:
        if st == "busy":
            hdl = fsm.csf_handle
            if hdl is None:
                hdl = fsm.csf_prev_handle
            # a claim the slot rejected leaves no handle behind, and
            # csf_prev_handle is then the lease before: judged already
            if hdl is None or hdl is self.p_od_last.get(fsm) or \
                    hdl.ch_slot is not fsm or hdl._fsm_state not in (
                        "claimed", "released", "closed"):
                return
            self.p_od_last[fsm] = hdl
            self.p_od_open[fsm] = hdl
            return
        hdl = self.p_od_open.pop(fsm, None)
        if hdl is not None:
            self._od_lease_ended(fsm, key, hdl, st)
        if st == "stopped" or st == "failed":
            self.p_od_last.pop(fsm, None)
            self.p_od_sock.pop(fsm, None)

    def _od_lease_ended(self, fsm: ConnectionSlotFSM, key: str, hdl: Any,
                        nxt: str) -> None:
        """Judge one lease: `nxt` is the state the slot left 'busy' for.
        True is a failure, False a success, None neutral."""
        od = self.p_od
        closed = hdl._fsm_state == "closed"
        # How the socket ended, if it did.  The slot may have left
        # 'busy' as if all were well ('idle', 'stopping', 'killing')
        # although the socket was gone: a socket that is destroyed on
        # 'error' emits 'close' from inside the socket manager's
        # transition, and a claimer that releases on 'close' is then
        # heard before the socket manager is.  What the socket manager
        # has reported by now settles it.
        how = self.p_od_sock.get(fsm)
        if how == "closed" and (nxt == "killing" or nxt == "stopping"):
            how = None          # the slot's own doing, on entering `nxt`
        if how is None:
            if nxt == "connecting" or nxt == "stopped":
                how = "closed"
            elif nxt == "retrying":
                how = "error"
        failed: Optional[bool] = None
        if how == "error":
            failed = True
        elif how == "closed":
            if od["countSocketClose"] or (closed and od["countClose"]):
                failed = True
        elif closed:
            if od["countClose"]:
                failed = True
        elif not hdl.ch_pinger:
            failed = False      # released, socket still connected
        if closed and hdl.ch_pinger:
            failed = True       # a failed health check
        if hdl.ch_failure_reported:
            failed = True
        if failed is None or key not in self.p_backends:
            return
        rec = self._od_record(key)
        if not failed:
            rec["successes"] += 1
            rec["streak"] = 0
            return
        rec["failures"] += 1
        rec["streak"] += 1
        if rec["streak"] >= od["consecutiveFailures"] and \
                key not in self.p_od_ejected:
            self._od_eject(key, "consecutive-failures", None)

    def _od_usable_without(self, key: str) -> bool:
        """Would a backend that is neither ejected nor declared dead be
        left without `key`?"""
        for k in self.p_keys:
            if k != key and k not in self.p_od_ejected and \
                    k not in self.p_dead:
                return True
        return False

    def _od_eject(self, key: str, reason: str,
                  ms: Optional[float]) -> bool:
        # A lease may outlive the pool's working life (it is held
        # through 'stopping.backends'); a pool that is winding down or
        # has failed ejects nothing and arms no timer.
        if self._fsm_state not in ("starting", "running"):
            return False
        ejected = self.p_od_ejected
        refused = not self._od_usable_without(key)
        if not refused and reason != "manual":
            share = (len(ejected) + 1) * 100.0 / len(self.p_keys)
            refused = share > self.p_od["maxEjectionPercent"]
        if refused:
            if reason != "manual":
                # the counter is an alarm about failing backends that
                # had to stay; an operator's refused request is not one
                self._incr_counter("ejection-refused")
            self.p_log.info('not ejecting backend "%s" (%s): too few '
                            'backends would be left', key, reason)
            return False

        now = self._loop.time()
        rec = self._od_record(key)
        n = self._od_ejections(key, rec, now) + 1
        rec["ejections"] = n
        if ms is None:
            od = self.p_od
            ms = min(od["baseEjectionTime"] * 2.0 ** (n - 1),
                     od["maxEjectionTime"])
        ent: Dict[str, Any] = {"reason": reason, "at": now,
                               "until": now + ms / 1000.0,
                               "durationMs": ms}
        ent["timer"] = self._loop.call_at(
            ent["until"], self._od_expired, key, ent)
        ejected[key] = ent
        self.p_log.warn('ejecting backend "%s" (%s) for %d ms',
                        key, reason, ms)
        self._incr_counter("backend-ejected")
        # Every slot goes, a monitor included, and not at maxChurnRate's
        # pace: idle ones stop now, claimed ones when released.
        for fsm in list(self.p_connections.get(key, ())):
            fsm.set_unwanted()
        self.rebalance()
        self.emit("backendEjected", key, {
            "reason": reason, "durationMs": ms, "ejections": n})
        return True

    def _od_expired(self, key: str, ent: Dict[str, Any]) -> None:
        if self.p_od_ejected.get(key) is ent and \
                self._fsm_state in ("starting", "running", "failed"):
            self._od_reinstate(key, "expired")

    def _od_reinstate(self, key: str, reason: str) -> None:
        ent = self.p_od_ejected.pop(key)
        ent["timer"].cancel()
        now = self._loop.time()
        rec = self._od_record(key)
        rec["streak"] = 0
        rec["cleanAt"] = now + ent["durationMs"] / 1000.0
        self.p_log.info('reinstating backend "%s" (%s)', key, reason)
        self._incr_counter("backend-reinstated")
        self.rebalance()
        self.emit("backendReinstated", key, reason)

    def _od_panic_check(self) -> None:
        """A backend was just declared dead, or removed by the
        resolver.  If that leaves none that is neither dead nor
        ejected, a suspect backend is better than none: lift every
        ejection."""
        ejected = self.p_od_ejected
        for k in self.p_keys:
            if k not in ejected and k not in self.p_dead:
                return
        for k in list(ejected):
            self._od_reinstate(k, "panic")

    def eject_backend(self, key: str, ms: Optional[float] = None) -> bool:
        """Eject backend `key` by hand for `ms` milliseconds (default:
        what outlier detection would give it next; required on a pool
        without ``outlierDetection``).  ``maxEjectionPercent`` does not
        apply.  False for an unknown or already ejected key, for the
        last usable backend, and for a pool that is not starting or
        running."""
        if ms is None:
            if self.p_od is None:
                raise ValueError("eject_backend() needs ms on a pool "
                                 "without outlierDetection")
        elif not mod_utils._num(ms):
            raise TypeError("ms must be a number")
        elif not math.isfinite(ms) or ms <= 0:
            raise ValueError("ms must be finite and > 0")
        if self._fsm_state not in ("starting", "running"):
            return False
        if key not in self.p_backends:
            return False
        self._od_init()
        if key in self.p_od_ejected:
            return False
        return self._od_eject(key, "manual", ms)

    def reinstate_backend(self, key: str) -> bool:
        """End the ejection of backend `key` now; False when it is not
        ejected."""
        if not self.p_od_ejected or key not in self.p_od_ejected:
            return False
        self._od_reinstate(key, "manual")
        return True

    def get_outlier_stats(self) -> Dict[str, Any]:
        """``{"enabled", "ejected": n, "backends": {key:
        {"consecutiveFailures", "failures", "successes", "ejected",
        "ejections", "ejectedForMs", "reinstatesInMs"}}}``, one entry
        per backend the pool knows; ``ejections`` counts consecutive
        ejections, and the two times are None for a backend that is not
        ejected."""
        now = self._loop.time()
        ejected = self.p_od_ejected or {}
        recs = self.p_od_backends or {}
        out: Dict[str, Any] = {}
        for k in self.p_keys:
            rec = recs.get(k)
            ent = ejected.get(k)
            out[k] = {
                "consecutiveFailures": rec["streak"] if rec else 0,
                "failures": rec["failures"] if rec else 0,
                "successes": rec["successes"] if rec else 0,
                "ejected": ent is not None,
                "ejections":
                    self._od_ejections(k, rec, now) if rec else 0,
                "ejectedForMs":
                    None if ent is None else (now - ent["at"]) * 1000.0,
                "reinstatesInMs": None if ent is None else
                    max(0.0, (ent["until"] - now) * 1000.0),
            }
        return {"enabled": self.p_od is not None,
                "ejected": len(ejected), "backends": out}

    # -- claim balancing -----------------------------------------------------
    #
    # Without the option a claim takes the head of the idle queue, and a
    # released slot goes to its tail: round-robin over idle connections,
    # whatever their backends take to answer.  With it, the claim's
    # ticket looks at the idle slots (all of them, or a few drawn at
    # random) and takes the one whose backend is cheapest by
    # balance.backend_costs(): its lease latency estimate times the
    # connections it has in use, plus one.
    #
    # Only the choice among idle slots changes.  When nothing is idle
    # the claim queues like any other, and the first slot to go idle
    # feeds the head waiter; the balancer has no say there.
    #
    # Leases are observed from outside the claim path, by the scheme of
    # outlier detection above: pinned to their handle when the slot's
    # 'busy' is heard, timed on the loop's clock from there to the
    # slot's next state being heard, and judged by what that state is.
    # A lease that failed leaves no sample, or a backend that fails fast
    # would look fast: such backends are outlierDetection's business.
    # Pinger leases are ignored altogether.

    def _lb_record(self, key: str) -> Any:
        rec = self.p_lb_backends.get(key)
        if rec is None:
            rec = mod_balance.BackendLoad(self.p_lb["decayTime"])
            if key in self.p_backends:
                self.p_lb_backends[key] = rec
            # else a slot of a backend that is gone already: counted on
            # a record that nobody keeps
        return rec

    def _lb_watch(self, fsm: ConnectionSlotFSM, key: str) -> None:
        fsm.on("stateChanged",
               functools.partial(self._lb_slot_changed, fsm, key))

    def _lb_slot_changed(self, fsm: ConnectionSlotFSM, key: str,
                         st: str) -> None:
        if st == "busy":
            handed = self.p_lb_handed.pop(fsm, None)
            hdl = fsm.csf_handle
            if hdl is None:
                hdl = fsm.csf_prev_handle
            # a claim the slot rejected leaves no handle behind, and
            # csf_prev_handle is then the lease before: seen already
            if hdl is None or hdl is self.p_lb_last.get(fsm) or \
                    hdl.ch_slot is not fsm or hdl._fsm_state not in (
                        "claimed", "released", "closed"):
                hdl = None
            if handed is not None and handed[0] is not hdl:
                handed[1].outstanding -= 1      # nothing came of it
                handed = None
            if hdl is None:
                return
            self.p_lb_last[fsm] = hdl
            if hdl.ch_pinger:
                return
            if handed is not None:
                rec = handed[1]                 # counted by the ticket
            else:
                # the lease began by feeding a waiter
                rec = self._lb_record(key)
                rec.outstanding += 1
            self.p_lb_open[fsm] = (hdl, rec, self._loop.time())
            return
        ent = self.p_lb_open.pop(fsm, None)
        if ent is not None:
            hdl, rec, t0 = ent
            rec.outstanding -= 1
            rec.leases += 1
            if hdl._fsm_state == "closed" or hdl.ch_failure_reported or \
                    st in ("retrying", "connecting", "failed", "stopped"):
                rec.failed += 1
            else:
                now = self._loop.time()
                rec.ewma.observe((now - t0) * 1000.0, now * 1000.0)
        if st == "stopped" or st == "failed":
            self.p_lb_last.pop(fsm, None)
            handed = self.p_lb_handed.pop(fsm, None)
            if handed is not None:
                handed[1].outstanding -= 1

    def _lb_pick(self, avoid: Optional[frozenset]) -> Optional[tuple]:
        """Unlink the idle slot the balancer chooses and return it, with
        whether it was not the first idle slot in queue order; None when
        nothing is idle.  The queue discipline of _idle_avoiding:
        stale entries met on the walk are unlinked, idle slots that are
        passed over stay linked where they are."""
        entries = list(self.p_idleq)
        m = len(entries)
        head = 0
        while head < m and entries[head]._fsm_state != "idle":
            fsm = entries[head]
            fsm.p_idleq_node.remove()
            fsm.p_idleq_node = None
            head += 1
        if head == m:
            return None
        first = entries[head]
        lb = self.p_lb
        n = lb["choices"]
        if n != "all" and avoid is None and m - head > n:
            # the common case of a few choices: no need to look at
            # every entry
            cands = self._lb_draw(entries, head, n)
        else:
            cands = [first]
            for fsm in entries[head + 1:]:
                if fsm._fsm_state == "idle":
                    cands.append(fsm)
                else:
                    fsm.p_idleq_node.remove()
                    fsm.p_idleq_node = None
            if avoid is not None:
                # the avoid filter narrows first, and yields when it
                # would leave nothing
                cands = [fsm for fsm in cands
                         if fsm.csf_backend.get("key") not in avoid] or cands
            if n != "all" and len(cands) > n:
                # uniformly, without replacement, still in queue order
                rng = lb["rng"] or random
                cands = [cands[i] for i in
                         sorted(rng.sample(range(len(cands)), n))]
        fsm = cands[0]
        if len(cands) > 1:
            loads = self.p_lb_backends
            # The cost is the backend's and a tie goes to the earliest:
            # only the first candidate of each backend can win.  A slot
            # of a backend that is gone already has no record, and
            # comes last.
            firsts: Dict[str, ConnectionSlotFSM] = {}
            for c in cands:
                k = c.csf_backend.get("key")
                if k not in firsts:
                    firsts[k] = c
                    self._lb_record(k)
            if len(firsts) > 1:
                costs = mod_balance.backend_costs(
                    loads, self._loop.time() * 1000.0, lb["policy"],
                    [k for k in firsts if k in loads])
                fsm = mod_balance.pick(
                    [(c, costs.get(k, math.inf))
                     for k, c in firsts.items()])
        fsm.p_idleq_node.remove()
        fsm.p_idleq_node = None
        return fsm, fsm is not first

    def _lb_draw(self, entries: List[ConnectionSlotFSM], head: int,
                 n: int) -> List[ConnectionSlotFSM]:
        """`n` of the live slots among ``entries[head:]``, drawn
        uniformly without replacement (a partial Fisher-Yates shuffle of
        the positions; a stale entry that is drawn is unlinked and drawn
        over), in queue order.  ``entries[head]`` is live, so the result
        is never empty."""
        rnd = (self.p_lb["rng"] or random).random
        order = list(range(head, len(entries)))
        left = len(order)
        chosen: List[int] = []
        i = 0
        while i < left and len(chosen) < n:
            j = i + int(rnd() * (left - i))
            order[i], order[j] = order[j], order[i]
            fsm = entries[order[i]]
            if fsm._fsm_state == "idle":
                chosen.append(order[i])
            else:
                fsm.p_idleq_node.remove()
                fsm.p_idleq_node = None
            i += 1
        chosen.sort()
        return [entries[k] for k in chosen]

    def _ticket_balanced(self, handle: ClaimHandle, err_on_empty: bool,
                         avoid: Optional[frozenset]) -> None:
        """_ticket_slow with the balancer's choice in place of the head
        of the idle queue; everything else is _ticket_slow itself."""
        if handle.is_in_state("waiting") and \
                self._fsm_state in ("starting", "running") and not (
                    self.p_cl_lim is not None and
                    self.p_cl_inflight >= self.p_cl_allowed):
            picked = self._lb_pick(avoid)
            if picked is not None:
                fsm, reordered = picked
                # counted from here, so that a burst of claims in one
                # loop turn sees its own picks
                rec = self._lb_record(fsm.csf_backend.get("key"))
                rec.outstanding += 1
                handle.try_(fsm)
                if handle._fsm_state in ("waiting", "cancelled"):
                    # rejected: the slot's socket was gone already.  The
                    # handle's 'waiting' brings the ticket back here.
                    rec.outstanding -= 1
                else:
                    self.p_lb_handed[fsm] = (handle, rec)
                    rec.picked += 1
                    if self.p_cl_lim is not None:
                        self._cl_handoff(handle, fsm)
                    counters = self.p_counters
                    counters["balanced-claim"] = \
                        counters.get("balanced-claim", 0) + 1
                    if reordered:
                        counters["balanced-reordered"] = \
                            counters.get("balanced-reordered", 0) + 1
                self._note_demand()
                return
        # nothing idle (the walk has emptied the queue), the pool is on
        # its way out, or it is at its concurrency limit
        self._ticket_slow(handle, err_on_empty)

    def _claim_balanced(self, options: Any = None,
                        cb: Optional[Callable] = None):
        """claim() of a pool with ``claimBalancing`` (installed on the
        instance): the same options, counters and return values; the
        handle is the runtime's own, its ticket a _BalancedClaimTicket."""
        handle, stub, err_on_empty, avoid, _, akey = \
            self._claim_begin(options, cb)
        if handle is None:
            return stub
        if akey is not None:
            ticket: Any = _AffinityClaimTicket(self, handle, err_on_empty,
                                               avoid, akey)
        else:
            ticket = _BalancedClaimTicket(self, handle, err_on_empty, avoid)
        handle.on("stateChanged", ticket)
        return handle

    def _lb_publish(self) -> None:
        lat_gauge, out_gauge = self._lb_gauges
        now = self._loop.time() * 1000.0
        for k, rec in self.p_lb_backends.items():
            labels = {**self._gauge_labels, "backend": k}
            out_gauge.set(rec.outstanding, labels)
            est = rec.ewma.get(now)
            if est is not None:
                lat_gauge.set(est / 1000.0, labels)

    def get_balancing_stats(self) -> Dict[str, Any]:
        """Claim balancing as the pool sees it: ``{"enabled", "policy",
        "choices", "decayTimeMs", "backends": {key: {"connections",
        "idle", "outstanding", "leases", "failedLeases", "latencyMs",
        "cost", "picked"}}}``, one entry per backend the pool knows.
        ``latencyMs`` is the estimate aged to now, None before the first
        sample; ``leases`` counts the leases that ended, the failed ones
        included.  ``{"enabled": False}`` when the pool was created
        without ``claimBalancing``."""
        lb = self.p_lb
        if lb is None:
            return {"enabled": False}
        now = self._loop.time() * 1000.0
        loads = {k: self._lb_record(k) for k in self.p_keys}
        costs = mod_balance.backend_costs(loads, now, lb["policy"])
        out: Dict[str, Any] = {}
        for k, rec in loads.items():
            conns = self.p_connections.get(k, ())
            out[k] = {
                "connections": len(conns),
                "idle": sum(1 for fsm in conns
                            if fsm._fsm_state == "idle"),
                "outstanding": rec.outstanding,
                "leases": rec.leases,
                "failedLeases": rec.failed,
                "latencyMs": rec.ewma.get(now),
                "cost": costs[k],
                "picked": rec.picked,
            }
        return {"enabled": True, "policy": lb["policy"],
                "choices": lb["choices"], "decayTimeMs": lb["decayTime"],
                "backends": out}

    # -- claim queue (opt-in) ------------------------------------------------
    #
    # With ``claimQueue`` the waiter queue is bounded, has priority
    # classes and may serve newest-first.  All of it is decided when a
    # claim is linked: the head of p_waiters is always the next claim to
    # serve, so whatever feeds a freed slot (the native dispatcher, the
    # drains, CoDel) shifts the head as it always did.  The queue is
    # kept sorted by class, class 0 at the head.

    def _claim_queued(self, options: Any = None,
                      cb: Optional[Callable] = None):
        """claim() of a pool with ``claimQueue`` (installed on the
        instance): the same options, counters and return values, and
        ``priority``.  The handle is the runtime's own; its ticket is a
        Python one on either runtime, so that every claim that has to
        wait is placed by _ticket_slow."""
        handle, stub, err_on_empty, avoid, prio, akey = \
            self._claim_begin(options, cb)
        if handle is None:
            return stub
        handle.ch_priority = prio
        if akey is not None:
            ticket: Any = _AffinityClaimTicket(self, handle, err_on_empty,
                                               avoid, akey)
        elif self.p_lb is not None:
            ticket = _BalancedClaimTicket(self, handle, err_on_empty,
                                          avoid)
        else:
            ticket = _AvoidClaimTicket(self, handle, err_on_empty, avoid)
        handle.on("stateChanged", ticket)
        return handle

    def _cq_newest_first(self, queued: int, now: float) -> bool:
        """Would a claim that has to wait now be placed ahead of its
        class?  `queued` is the length of the waiter queue."""
        cq = self.p_cq
        order = cq["order"]
        if order == "fifo":
            return False
        if order == "lifo":
            return True
        # adaptive: a queue that has not been empty for lifoAfter ms is
        # not draining, whatever was dequeued in between
        return queued > 0 and now - self.p_cq_since >= cq["lifoAfter"]

    def _cq_place(self, handle: ClaimHandle) -> bool:
        """Link `handle` into the waiter queue where its class and the
        queue's order put it, and enforce ``maxQueued``: the claim that
        would be served last fails with ClaimQueueFullError, be it this
        one (never linked; returns False) or the tail waiter.

        Cost: O(1) with a single class (a push or an unshift, no walk).
        With several classes O(priorities), from the remembered last
        node of each class; when one of the remembered nodes has left
        the queue (served, timed out, cancelled, shed), all of them are
        recomputed in one for_each pass over the queue, at most once per
        placement.

        A claim that ``errorOnEmpty`` has just failed is not linked
        either, nor counted as queued: a pool without the option pushes
        such a handle as the reference does, a dead entry that the next
        feed skips, but here it would take a live claim's place under
        the bound."""
        if not handle.is_in_state("waiting"):
            return False
        cq = self.p_cq
        q = self.p_waiters
        prio = handle.ch_priority
        queued = q._len
        now = self._loop.time() * 1000.0
        if queued == 0:
            # noted on arrival: displacing the only waiter below does
            # not count as the queue having emptied
            self.p_cq_since = now
        newest_first = self._cq_newest_first(queued, now)

        bound = cq["maxQueued"]
        if bound is not None and queued >= bound:
            tail = q.peek_last()
            tail_prio = tail.ch_priority
            if tail_prio < prio or (tail_prio == prio and not newest_first):
                # this claim would be the tail
                self._incr_counter("queue-rejected")
                handle.fail(mod_errors.ClaimQueueFullError(self, False))
                return False
            self._incr_counter("queue-shed")
            tail.fail(mod_errors.ClaimQueueFullError(self, True))

        last = self.p_cq_last
        if last is None:
            node = q.unshift(handle) if newest_first else q.push(handle)
        else:
            # every class is looked at, not only the ones this placement
            # needs: a node that has left the queue (the tail shed just
            # now, for one) is let go of, and its handle with it
            for n in last:
                if n is not None and not n.linked:
                    last = self._cq_remember()
                    break
            # behind the last waiter of the nearest class that is served
            # ahead of this claim
            anchor = None
            for c in range(prio - 1 if newest_first else prio, -1, -1):
                anchor = last[c]
                if anchor is not None:
                    break
            if anchor is None:
                node = q.unshift(handle)
            else:
                node = q.insert_after(anchor, handle)
            if not newest_first or last[prio] is None:
                last[prio] = node
        handle.ch_waiter_node = node
        if newest_first:
            self._incr_counter("queue-lifo")
        return True

    def _cq_remember(self) -> List[Any]:
        """Recompute the last node of every class in one pass."""
        last: List[Any] = [None] * self.p_cq["priorities"]

        def visit(hdl: ClaimHandle, node: Any) -> None:
            last[hdl.ch_priority] = node

        self.p_waiters.for_each(visit)
        self.p_cq_last = last
        return last

    def _cq_census(self) -> List[int]:
        counts = [0] * self.p_cq["priorities"]

        def visit(hdl: ClaimHandle, node: Any) -> None:
            counts[hdl.ch_priority] += 1

        self.p_waiters.for_each(visit)
        return counts

    def _cq_publish(self) -> None:
        for prio, n in enumerate(self._cq_census()):
            self._cq_gauge.set(n, {**self._gauge_labels,
                                   "priority": str(prio)})

    def get_queue_stats(self) -> Dict[str, Any]:
        """The claim queue as the pool sees it: ``{"enabled",
        "maxQueued", "priorities", "order", "lifo", "queued",
        "rejected", "shed", "lifoPlaced"}``.  ``lifo`` says whether a
        claim that had to wait right now would be placed newest-first;
        ``queued`` has one count per class, from a walk of the queue.
        ``{"enabled": False}`` when the pool was created without
        ``claimQueue``."""
        cq = self.p_cq
        if cq is None:
            return {"enabled": False}
        counters = self.p_counters
        return {"enabled": True, "maxQueued": cq["maxQueued"],
                "priorities": cq["priorities"], "order": cq["order"],
                "lifo": self._cq_newest_first(
                    self.p_waiters._len, self._loop.time() * 1000.0),
                "queued": self._cq_census(),
                "rejected": counters.get("queue-rejected", 0),
                "shed": counters.get("queue-shed", 0),
                "lifoPlaced": counters.get("queue-lifo", 0)}

    # -- key affinity (opt-in) -----------------------------------------------
    #
    # With ``claimAffinity`` a claim may carry an ``affinityKey``, and
    # among the idle connections it then prefers the backend that
    # rendezvous hashing ranks first for the key (cueball_amd.affinity),
    # so that the same key keeps reaching the same backend from every
    # client that sees the same DNS.  A soft preference, like
    # avoidBackends: decided when the claim's ticket runs, among what is
    # idle then.  A claim that finds nothing idle waits like any other,
    # and is fed by whatever frees up first.
    #
    # The load bound reads the slots themselves: a slot is in use from
    # the try_ that hands it over (its state changes there and then, so
    # a burst of claims in one loop turn sees its own picks) until the
    # slot has heard of the lease's end.  Nothing is kept per lease.

    def _af_order(self, key: bytes) -> List[str]:
        """Every backend the resolver lists, in the order `key` prefers
        them."""
        ranked = self.p_af_ranked
        if ranked is None:
            hashes = self.p_af_hashes
            keys = tuple(sorted(hashes))
            ranked = self.p_af_ranked = (
                keys, tuple(hashes[k] for k in keys))
        keys, hashes = ranked
        return [keys[i] for i in mod_affinity.rank(key, hashes)]

    def _af_census(self) -> tuple:
        """``({key: connections in use}, their sum, backends with a
        connection that is idle or in use)``.  A pinger's lease is
        neither."""
        in_use: Dict[str, int] = {}
        total = 0
        live = 0
        for k, conns in self.p_connections.items():
            n = 0
            idle = False
            for fsm in conns:
                st = fsm._fsm_state
                if st == "idle":
                    idle = True
                elif st == "busy":
                    hdl = fsm.csf_handle
                    if hdl is not None and not hdl.ch_pinger:
                        n += 1
            if n > 0 or idle:
                live += 1
            in_use[k] = n
            total += n
        return in_use, total, live

    def _af_unused(self, key: str) -> bool:
        """Has backend `key` no connection in use?  Such a backend is
        under any bound, the cap being 1 at the least, so the common
        case needs no census."""
        for fsm in self.p_connections.get(key, ()):
            if fsm._fsm_state == "busy":
                hdl = fsm.csf_handle
                if hdl is not None and not hdl.ch_pinger:
                    return False
        return True

    def _af_pick(self, order: List[str]) -> Optional[tuple]:
        """Unlink the idle slot that `order` (the key's, avoided
        backends moved to its end) chooses, and return it with whether
        the first backend of the order had an idle slot; None when
        nothing is idle.  One walk, with the queue discipline of
        _idle_avoiding: stale entries that are met are unlinked, idle
        slots that are passed over stay linked where they are.  The walk
        ends at the first choice's first idle slot when that settles
        it, which it does unless the load bound has a say."""
        entries = list(self.p_idleq)
        first = order[0] if order else None
        firsts: Dict[Any, ConnectionSlotFSM] = {}
        fraction = self.p_af["loadFraction"]
        picked = None
        at = 0
        for fsm in entries:
            at += 1
            if fsm._fsm_state != "idle":
                fsm.p_idleq_node.remove()
                fsm.p_idleq_node = None
                continue
            k = fsm.csf_backend.get("key")
            if k not in firsts:
                firsts[k] = fsm
                if k == first:
                    if fraction is None or self._af_unused(k):
                        picked = fsm
                    break
        if picked is None:
            for fsm in entries[at:]:
                if fsm._fsm_state != "idle":
                    fsm.p_idleq_node.remove()
                    fsm.p_idleq_node = None
                    continue
                k = fsm.csf_backend.get("key")
                if k not in firsts:
                    firsts[k] = fsm
            if not firsts:
                return None
            cap = None
            in_use: Dict[str, int] = {}
            if fraction is not None:
                in_use, total, live = self._af_census()
                cap = mod_affinity.cap_of(fraction[0], fraction[1],
                                          total, live or 1)
            spill = None
            for k in order:
                fsm = firsts.get(k)
                if fsm is None:
                    continue
                if cap is None or in_use.get(k, 0) < cap:
                    picked = fsm
                    break
                if spill is None:
                    spill = fsm
            if picked is None:
                # every backend with an idle slot is over the bound (or,
                # the slot of a backend that is gone already: the head
                # of the queue)
                picked = spill if spill is not None else \
                    next(iter(firsts.values()))
        picked.p_idleq_node.remove()
        picked.p_idleq_node = None
        return picked, first in firsts

    def _af_count(self, ticket: _AffinityClaimTicket, outcome: str,
                  first: Optional[str], placed: Optional[str]) -> None:
        ticket.counted = True
        counters = self.p_counters
        counters["affinity-claim"] = counters.get("affinity-claim", 0) + 1
        counters[outcome] = counters.get(outcome, 0) + 1
        books = self.p_af_placed
        for i, k in ((0, first), (1, placed)):
            if k is not None and k in self.p_backends:
                ent = books.get(k)
                if ent is None:
                    ent = books[k] = [0, 0]
                ent[i] += 1

    def _ticket_affine(self, handle: ClaimHandle,
                       ticket: _AffinityClaimTicket) -> None:
        """_ticket_slow with the key's choice in place of the head of
        the idle queue; everything else is _ticket_slow itself."""
        order: List[str] = []
        if handle.is_in_state("waiting") and \
                self._fsm_state in ("starting", "running") and not (
                    self.p_cl_lim is not None and
                    self.p_cl_inflight >= self.p_cl_allowed):
            order = self._af_order(ticket.key)
            avoid = ticket.avoid
            if avoid is not None:
                order = [k for k in order if k not in avoid] + \
                    [k for k in order if k in avoid]
            found = self._af_pick(order)
            if found is not None:
                fsm, first_idle = found
                key = fsm.csf_backend.get("key")
                rec = None
                if self.p_lb is not None:
                    # the balancer's books count the claim as one of
                    # their own (see _ticket_balanced)
                    rec = self._lb_record(key)
                    rec.outstanding += 1
                handle.try_(fsm)
                if handle._fsm_state in ("waiting", "cancelled"):
                    # rejected: the slot's socket was gone already.  The
                    # handle's 'waiting' brings the ticket back here.
                    if rec is not None:
                        rec.outstanding -= 1
                else:
                    if rec is not None:
                        self.p_lb_handed[fsm] = (handle, rec)
                    if self.p_cl_lim is not None:
                        self._cl_handoff(handle, fsm)
                    if not ticket.counted:
                        first = order[0] if order else None
                        if key == first:
                            outcome = "affinity-hit"
                        elif first_idle:
                            outcome = "affinity-spill-load"
                        else:
                            outcome = "affinity-spill-busy"
                        self._af_count(ticket, outcome, first, key)
                self._note_demand()
                return
        # nothing idle (the walk has emptied the queue), the pool is on
        # its way out, or it is at its concurrency limit
        self._ticket_slow(handle, ticket.err_on_empty)
        if not ticket.counted and handle._fsm_state == "waiting":
            self._af_count(ticket, "affinity-queued",
                           order[0] if order else None, None)

    def _claim_affine(self, options: Any = None,
                      cb: Optional[Callable] = None):
        """claim() of a pool with ``claimAffinity`` and neither
        ``claimBalancing`` nor ``claimQueue`` (installed on the
        instance).  A claim without a key is the class's claim(), native
        fast path and all; one with a key gets the runtime's own handle
        and an _AffinityClaimTicket."""
        if not isinstance(options, Mapping) or \
                options.get("affinityKey") is None:
            if self.p_cl_lim is not None:
                return self._claim_limited(options, cb)
            return ConnectionPool.claim(self, options, cb)
        handle, stub, err_on_empty, avoid, _, akey = \
            self._claim_begin(options, cb)
        if handle is None:
            return stub
        handle.on("stateChanged", _AffinityClaimTicket(
            self, handle, err_on_empty, avoid, akey))
        return handle

    def _af_publish(self) -> None:
        counters = self.p_counters
        claims = counters.get("affinity-claim", 0)
        if claims > 0:
            self._af_gauge.set(counters.get("affinity-hit", 0) / claims,
                               self._gauge_labels)

    def get_affinity_order(self, key: Any) -> List[str]:
        """The keys of the backends the resolver lists right now, in
        the order a claim with ``affinityKey`` `key` (bytes, or a str,
        read as UTF-8) prefers them: a function of the key and of DNS
        alone, the same in every client.  A ValueError on a pool
        without ``claimAffinity``."""
        return self._af_order(mod_utils.assert_affinity_key(
            key, self.p_af, "key", "a pool"))

    def get_affinity_stats(self) -> Dict[str, Any]:
        """Key affinity as the pool sees it: ``{"enabled", "loadFactor",
        "claims", "hits", "spilledBusy", "spilledLoad", "queued",
        "backends": {key: {"connections", "idle", "inUse",
        "firstChoice", "placed"}}}``, one entry per backend the pool
        knows.  ``claims`` counts the claims that carried a key, each
        once: when a connection was handed to it (a hit or one of the
        spills), or when it had to wait.  ``firstChoice`` counts the
        ones whose first choice the backend was, ``placed`` the ones
        that were handed one of its connections by their key.
        ``{"enabled": False}`` when the pool was created without
        ``claimAffinity``."""
        af = self.p_af
        if af is None:
            return {"enabled": False}
        counters = self.p_counters
        in_use, _, _ = self._af_census()
        out: Dict[str, Any] = {}
        for k in self.p_keys:
            conns = self.p_connections.get(k, ())
            first, placed = self.p_af_placed.get(k, (0, 0))
            out[k] = {
                "connections": len(conns),
                "idle": sum(1 for fsm in conns
                            if fsm._fsm_state == "idle"),
                "inUse": in_use.get(k, 0),
                "firstChoice": first,
                "placed": placed,
            }
        return {"enabled": True, "loadFactor": af["loadFactor"],
                "claims": counters.get("affinity-claim", 0),
                "hits": counters.get("affinity-hit", 0),
                "spilledBusy": counters.get("affinity-spill-busy", 0),
                "spilledLoad": counters.get("affinity-spill-load", 0),
                "queued": counters.get("affinity-queued", 0),
                "backends": out}

    # -- concurrency limit (opt-in) ------------------------------------------
    #
    # With ``concurrencyLimit`` the pool carries at most ``allowed()``
    # leases at once, a number that follows measured lease latency
    # (cueball_amd.limit).  ``maximum`` stays what it is, a bound on
    # sockets; the limit bounds the work in flight.
    #
    # The gate sits wherever an idle slot meets a claim.  A claim's
    # ticket that finds the pool at its limit takes no idle slot and
    # queues as if none were idle (the ticket gate); a slot that goes
    # idle while the pool is at its limit parks on the idle queue and
    # leaves the waiters where they are (the feed gate); and whenever
    # room appears, by the limit rising or a lease ending, head waiters
    # are fed from the head of the idle queue (the kick).
    #
    # Leases are observed from outside the claim path, by the scheme of
    # claim balancing above.  A lease counts from the try_ that hands
    # its slot over, so that a burst of claims in one loop turn sees
    # itself, and until the slot's next state after 'busy' is heard, or
    # the 'busy' that is heard shows that nothing came of the try.  It
    # is timed on the loop's clock between the two.  A lease that failed
    # leaves no sample; pinger leases are never seen.
    #
    # Accounting and gate share one stateChanged listener per slot,
    # installed in place of the native dispatcher: the lease's end is
    # counted, then _slot_state_changed sees the slot, then the kick.

    def _cl_held(self) -> bool:
        """Is the pool at its limit?  Asked by a ticket about to take an
        idle slot; ``limit-held`` counts the times one was there."""
        if self.p_cl_inflight < self.p_cl_allowed:
            return False
        for fsm in self.p_idleq:
            if fsm._fsm_state == "idle":
                self._incr_counter("limit-held")
                break
        return True

    def _cl_handoff(self, handle: ClaimHandle,
                    fsm: ConnectionSlotFSM) -> None:
        """After every ``handle.try_(fsm)`` of an opted-in pool."""
        if handle._fsm_state in ("waiting", "cancelled"):
            return      # rejected: the slot's socket was gone already
        self.p_cl_handed[fsm] = (
            handle, self.p_cl_lim.on_start(self._loop.time() * 1000.0))
        self.p_cl_inflight += 1

    def _cl_slot_changed(self, fsm: ConnectionSlotFSM, key: str,
                         st: str) -> None:
        fell = False
        if st == "busy":
            handed = self.p_cl_handed.pop(fsm, None)
            hdl = fsm.csf_handle
            if hdl is None:
                hdl = fsm.csf_prev_handle
            # a claim the slot rejected leaves no handle behind, and
            # csf_prev_handle is then the lease before: seen already
            if hdl is None or hdl is self.p_cl_last.get(fsm) or \
                    hdl.ch_slot is not fsm or hdl._fsm_state not in (
                        "claimed", "released", "closed"):
                hdl = None
            if handed is not None and handed[0] is not hdl:
                self._cl_ended(handed[1], None)     # nothing came of it
                fell = True
                handed = None
            if hdl is not None:
                self.p_cl_last[fsm] = hdl
                if not hdl.ch_pinger:
                    if handed is None:
                        # handed over by something that does not report
                        # to _cl_handoff: counted from here
                        handed = (hdl, self.p_cl_lim.on_start(
                            self._loop.time() * 1000.0))
                        self.p_cl_inflight += 1
                    self.p_cl_open[fsm] = handed
        else:
            ent = self.p_cl_open.pop(fsm, None)
            if ent is not None:
                hdl, token = ent
                if hdl._fsm_state == "closed" or hdl.ch_failure_reported \
                        or st in ("retrying", "connecting", "failed",
                                  "stopped"):
                    self._cl_ended(token, None)
                else:
                    now = self._loop.time() * 1000.0
                    self._cl_ended(token, now - token[0])
                fell = True
            if st == "stopped" or st == "failed":
                self.p_cl_last.pop(fsm, None)
                handed = self.p_cl_handed.pop(fsm, None)
                if handed is not None:
                    self._cl_ended(handed[1], None)
                    fell = True
        self._slot_state_changed(fsm, key, st)
        if fell:
            self._cl_kick()

    def _cl_ended(self, token: tuple, hold_ms: Optional[float]) -> None:
        """One lease less in flight; with `hold_ms` None it leaves no
        sample."""
        self.p_cl_inflight -= 1
        lim = self.p_cl_lim
        if hold_ms is None:
            lim.on_discard(token)
            return
        was_probing = lim.probing
        lim.on_sample(token, hold_ms, self._loop.time() * 1000.0)
        if lim.probing and not was_probing:
            self._incr_counter("limit-probe")
        floor = int(math.floor(lim.limit))
        if floor != self.p_cl_floor:
            self._incr_counter("limit-raised" if floor > self.p_cl_floor
                               else "limit-lowered")
            self.p_cl_floor = floor
            self.rebalance()
        allowed = lim.allowed()
        previous = self.p_cl_allowed
        if allowed != previous:
            # the limit moved, or a probe began or ended
            self.p_cl_allowed = allowed
            self.emit("limitChanged", allowed, previous)

    def _cl_kick(self) -> None:
        """Room has appeared under the limit: feed head waiters from the
        head of the idle queue until waiters, idle slots or room run
        out."""
        if self._fsm_state not in ("starting", "running"):
            return
        idleq = self.p_idleq
        waiters = self.p_waiters
        while waiters._len > 0 and idleq._len > 0 and \
                self.p_cl_inflight < self.p_cl_allowed:
            fsm = idleq.shift()
            fsm.p_idleq_node = None
            if not fsm.is_in_state("idle"):
                continue
            if not self._feed_waiters(fsm):
                # every waiter had gone: back where the slot came from
                fsm.p_idleq_node = idleq.unshift(fsm)
                break

    def _claim_limited(self, options: Any = None,
                       cb: Optional[Callable] = None):
        """claim() of a pool with ``concurrencyLimit`` and none of
        ``claimBalancing``, ``claimQueue`` and ``claimAffinity``
        (installed on the instance): the same options, counters and
        return values.  The handle is the runtime's own; its ticket is a
        Python one on either runtime, so that every try passes the gate
        in _ticket_slow."""
        handle, stub, err_on_empty, avoid, _, _ = \
            self._claim_begin(options, cb)
        if handle is None:
            return stub
        handle.on("stateChanged",
                  _AvoidClaimTicket(self, handle, err_on_empty, avoid))
        return handle

    def get_limit_stats(self) -> Dict[str, Any]:
        """The concurrency limit as the pool sees it: ``{"enabled",
        "algorithm", "limit", "allowed", "inFlight", "probing",
        "baselineMs", "lastWindowMeanMs", "windows", "probes",
        "samples", "discarded", "raised", "lowered"}``.  ``limit`` is
        the controller's float, ``allowed`` the integer in force (the
        probe's while ``probing``); ``baselineMs`` is None under
        ``"aimd"`` and before the first probe has ended;
        ``discarded`` counts the leases that left no sample, ``raised``
        and ``lowered`` the windows that moved the limit.
        ``{"enabled": False}`` when the pool was created without
        ``concurrencyLimit``."""
        lim = self.p_cl_lim
        if lim is None:
            return {"enabled": False}
        return {"enabled": True, "algorithm": lim.algorithm,
                "limit": lim.limit, "allowed": self.p_cl_allowed,
                "inFlight": self.p_cl_inflight, "probing": lim.probing,
                "baselineMs": lim.baseline,
                "lastWindowMeanMs": lim.last_mean,
                "windows": lim.windows, "probes": lim.probes,
                "samples": lim.samples, "discarded": lim.discarded,
                "raised": lim.raised, "lowered": lim.lowered}

    # -- slot lifecycle ----------------------------------------------------
    def add_connection(self, key: str) -> None:
        if self.is_in_state("stopping") or self.is_in_state("stopped"):
            return

        backend = self.p_backends[key]
        backend["key"] = key

        fsm = ConnectionSlotFSM({
            "constructor": self.p_constructor,
            "backend": backend,
            "log": self.p_log,
            "pool": self,
            "checker": self.p_checker,
            "checkTimeout": self.p_check_timeout,
            "recovery": self.p_recovery,
            "monitor": self.p_dead.get(key) is True,
            "loop": self._loop,
        })
        self.p_connections.setdefault(key, []).append(fsm)
        self.p_total_conns += 1

        fsm.p_initq_node = self.p_initq.push(fsm)
        fsm.p_idleq_node = None

        # Native dispatcher when available (idle-feed/busy fast paths
        # in C, everything else falls back to _slot_state_changed);
        # else functools.partial, which dispatches at C level.
        if self.p_cl_lim is not None:
            # the limit's accounting and its gate in one listener, in
            # this order whatever else is registered (see _cl_slot_changed)
            fsm.on("stateChanged",
                   functools.partial(self._cl_slot_changed, fsm, key))
        elif _NativeSlotDispatch is not None:
            fsm.on("stateChanged", _NativeSlotDispatch(
                self, fsm, key, self.p_codel is not None))
        else:
            fsm.on("stateChanged",
                   functools.partial(self._slot_state_changed, fsm, key))
        if self.p_age_slots is not None:
            self._age_watch(fsm)
        if self.p_od is not None:
            self._od_watch(fsm, key)
        if self.p_lb is not None:
            self._lb_watch(fsm, key)
        fsm.start()

    def _slot_state_changed(self, fsm: ConnectionSlotFSM, key: str,
                            new_state: str) -> None:
        """The big per-slot dispatcher (lib/pool.js:692-807)."""
        if fsm.p_initq_node is not None:
            if new_state in ("init", "connecting", "retrying"):
                return  # still starting up
            fsm.p_initq_node.remove()
            fsm.p_initq_node = None

        if new_state == "idle":
            self.emit("connectedToBackend", key, fsm)
            if key in self.p_dead:
                del self.p_dead[key]
                self.rebalance()

            if fsm._fsm_state == "idle":
                # Just became available: either released by its user
                # or done connecting.
                if key not in self.p_backends:
                    fsm.set_unwanted()
                    return

                if self.p_cl_lim is not None and \
                        self.p_waiters._len > 0 and \
                        self.p_cl_inflight >= self.p_cl_allowed:
                    # the feed gate: at the limit the waiters stay, and
                    # the slot parks until _cl_kick comes for it
                    pass
                elif self._feed_waiters(fsm):
                    return

                fsm.p_idleq_node = self.p_idleq.push(fsm)
                return

        elif new_state == "busy":
            # Health-checking connections ride the initq so they don't
            # count as busy (lib/pool.js:762-769); inline of
            # fsm.is_running_ping() with the cheap checks first
            hdl = fsm.csf_handle
            if hdl is not None and fsm.p_initq_node is None and \
                    hdl.ch_pinger and fsm._fsm_state == "busy":
                fsm.p_initq_node = self.p_initq.push(fsm)

        elif new_state == "failed":
            if key in self.p_backends:
                self.p_dead[key] = True
                if self.p_od_ejected:
                    # before closedBackend weighs the 'failed' state
                    self._od_panic_check()
            err = fsm.get_socket_mgr().get_last_error()
            if err is not None:
                self.p_last_error = err

        if new_state in ("stopped", "failed"):
            conns = self.p_connections.get(key)
            if conns is not None:
                conns.remove(fsm)
                self.p_total_conns -= 1
                if not conns:
                    del self.p_connections[key]
            self.emit("closedBackend", key, fsm)
            self.rebalance()
            if self.p_age_slots is not None:
                self._age_slot_gone(fsm)

        if fsm.p_idleq_node is not None:
            # Was idle, now isn't: unlink and rebalance in case we were
            # closed or died.
            fsm.p_idleq_node.remove()
            fsm.p_idleq_node = None
            self.rebalance()

    def _feed_waiters(self, fsm: ConnectionSlotFSM) -> bool:
        """Offer the idle `fsm` to the head waiter, with the CoDel drop
        check on each dequeue; False when no waiter was left to take it
        (the queue is empty then, and CoDel is told so)."""
        waiters = self.p_waiters
        while waiters._len > 0:
            hdl = waiters.shift()
            drop = self.p_codel is not None and \
                self.p_codel.overloaded(hdl.ch_started)
            if not hdl.is_in_state("waiting"):
                continue
            if drop:
                hdl.timeout()
                continue
            hdl.try_(fsm)
            if self.p_cl_lim is not None:
                self._cl_handoff(hdl, fsm)
            return True

        if self.p_codel is not None:
            self.p_codel.empty()
        return False

    def print_connections(self) -> None:
        """Debugging helper: dump live connection states and dead set
        (lib/pool.js:812-832)."""
        obj: Dict[str, Dict[str, int]] = {}
        ks = list(self.p_keys)
        for k in self.p_connections.keys():
            if k not in ks:
                ks.append(k)
        for k in ks:
            per_state: Dict[str, int] = {}
            for fsm in self.p_connections.get(k, ()):
                s = fsm.get_state()
                per_state[s] = per_state.get(s, 0) + 1
            obj[k] = per_state
        print("live:", obj)
        print("dead:", dict(self.p_dead))

    # -- stats / claim ------------------------------------------------------
    def get_stats(self) -> Dict[str, Any]:
        tconns = sum(len(v) for v in self.p_connections.values())
        return {
            "counters": dict(self.p_counters),
            "totalConnections": tconns,
            "idleConnections": len(self.p_idleq),
            "pendingConnections": len(self.p_initq),
            "waiterCount": len(self.p_waiters),
        }

    def has_idle_connection(self, avoidBackends: Any = None) -> bool:
        """Is a connection idle right now, on a backend that is not
        among `avoidBackends` (an iterable of backend keys, as for
        ``claim()``)?  A read-only walk of the idle queue: stale
        entries are skipped, not unlinked.  Advisory: a claim's first
        try runs on the next loop turn, and another claim may have
        taken the slot by then."""
        avoid = None
        if avoidBackends is not None:
            avoid = self._assert_avoid(avoidBackends)
        if self.p_cl_lim is not None and \
                self.p_cl_inflight >= self.p_cl_allowed:
            return False    # idle, but not to be had: see _cl_held
        for fsm in self.p_idleq:
            if fsm.is_in_state("idle") and (
                    avoid is None or
                    fsm.csf_backend.get("key") not in avoid):
                return True
        return False

    def _idle_avoiding(self, avoid: frozenset) -> Optional[ConnectionSlotFSM]:
        """Unlink and return the first idle slot, in queue order, whose
        backend is not in `avoid`; the first idle slot of all when every
        one is; None when nothing is idle.  Stale entries ahead of the
        slot that decides the walk are unlinked, as in _ticket_slow;
        idle slots that are passed over stay linked where they are."""
        found: List[Any] = [None, None]     # [first idle, match]

        def visit(fsm: ConnectionSlotFSM, node: Any) -> None:
            if found[1] is not None:
                return
            if not fsm.is_in_state("idle"):
                node.remove()
                fsm.p_idleq_node = None
                return
            if fsm.csf_backend.get("key") not in avoid:
                found[1] = fsm
            elif found[0] is None:
                found[0] = fsm

        self.p_idleq.for_each(visit)
        fsm = found[1] if found[1] is not None else found[0]
        if fsm is not None:
            fsm.p_idleq_node.remove()
            fsm.p_idleq_node = None
        return fsm

    def _ticket_slow(self, handle: ClaimHandle, err_on_empty: bool,
                     avoid: Optional[frozenset] = None) -> None:
        """The full claim-retry logic (lib/pool.js:922-968): invoked on
        every handle return to 'waiting' — directly in pure mode, and
        as the native ClaimTicket's off-hot-path fallback (pool not in
        'running', or the idle queue empty)."""
        if not handle.is_in_state("waiting"):
            return
        # The first try runs on the next loop turn; the pool may have
        # started stopping (or failed) in between — fail now rather
        # than queueing a waiter nothing will ever feed (companion to
        # the stopping-state waiter drain).
        if self.is_in_state("stopping") or self.is_in_state("stopped"):
            handle.fail(mod_errors.PoolStoppingError(self))
            return
        if self.is_in_state("failed"):
            handle.fail(mod_errors.PoolFailedError(
                self, self.p_last_error))
            return
        # Idle connections sitting around?  Take one.  Entries may be
        # stale ('stateChanged' is async): just unlink and skip them;
        # the slot dispatcher copes (lib/pool.js:934-951).
        idleq = self.p_idleq
        lim = self.p_cl_lim
        if lim is not None and self._cl_held():
            # at the concurrency limit: queued as if nothing were idle
            idleq = _NO_IDLE
        elif avoid is not None:
            # a soft preference among the idle slots, nothing more:
            # from here on the claim is like any other
            fsm = self._idle_avoiding(avoid)
            if fsm is not None:
                handle.try_(fsm)
                if lim is not None:
                    self._cl_handoff(handle, fsm)
                self._note_demand()
                return
        while idleq._len > 0:
            fsm = idleq.shift()
            fsm.p_idleq_node = None
            if not fsm.is_in_state("idle"):
                continue
            handle.try_(fsm)
            if lim is not None:
                self._cl_handoff(handle, fsm)
            self._note_demand()
            return

        if err_on_empty and self.p_resolver.count() < 1:
            handle.fail(mod_errors.NoBackendsError(
                self, self.p_resolver.get_last_error()))

        # Keep the node handle so the claim can unlink itself the
        # moment it leaves 'waiting' (timeout/cancel): a sustained
        # overload no longer accumulates dead entries between feeds.
        # (Deliberate divergence: the reference leaves timed-out
        # entries linked until a dequeue walks past them,
        # lib/pool.js:934-951, which grows without bound when claims
        # time out faster than connections free up.)
        if self.p_cq is None:
            handle.ch_waiter_node = self.p_waiters.push(handle)
        elif not self._cq_place(handle):
            return
        self._note_demand()
        self._hwm_counter("max-claim-queue", self.p_waiters._len)
        self._incr_counter("queued-claim")
        self.rebalance()

    def claim(self, options: Any = None, cb: Optional[Callable] = None):
        """Claim a connection: cb(err, handle, connection).

        Returns the ClaimHandle (or a cancel-only stub when the pool is
        stopping/failed, lib/pool.js:889-910).

        Options: ``timeout`` (ms), ``errorOnEmpty``, and
        ``avoidBackends``, an iterable of backend keys: among the idle
        slots the claim prefers one on another backend.  Only a
        preference: it never makes the claim wait, fail or time out.
        On a pool with ``claimQueue`` also ``priority``, the claim's
        class (an integer, 0 served first); a ValueError elsewhere.
        On a pool with ``claimAffinity`` also ``affinityKey`` (bytes or
        str): among the idle slots the claim prefers the backend that
        rendezvous hashing ranks first for the key; likewise only a
        preference, and a ValueError elsewhere.
        """
        # fast path: claim({}, cb) / claim(cb) with no CoDel — the
        # overwhelmingly common call shape on the hot path
        if not options and cb is not None and self.p_codel is None:
            if _native_pool_claim is not None:
                # counter + state check + stack + handle/ticket in C;
                # True means stopping/stopped/failed (counter already
                # bumped): build the short-circuit error here
                h = _native_pool_claim(ClaimHandle, self, cb,
                                       self.p_claim_log, self._loop)
                if h is not True:
                    return h
                if self._fsm_state == "failed":
                    return self._claim_shortcircuit(
                        cb, mod_errors.PoolFailedError(
                            self, self.p_last_error))
                return self._claim_shortcircuit(
                    cb, mod_errors.PoolStoppingError(self))
            err_on_empty = False
            timeout = math.inf
            avoid = None
        else:
            # (a pool whose claim() this is has no claimQueue, so a
            # ``priority`` has been refused in there)
            # (a pool whose claim() this is has no claimAffinity
            # either, so an ``affinityKey`` has been refused as well)
            cb, err_on_empty, avoid, _, timeout, _ = \
                self._claim_options(options, cb)

        counters = self.p_counters
        counters["claim"] = counters.get("claim", 0) + 1

        st = self._fsm_state
        if st == "stopping" or st == "stopped" or \
                st == "stopping.backends":
            return self._claim_shortcircuit(
                cb, mod_errors.PoolStoppingError(self))
        if st == "failed":
            return self._claim_shortcircuit(
                cb, mod_errors.PoolFailedError(self, self.p_last_error))

        stack = mod_utils.maybe_capture_stack_trace()
        # The handle's construction already queues its async
        # stateChanged('waiting'); the ticket receives it on the next
        # loop turn and runs the first try_next then — claim() never
        # fires the callback synchronously (lib/pool.js:922-968).
        if avoid is not None:
            handle = ClaimHandle.fast(self, stack, cb, self.p_claim_log,
                                      timeout, self._loop)
            handle.on("stateChanged",
                      _AvoidClaimTicket(self, handle, err_on_empty, avoid))
            return handle
        if _native_claim_fast is not None:
            return _native_claim_fast(ClaimHandle, self, stack, cb,
                                      self.p_claim_log, timeout,
                                      self._loop, err_on_empty)
        handle = ClaimHandle.fast(self, stack, cb, self.p_claim_log,
                                  timeout, self._loop)
        handle.on("stateChanged", _ClaimTicket(self, handle, err_on_empty))
        return handle

    def _claim_options(self, options: Any, cb: Optional[Callable]) -> tuple:
        """Read and validate the arguments of a claim, for claim() and
        for the claim()s that opted-in pools install on themselves:
        ``(cb, err_on_empty, avoid, priority, timeout, affinity key)``.
        `priority` is the claim's class on a pool with ``claimQueue``
        (its default when the claim names none) and None on any other,
        where naming one is an error.  The affinity key is the bytes of
        the claim's ``affinityKey`` on a pool with ``claimAffinity``,
        None for a claim without one, and likewise an error on any
        other pool."""
        if callable(options) and cb is None:
            cb = options
            options = {}
        options = options or {}
        if cb is None:
            raise TypeError("claim() requires a callback")
        err_on_empty = bool(options.get("errorOnEmpty", False))
        avoid = options.get("avoidBackends")
        if avoid is not None:
            avoid = self._assert_avoid(avoid)
        prio = options.get("priority")
        if prio is not None:
            prio = mod_utils.assert_claim_priority(prio, self.p_cq)
        elif self.p_cq is not None:
            prio = self.p_cq["defaultPriority"]
        akey = options.get("affinityKey")
        if akey is not None:
            akey = mod_utils.assert_affinity_key(akey, self.p_af)

        if self.p_codel is not None:
            if options.get("timeout") is not None:
                raise ValueError("options.timeout not allowed when "
                                 "targetClaimDelay has been set")
            timeout = self.p_codel.get_max_idle()
        elif options.get("timeout") is not None:
            timeout = options["timeout"]
        else:
            timeout = math.inf
        return cb, err_on_empty, avoid, prio, timeout, akey

    def _claim_begin(self, options: Any, cb: Optional[Callable]) -> tuple:
        """What the claim()s of opted-in pools share: the arguments, the
        ``claim`` counter, the short-circuit of a pool that takes no
        claims, and the runtime's handle.  Returns ``(handle, stub,
        err_on_empty, avoid, priority, affinity key)``: a handle that
        still needs its ticket and None, or None and the cancel-only stub of the
        short-circuit, which is then what claim() returns."""
        cb, err_on_empty, avoid, prio, timeout, akey = \
            self._claim_options(options, cb)
        counters = self.p_counters
        counters["claim"] = counters.get("claim", 0) + 1
        st = self._fsm_state
        handle = stub = None
        if st == "stopping" or st == "stopped" or \
                st == "stopping.backends":
            stub = self._claim_shortcircuit(
                cb, mod_errors.PoolStoppingError(self))
        elif st == "failed":
            stub = self._claim_shortcircuit(
                cb, mod_errors.PoolFailedError(self, self.p_last_error))
        else:
            handle = ClaimHandle.fast(
                self, mod_utils.maybe_capture_stack_trace(), cb,
                self.p_claim_log, timeout, self._loop)
        return handle, stub, err_on_empty, avoid, prio, akey

    def _assert_avoid(self, avoid: Any) -> Optional[frozenset]:
        """``avoidBackends``: an iterable of backend keys.  Returns the
        keys this pool knows, or None when that leaves nothing to
        avoid."""
        if isinstance(avoid, (str, bytes)) or isinstance(avoid, Mapping):
            raise TypeError("options.avoidBackends must be an iterable of "
                            "backend keys")
        try:
            keys = list(avoid)
        except TypeError:
            raise TypeError("options.avoidBackends must be an iterable of "
                            "backend keys")
        for k in keys:
            if not isinstance(k, str):
                raise TypeError("options.avoidBackends must hold backend "
                                "keys (strings)")
        known = frozenset(k for k in keys if k in self.p_backends)
        return known or None

    def _claim_shortcircuit(self, cb: Callable, err: BaseException):
        state = {"done": False}

        def fire() -> None:
            if not state["done"]:
                cb(err)
            state["done"] = True

        self._loop.call_soon(fire)
        return _CancelStub(state)

    async def claim_async(self, options: Any = None):
        """Coroutine sugar over claim(): returns (handle, connection)."""
        import asyncio
        fut = self._loop.create_future()

        def cb(err, hdl=None, conn=None):
            if fut.cancelled():
                if hdl is not None:
                    hdl.release()
                return
            if err is not None:
                fut.set_exception(err)
            else:
                fut.set_result((hdl, conn))

        res = self.claim(options or {}, cb)
        try:
            return await fut
        except asyncio.CancelledError:
            res.cancel()
            raise


if _native_pool_claim is not None:
    # claim({}, cb) on a running pool without CoDel enters the native core
    # without a Python frame; every other call shape runs the function
    # above (cueball_amd/_native/speed.cpp, ClaimMethod)
    from ._speed import claim_method as _claim_method
    ConnectionPool.claim = _claim_method(  # type: ignore[assignment]
        ConnectionPool.__dict__["claim"], ClaimHandle)
    from ._speed import _set_cycle_classes
    _set_cycle_classes(None, None, ConnectionPool)
