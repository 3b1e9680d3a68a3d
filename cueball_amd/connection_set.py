"""ConnectionSet: at most one connection per backend, added/removed contract.

Re-design of reference lib/set.js.  Unlike a pool, a Set hands every
connection to the consumer as soon as it is up (for protocols that
multiplex many requests over one connection): it emits ``added(ckey,
conn, handle)`` — which MUST be handled — and later ``removed(ckey,
conn, handle)`` when the connection should be drained; the consumer then
calls ``handle.release()`` (drained cleanly) or ``handle.close()``.

Each connection key is serial-numbered ``<backend-key>.<n>``; a
LogicalConnection FSM tracks one ckey through init -> advertised ->
draining -> stopped (state diagram at lib/set.js:632-675).
"""

from __future__ import annotations

import functools
import math
import random
import time as mod_time
import uuid as mod_uuid
from typing import Any, Dict, List, Optional

from . import utils as mod_utils
from .connection_fsm import ClaimHandle, ConnectionSlotFSM
from .fsm import FSM, StateScope
from .logutil import CueballLogger, default_logger
from .pool import _IntervalTimer
from .pool_monitor import monitor as global_monitor

__all__ = ["ConnectionSet", "LogicalConnection"]


class ConnectionSet(FSM):
    # SRV ranking state: class-level defaults, instance attributes only
    # with srvRanking on (as in ConnectionPool)
    cs_ranks: Optional[Dict[str, tuple]] = None
    cs_active_priority: Optional[int] = None

    # Connection age / recycle() state, class-level for the same
    # reason: a set without maxConnectionAge that never called
    # recycle() has none of these in its instance dict.
    cs_age_max: Optional[float] = None      # maxConnectionAge, ms
    cs_age_spread: Optional[float] = None
    # slot -> [deadline (loop time), "age" | "manual"]; None when off
    cs_age_slots: Optional[Dict[Any, list]] = None
    # the one replacement in flight: {"key", "old", "new", "reason"}
    cs_age_repl: Optional[Dict[str, Any]] = None
    # slots no longer (or never) in cs_fsm that are still closing:
    # swapped-out predecessors and given-up replacements -> backend key
    cs_age_retired: Optional[Dict[Any, str]] = None
    cs_age_timer = None
    cs_age_timer_at: Optional[float] = None

    def __init__(self, options: Dict[str, Any]) -> None:
        if not callable(options.get("constructor")):
            raise TypeError("options.constructor (callable) is required")
        loop_opt = options.get("loop")

        self.cs_uuid = str(mod_uuid.uuid4())
        self.cs_constructor = options["constructor"]

        if options.get("resolver") is None:
            raise TypeError("options.resolver is required")
        self.cs_resolver = options["resolver"]

        recovery = options.get("recovery")
        mod_utils.assert_recovery_set(recovery)
        self.cs_recovery = recovery

        self.cs_conn_handles_err = bool(options.get("connectionHandlesError"))

        log: CueballLogger = options.get("log") or default_logger()
        self.cs_log = log.child(
            component="ConnectionSet",
            domain=options.get("domain"),
            service=options.get("service"),
            cset=self.cs_uuid,
        )
        self.cs_domain = options.get("domain")

        self.cs_collector = mod_utils.create_error_metrics(options)

        target = options.get("target")
        maximum = options.get("maximum")
        if not isinstance(target, int) or not isinstance(maximum, int):
            raise TypeError("options.target and options.maximum are required")
        self.cs_target = target
        self.cs_max = maximum

        self.cs_keys: List[str] = []
        self.cs_backends: Dict[str, Dict[str, Any]] = {}
        self.cs_fsm: Dict[str, ConnectionSlotFSM] = {}
        self.cs_dead: Dict[str, bool] = {}

        # serial numbers generate per-connection keys "key.N"
        self.cs_serials: Dict[str, int] = {}
        self.cs_connections: Dict[str, Any] = {}
        self.cs_connection_keys: Dict[str, List[str]] = {}
        self.cs_lconns: Dict[str, "LogicalConnection"] = {}

        self.cs_last_rebalance: Optional[float] = None
        self.cs_in_rebalance = False
        self.cs_rebal_scheduled = False
        self.cs_counters: Dict[str, int] = {}
        self.cs_last_error: Optional[BaseException] = None

        # SRV ranking (opt-in): key -> (priority, weight) for the
        # rebalance planner; None when off
        srv_ranking = options.get("srvRanking")
        if srv_ranking is None:
            srv_ranking = False
        if not isinstance(srv_ranking, bool):
            raise TypeError("options.srvRanking must be a bool")
        if srv_ranking:
            self.cs_ranks = {}

        # Connection age (opt-in): see the "connection age" section
        # below.  Off means not one attribute is set here.
        age, spread = mod_utils.assert_connection_age(options)
        if age is not None:
            self.cs_age_max = age
            self.cs_age_spread = spread
            self.cs_age_slots = {}
            self.cs_age_retired = {}

        super().__init__("starting", loop=loop_opt)

        self.cs_rebal_timer = _IntervalTimer(self._loop, 10_000)
        shuffle_intvl = options.get("decoherenceInterval")
        if shuffle_intvl is None or shuffle_intvl < 60:
            shuffle_intvl = 60
        self.cs_shuffle_timer = _IntervalTimer(self._loop,
                                               shuffle_intvl * 1000)

    # -- resolver events -------------------------------------------------
    def _on_resolver_added(self, k: str, backend: Dict[str, Any]) -> None:
        backend["key"] = k
        if k in self.cs_keys:
            raise AssertionError("Resolver key is a duplicate")
        idx = random.randrange(len(self.cs_keys) + 1)
        self.cs_keys.insert(idx, k)
        self.cs_backends[k] = backend
        if self.cs_ranks is not None:
            self.cs_ranks[k] = (backend.get("priority", 0),
                                backend.get("weight", 0))
        self.rebalance()

    def _on_resolver_changed(self, k: str, backend: Dict[str, Any]) -> None:
        """A known backend's SRV rank changed (srvRanking only)."""
        if k not in self.cs_backends:
            return
        # update in place: a live slot holds a reference to this dict
        self.cs_backends[k].update(backend)
        self.cs_backends[k]["key"] = k
        self.cs_ranks[k] = (backend.get("priority", 0),
                            backend.get("weight", 0))
        self.rebalance()

    def _subscribe_resolver(self, S: StateScope) -> None:
        S.on(self.cs_resolver, "added", self._on_resolver_added)
        S.on(self.cs_resolver, "removed", self._on_resolver_removed)
        if self.cs_ranks is not None:
            S.on(self.cs_resolver, "changed", self._on_resolver_changed)

    def _on_resolver_removed(self, k: str) -> None:
        try:
            self.cs_keys.remove(k)
        except ValueError:
            raise AssertionError(
                "Resolver removed key that is not present in cs_keys")
        self.cs_backends.pop(k, None)
        self.cs_dead.pop(k, None)
        if self.cs_ranks is not None:
            self.cs_ranks.pop(k, None)

        fsm = self.cs_fsm.get(k)
        if fsm is not None:
            fsm.set_unwanted()
        for ck in list(self.cs_connection_keys.get(k, ())):
            lconn = self.cs_lconns.get(ck)
            if lconn is not None and not lconn.is_in_state("stopped"):
                lconn.drain()
        if self.cs_age_repl is not None:
            self._age_cancel(k)

    def is_declared_dead(self, backend: str) -> bool:
        return self.cs_dead.get(backend) is True

    def should_retry_backend(self, backend: str) -> bool:
        return backend in self.cs_backends

    # -- states -----------------------------------------------------------
    def state_starting(self, S: StateScope) -> None:
        S.valid_transitions(["failed", "running", "stopping"])
        global_monitor.register_set(self)

        self._subscribe_resolver(S)

        if self.cs_resolver.is_in_state("failed"):
            self.cs_log.warn('resolver has already failed, cset will start '
                             'up in "failed" state')
            self.cs_last_error = self.cs_resolver.get_last_error()
            S.goto_state("failed")
            return

        def on_res_state(st: str) -> None:
            if st == "failed":
                self.cs_log.warn('underlying resolver failed, moving cset '
                                 'to "failed" state')
                self.cs_last_error = self.cs_resolver.get_last_error()
                S.goto_state("failed")

        S.on(self.cs_resolver, "stateChanged", on_res_state)

        if self.cs_resolver.is_in_state("running"):
            for k, backend in self.cs_resolver.list().items():
                self._on_resolver_added(k, backend)

        S.on(self, "connectedToBackend", lambda *a: S.goto_state("running"))

        def on_closed_backend(*a: Any) -> None:
            dead = len(self.cs_dead)
            if dead >= len(self.cs_keys):
                self.cs_log.warn('cset has exhausted all retries, now '
                                 'moving to "failed" state', dead=dead)
                S.goto_state("failed")

        S.on(self, "closedBackend", on_closed_backend)
        S.on(self, "stopAsserted", lambda: S.goto_state("stopping"))

    def state_failed(self, S: StateScope) -> None:
        S.valid_transitions(["running", "stopping"])
        self._subscribe_resolver(S)
        S.on(self.cs_shuffle_timer, "timeout", self.reshuffle)

        def on_connected(*a: Any) -> None:
            if self.cs_resolver.is_in_state("failed"):
                raise AssertionError("resolver failed while cset recovering")
            self.cs_log.info("successfully connected to a backend, moving "
                             "back to running state")
            S.goto_state("running")

        S.on(self, "connectedToBackend", on_connected)
        S.on(self, "stopAsserted", lambda: S.goto_state("stopping"))

    def state_running(self, S: StateScope) -> None:
        S.valid_transitions(["failed", "stopping"])
        self._subscribe_resolver(S)
        S.on(self.cs_rebal_timer, "timeout", self.rebalance)
        S.on(self.cs_shuffle_timer, "timeout", self.reshuffle)
        if self.cs_age_slots is not None:
            # whatever came due while the set was not running
            S.immediate(self._age_run)

        def on_closed_backend(*a: Any) -> None:
            dead = len(self.cs_dead)
            if dead >= len(self.cs_keys):
                self.cs_log.warn('cset has exhausted all retries, now '
                                 'moving to "failed" state', dead=dead)
                S.goto_state("failed")

        S.on(self, "closedBackend", on_closed_backend)
        S.on(self, "stopAsserted", lambda: S.goto_state("stopping"))

    def state_stopping(self, S: StateScope) -> None:
        S.valid_transitions(["stopped"])
        self.cs_backends = {}
        fsms = list(self.cs_fsm.values())
        if self.cs_age_slots is not None:
            # a replacement in flight and predecessors still closing
            # are waited for like every other slot
            self._age_stop()
            fsms.extend(self.cs_age_retired)
        remaining = {"n": len(fsms)}

        def one_done() -> None:
            remaining["n"] -= 1
            if remaining["n"] == 0:
                S.goto_state("stopped")

        if not fsms:
            S.goto_state("stopped")
            return

        for fsm in fsms:
            if fsm.is_in_state("stopped") or fsm.is_in_state("failed"):
                one_done()
                continue
            k = fsm.csf_backend["key"]
            cks = list(self.cs_connection_keys.get(k, ()))
            fired = {"done": False}

            def make_cb(f=fired):
                def cb(s: str) -> None:
                    if f["done"]:
                        return
                    if s in ("stopped", "failed"):
                        f["done"] = True
                        one_done()
                return cb

            # Scoped: auto-removed when the set leaves this state (see
            # the matching fix in pool.state_stopping_backends).
            S.on(fsm, "stateChanged", make_cb())
            fsm.set_unwanted()
            for ck in cks:
                # async: avoid FSM loops when .stop() was called from an
                # 'added' handler (lib/set.js:307-318)
                lconn = self.cs_lconns.get(ck)

                def drain_later(lc=lconn):
                    if lc is not None and not lc.is_in_state("stopped"):
                        lc.drain()

                self._loop.call_soon(drain_later)

    def state_stopped(self, S: StateScope) -> None:
        S.valid_transitions([])
        global_monitor.unregister_set(self)
        self.cs_keys = []
        self.cs_fsm = {}
        self.cs_connections = {}
        self.cs_backends = {}
        self.cs_rebal_timer.cancel()
        self.cs_shuffle_timer.cancel()

    # -- public API --------------------------------------------------------
    def reshuffle(self) -> None:
        if len(self.cs_keys) <= 1:
            return
        taken = self.cs_keys.pop()
        idx = random.randrange(len(self.cs_keys) + 1)
        if len(self.cs_keys) > self.cs_target and idx < self.cs_target:
            self.cs_log.info('random shuffle puts backend "%s" at idx %d',
                             taken, idx)
        self.cs_keys.insert(idx, taken)
        self.rebalance()

    def stop(self) -> None:
        self.emit("stopAsserted")

    def set_target(self, target: int) -> None:
        self.cs_target = target
        self.rebalance()

    def get_last_error(self) -> Optional[BaseException]:
        return self.cs_last_error

    def get_connections(self) -> List[Any]:
        """Currently-advertised connections (lib/set.js:613-623 intent;
        the reference's own implementation of this accessor is broken —
        it references fields that don't exist — so this returns what the
        docs promise: connections 'added' and not yet 'removed')."""
        return list(self.cs_connections.values())

    def get_stats(self) -> Dict[str, Any]:
        return {
            "counters": dict(self.cs_counters),
            "totalConnections": len(self.cs_fsm) +
            (0 if self.cs_age_repl is None else 1),
            "connections": len(self.cs_connections),
            "deadBackends": len(self.cs_dead),
        }

    def get_ranking(self) -> Dict[str, Any]:
        """SRV ranking as the set sees it; same shape as
        ``ConnectionPool.get_ranking()``."""
        return mod_utils.ranking_report(
            self.cs_keys, self.cs_dead, self.cs_ranks,
            {k: 1 for k in self.cs_fsm})

    def _note_active_priority(self, new: Optional[int]) -> None:
        old = self.cs_active_priority
        if new == old:
            return
        self.cs_active_priority = new
        if old is None or new is None:
            return  # first backends seen: nothing to fail over from
        self.cs_log.info("failing %s to priority %d"
                         % ("over" if new > old else "back", new))
        self.emit("priorityChanged", old, new)

    # -- rebalancing --------------------------------------------------------
    def rebalance(self) -> None:
        if len(self.cs_keys) < 1:
            return
        if self.is_in_state("stopping") or self.is_in_state("stopped"):
            return
        if self.cs_rebal_scheduled:
            return
        self.cs_rebal_scheduled = True
        self._loop.call_soon(self._rebalance)

    def _rebalance(self) -> None:
        if self.cs_in_rebalance:
            return
        self.cs_in_rebalance = True
        self.cs_rebal_scheduled = False

        conns: Dict[str, List[ConnectionSlotFSM]] = {}
        total = 0
        working = 0
        for k in self.cs_keys:
            conns[k] = []
            fsm = self.cs_fsm.get(k)
            if fsm is not None:
                conns[k].append(fsm)
                if fsm.is_in_state("busy") or fsm.is_in_state("idle"):
                    working += 1
                total += 1

        ranks = self.cs_ranks
        plan = mod_utils.plan_rebalance(conns, self.cs_dead, self.cs_target,
                                        self.cs_max, singleton=True,
                                        ranks=ranks)
        if ranks is not None:
            self._note_active_priority(mod_utils.active_priority(
                self.cs_keys, self.cs_dead, ranks))

        if plan["remove"] or plan["add"]:
            self.cs_log.trace("rebalancing cset, remove %d, add %d "
                              "(target = %d, total = %d)",
                              len(plan["remove"]), len(plan["add"]),
                              self.cs_target, total)

        for fsm in plan["remove"]:
            # Never deliberately remove the last working connection: wait
            # for a replacement to come up first (lib/set.js:417-429).
            if (fsm.is_in_state("busy") or fsm.is_in_state("idle")) and \
                    working <= 1:
                continue
            k = fsm.csf_backend["key"]
            if fsm.is_in_state("busy") or fsm.is_in_state("idle"):
                working -= 1
            fsm.set_unwanted()
            if self.cs_age_repl is not None:
                self._age_cancel(k)
            if fsm.is_in_state("stopped") or fsm.is_in_state("failed"):
                self.cs_fsm.pop(k, None)
                total -= 1
            # drain any advertised connections from this FSM
            for ck in list(self.cs_connection_keys.get(k, ())):
                lconn = self.cs_lconns.get(ck)
                if lconn is not None and not lconn.is_in_state("stopped"):
                    lconn.drain()

        for k in plan["add"]:
            total += 1
            if total > self.cs_max + 1:
                continue
            if k in self.cs_fsm:  # never >1 slot per backend
                continue
            self.add_connection(k)

        self.cs_in_rebalance = False
        self.cs_last_rebalance = mod_time.time()

    def assert_emit(self, event: str, *args: Any) -> bool:
        """emit() that throws if nobody is listening — the added/removed
        contract is mandatory (lib/set.js:471-479)."""
        if self.listener_count(event) < 1:
            raise RuntimeError('Event "%s" on ConnectionSet must be handled'
                               % event)
        return self.emit(event, *args)

    def create_logi_conn(self, key: str,
                         fsm: Optional[ConnectionSlotFSM] = None) -> None:
        """Open the next serial-numbered LogicalConnection on `fsm`, the
        slot it serves: ``cs_fsm[key]`` unless told otherwise (with a
        replacement in flight a backend has two slots)."""
        if fsm is None:
            fsm = self.cs_fsm[key]
        if key not in self.cs_serials:
            self.cs_serials[key] = 1
        self.cs_connection_keys.setdefault(key, [])

        serial = self.cs_serials[key]
        self.cs_serials[key] += 1
        ckey = "%s.%d" % (key, serial)
        self.cs_connection_keys[key].append(ckey)

        lconn = LogicalConnection({
            "set": self,
            "log": self.cs_log,
            "key": key,
            "ckey": ckey,
            "fsm": fsm,
            "loop": self._loop,
        })
        self.cs_lconns[ckey] = lconn

        def on_lconn_state(st: str) -> None:
            if st == "advertised":
                # the successor has been 'added': now, and only now,
                # its predecessor may go
                repl = self.cs_age_repl
                if repl is not None and repl["new"] is fsm and \
                        lconn.is_in_state("advertised"):
                    self._age_swap()
                return
            if st != "stopped":
                return
            self.cs_lconns.pop(ckey, None)
            cks = self.cs_connection_keys.get(key, [])
            if ckey in cks:
                cks.remove(ckey)
            # Chain the next serial if this slot will contribute another
            # connection (lib/set.js:514-533).
            if key not in self.cs_backends:
                return
            if fsm.is_in_state("failed") or fsm.is_in_state("stopped"):
                return
            if not fsm.csf_wanted:
                # an unwanted slot never offers itself again: a
                # LogicalConnection chained here would sit in init
                # for good
                return
            repl = self.cs_age_repl
            if repl is not None and repl["old"] is fsm:
                # the predecessor went away by itself (socket death or
                # hdl.close()) before its replacement was up: the
                # replacement takes over, nothing more is chained here
                self._age_swap()
                return
            self.create_logi_conn(key, fsm)

        lconn.on("stateChanged", on_lconn_state)

    def add_connection(self, key: str) -> None:
        if self.is_in_state("stopping") or self.is_in_state("stopped"):
            return

        fsm = self._make_slot(key, self.cs_dead.get(key) is True)
        if key in self.cs_fsm:
            raise AssertionError("slot for %s already exists" % key)
        self.cs_fsm[key] = fsm
        self._start_slot(key, fsm)

    def _make_slot(self, key: str, monitor: bool) -> ConnectionSlotFSM:
        backend = self.cs_backends[key]
        backend["key"] = key
        return ConnectionSlotFSM({
            "constructor": self.cs_constructor,
            "backend": backend,
            "log": self.cs_log,
            "pool": self,
            "recovery": self.cs_recovery,
            "monitor": monitor,
            "loop": self._loop,
        })

    def _start_slot(self, key: str, fsm: ConnectionSlotFSM) -> None:
        if self.cs_age_slots is not None:
            self._age_watch(fsm)
        self.create_logi_conn(key, fsm)

        # rebalance when a slot reaches idle or leaves it — those are the
        # points where the plan can meaningfully change (lib/set.js:559-565)
        was_idle = {"v": False}

        def on_slot_state(new_state: str) -> None:
            # Only the slot that is cs_fsm[key] does the bookkeeping
            # below; a replacement in flight or a swapped-out
            # predecessor is the age section's business.
            if self.cs_age_slots is not None and \
                    self._age_slot_state(key, fsm, new_state):
                return
            if new_state == "idle":
                self.emit("connectedToBackend", key, fsm)
                if key in self.cs_dead:
                    del self.cs_dead[key]
                self.rebalance()
                was_idle["v"] = True
                return

            if was_idle["v"]:
                was_idle["v"] = False
                self.rebalance()

            if new_state == "failed":
                if key in self.cs_backends:
                    self.cs_dead[key] = True
                    err = fsm.get_socket_mgr().get_last_error()
                    if err is not None:
                        self.cs_last_error = err

            if new_state in ("stopped", "failed"):
                self.cs_fsm.pop(key, None)
                self.emit("closedBackend", fsm)
                self.rebalance()

        fsm.on("stateChanged", on_slot_state)
        fsm.start()

    # -- connection age / recycle() ------------------------------------------
    #
    # Every connected socket may carry a deadline: its connect time plus
    # a lifetime drawn once per socket (maxConnectionAge), or "now"
    # (recycle()).  One call_at timer waits for the earliest deadline
    # still ahead; everything else is driven by events the set sees
    # anyway.  Unlike the pool, which closes an idle socket and lets the
    # rebalance open another, a set replaces make-before-break: a second
    # slot for the same backend is opened apart from cs_fsm (the
    # rebalance planner never sees it), and only once its connection has
    # been 'added' does it become cs_fsm[key] while the predecessor is
    # drained and made unwanted.  One replacement at a time per set.

    def _age_watch(self, fsm: ConnectionSlotFSM) -> None:
        fsm.csf_smgr.on("stateChanged",
                        functools.partial(self._age_smgr_changed, fsm))

    def _age_draw(self, since: float) -> list:
        life = self.cs_age_max * (1.0 - self.cs_age_spread * random.random())
        return [since + life / 1000.0, "age"]

    def _age_smgr_changed(self, fsm: ConnectionSlotFSM, st: str) -> None:
        if st == "connected":
            smgr = fsm.csf_smgr
            if smgr.is_in_state("connected") and fsm.csf_wanted:
                if self.cs_age_max is not None:
                    self.cs_age_slots[fsm] = self._age_draw(
                        smgr.sm_connected_at)
                else:
                    # a new socket: a recycle() mark was for the old one
                    self.cs_age_slots.pop(fsm, None)
            self._loop.call_soon(self._age_run)
        elif st == "error" or st == "closed":
            self.cs_age_slots.pop(fsm, None)
            repl = self.cs_age_repl
            if repl is not None and repl["old"] is fsm:
                # the predecessor's socket died under its replacement
                self._age_swap()

    def _age_lconns(self,
                    fsm: ConnectionSlotFSM) -> List["LogicalConnection"]:
        """The live LogicalConnections that serve this very slot."""
        out = []
        for ck in self.cs_connection_keys.get(fsm.csf_backend["key"], ()):
            lconn = self.cs_lconns.get(ck)
            if lconn is not None and lconn.lc_fsm is fsm and \
                    not lconn.is_in_state("stopped"):
                out.append(lconn)
        return out

    def _age_advertised(self, fsm: ConnectionSlotFSM) -> Optional[str]:
        """The ckey under which this slot's socket is advertised now:
        'added' has been emitted, 'removed' has not, and the consumer
        still holds the handle."""
        for lconn in self._age_lconns(fsm):
            if lconn.is_in_state("advertised") and \
                    lconn.lc_hdl.is_in_state("claimed"):
                return lconn.lc_ckey
        return None

    def _age_slot_state(self, key: str, fsm: ConnectionSlotFSM,
                        st: str) -> bool:
        """A slot changed state.  True if it is not the backend's slot
        of record, so that the caller leaves cs_dead, cs_fsm and the
        backend events alone."""
        gone = st == "stopped" or st == "failed"
        if gone:
            self.cs_age_slots.pop(fsm, None)
        repl = self.cs_age_repl
        if gone and repl is not None and repl["old"] is fsm:
            self._age_swap()
            repl = None
        if self.cs_fsm.get(key) is fsm:
            return False
        if repl is not None and repl["new"] is fsm:
            if st == "failed":
                self._age_failed()
            return True
        if gone:
            self.cs_age_retired.pop(fsm, None)
            self.rebalance()
        return True

    def _age_timer_fired(self) -> None:
        at = self.cs_age_timer_at
        self.cs_age_timer = None
        self.cs_age_timer_at = None
        # a loop may fire a timer a clock tick early
        self._age_run(max(self._loop.time(), at))

    def _age_run(self, now: Optional[float] = None) -> None:
        """Start replacing what is due, oldest deadline first and one at
        a time.  Then re-arm the timer."""
        st = self._fsm_state
        if st == "stopping" or st == "stopped":
            return
        if now is None:
            now = self._loop.time()
        slots = self.cs_age_slots
        # only a running set starts a replacement; entering running
        # brings us back here
        if st == "running" and self.cs_age_repl is None:
            due = [(ent[0], i, fsm) for i, (fsm, ent) in
                   enumerate(slots.items()) if ent[0] <= now]
            due.sort()
            for _, _, fsm in due:
                key = fsm.csf_backend["key"]
                # due means advertised: anything else is on its way
                # somewhere, and the event that ends it brings us back
                if self.cs_fsm.get(key) is fsm and fsm.csf_wanted and \
                        key in self.cs_backends and \
                        self._age_advertised(fsm) is not None:
                    self._age_replace(key, fsm)
                    break
        nxt: Optional[float] = None
        for ent in slots.values():
            if ent[0] > now and (nxt is None or ent[0] < nxt):
                nxt = ent[0]
        if nxt != self.cs_age_timer_at:
            if self.cs_age_timer is not None:
                self.cs_age_timer.cancel()
                self.cs_age_timer = None
            if nxt is not None:
                self.cs_age_timer = self._loop.call_at(
                    nxt, self._age_timer_fired)
            self.cs_age_timer_at = nxt

    def _age_replace(self, key: str, old: ConnectionSlotFSM) -> None:
        """Open the replacement slot for `old`, apart from cs_fsm."""
        reason = self.cs_age_slots.pop(old)[1]
        new = self._make_slot(key, False)
        self.cs_age_repl = {"key": key, "old": old, "new": new,
                            "reason": reason}
        self._start_slot(key, new)

    def _age_swap(self) -> None:
        """The replacement becomes the backend's slot and its
        predecessor goes: either the successor has just been 'added',
        or the predecessor went away by itself."""
        repl = self.cs_age_repl
        self.cs_age_repl = None
        key, old, new, reason = (repl["key"], repl["old"], repl["new"],
                                 repl["reason"])
        self.cs_fsm[key] = new
        if not (old.is_in_state("stopped") or old.is_in_state("failed")):
            self.cs_age_retired[old] = key
        self.emit("connectionRecycled", key, reason)
        self._incr_counter("recycled-" + reason)
        for lconn in self._age_lconns(old):
            lconn.drain()
        old.set_unwanted()
        now = self._loop.time()
        at = old.csf_smgr.sm_connected_at
        old.csf_log.info(
            'recycling connection to backend "%s" (%s) at age %d ms',
            key, reason, round((now - at) * 1000.0) if at is not None else 0)
        self.rebalance()
        self._loop.call_soon(self._age_run)

    def _age_failed(self) -> None:
        """The replacement ran out of retries.  Its predecessor is alive
        and advertised, so the backend is not dead: keep what we have."""
        repl = self.cs_age_repl
        self.cs_age_repl = None
        key, old, reason = repl["key"], repl["old"], repl["reason"]
        self._incr_counter("recycle-failed")
        if reason == "age" and self.cs_age_max is not None and \
                old.csf_smgr.is_in_state("connected"):
            self.cs_age_slots[old] = self._age_draw(self._loop.time())
        self.cs_log.warn('could not replace connection to backend "%s" '
                         '(%s), keeping the old one' % (key, reason))
        self.emit("connectionRecycleFailed", key, reason)
        self._loop.call_soon(self._age_run)

    def _age_cancel(self, key: Optional[str] = None) -> None:
        """Give up the replacement in flight (for backend `key` only,
        if given): its backend is leaving the set."""
        repl = self.cs_age_repl
        if repl is None or (key is not None and repl["key"] != key):
            return
        self.cs_age_repl = None
        new = repl["new"]
        if not (new.is_in_state("stopped") or new.is_in_state("failed")):
            self.cs_age_retired[new] = repl["key"]
        new.set_unwanted()
        for lconn in self._age_lconns(new):
            lconn.drain()
        self._loop.call_soon(self._age_run)

    def _age_stop(self) -> None:
        self._age_cancel()
        self.cs_age_slots.clear()
        if self.cs_age_timer is not None:
            self.cs_age_timer.cancel()
            self.cs_age_timer = None
            self.cs_age_timer_at = None

    def recycle(self) -> int:
        """Treat every socket that is connected and advertised right now
        as expired: each is replaced make-before-break, one at a time.
        Connections opened later are unaffected.  Returns the number of
        connections marked (0 once the set is stopping, stopped or
        failed)."""
        if self._fsm_state not in ("starting", "running"):
            return 0
        if self.cs_age_slots is None:
            self.cs_age_slots = {}
            self.cs_age_retired = {}
            for fsm in self.cs_fsm.values():
                self._age_watch(fsm)
        now = self._loop.time()
        repl = self.cs_age_repl
        marked = 0
        for fsm in self.cs_fsm.values():
            if (repl is not None and repl["old"] is fsm) or \
                    not fsm.csf_wanted or \
                    fsm.csf_smgr._fsm_state != "connected" or \
                    self._age_advertised(fsm) is None:
                continue
            ent = self.cs_age_slots.get(fsm)
            if ent is not None and ent[1] == "manual":
                continue
            at = now if ent is None or ent[0] > now else ent[0]
            self.cs_age_slots[fsm] = [at, "manual"]
            marked += 1
        self._age_run(now)
        return marked

    def get_connection_ages(self) -> Dict[str, Any]:
        """``{"maxAgeMs", "oldestMs", "connections": [{"backend",
        "ckey", "state", "ageMs", "expiresInMs", "recycling"}, ...]}``;
        ages and expiries are None for a slot without a connected
        socket, ``expiresInMs`` also for a socket without a deadline,
        ``ckey`` for a socket that is not advertised.  A replacement in
        flight is listed after its predecessor, which is ``recycling``
        from the moment the replacement is created until its socket is
        closed."""
        now = self._loop.time()
        slots = self.cs_age_slots or {}
        repl = self.cs_age_repl
        listed = [(k, fsm, repl is not None and repl["old"] is fsm)
                  for k, fsm in self.cs_fsm.items()]
        if repl is not None:
            listed.append((repl["key"], repl["new"], False))
        for fsm, k in (self.cs_age_retired or {}).items():
            listed.append((k, fsm, True))
        out = []
        oldest: Optional[float] = None
        for k, fsm, recycling in listed:
            smgr = fsm.csf_smgr
            age = expires = None
            if smgr._fsm_state == "connected":
                age = (now - smgr.sm_connected_at) * 1000.0
                if oldest is None or age > oldest:
                    oldest = age
                ent = slots.get(fsm)
                if ent is not None:
                    expires = max(0.0, (ent[0] - now) * 1000.0)
            out.append({"backend": k, "ckey": self._age_advertised(fsm),
                        "state": fsm.get_state(), "ageMs": age,
                        "expiresInMs": expires, "recycling": recycling})
        return {"maxAgeMs": self.cs_age_max, "oldestMs": oldest,
                "connections": out}

    def _incr_counter(self, counter: str) -> None:
        mod_utils.update_error_metrics(self.cs_collector, self.cs_uuid,
                                       counter)
        self.cs_counters[counter] = self.cs_counters.get(counter, 0) + 1


class LogicalConnection(FSM):
    """Tracks one connection key through its advertised lifetime
    (lib/set.js:632-820): init -> advertised -> draining -> stopped.
    """

    def __init__(self, options: Dict[str, Any]) -> None:
        self.lc_set: ConnectionSet = options["set"]
        self.lc_key: str = options["key"]
        self.lc_fsm: ConnectionSlotFSM = options["fsm"]
        self.lc_smgr = options["fsm"].get_socket_mgr()
        self.lc_conn: Any = None
        self.lc_ckey: str = options["ckey"]
        self.lc_hdl: Optional[ClaimHandle] = None
        self.lc_log: CueballLogger = options["log"]
        super().__init__("init", loop=options.get("loop"))

    def drain(self) -> None:
        if self.is_in_state("stopped"):
            raise AssertionError("drain() on stopped LogicalConnection")
        self.emit("drainAsserted")

    def state_init(self, S: StateScope) -> None:
        S.valid_transitions(["advertised", "stopped"])

        def on_claimed(err, hdl=None, conn=None):
            if err is not None:
                raise AssertionError("cset claim handle failed: %r" % err)
            if hdl is not self.lc_hdl:
                raise AssertionError("claimed foreign handle")
            self.lc_conn = conn
            S.goto_state("advertised")

        self.lc_hdl = ClaimHandle({
            "pool": self.lc_set,
            "claimStack": ["claim", "ConnectionSet.add_connection",
                           "ConnectionSet.add_connection"],
            "callback": S.callback(on_claimed),
            "log": self.lc_log,
            "throwError": not self.lc_set.cs_conn_handles_err,
            "claimTimeout": math.inf,
            "loop": self._loop,
        })

        # Keep trying the slot until we get a claim; multiple attempts in
        # this state are fine — 'added' has not been emitted yet.
        def on_hdl_state(st: str) -> None:
            if st == "waiting" and self.lc_hdl.is_in_state("waiting"):
                if self.lc_fsm.is_in_state("idle"):
                    self.lc_hdl.try_(self.lc_fsm)
            elif st in ("failed", "cancelled"):
                S.goto_state("stopped")

        S.on(self.lc_hdl, "stateChanged", on_hdl_state)

        def on_fsm_state(st: str) -> None:
            if st == "idle" and self.lc_fsm.is_in_state("idle"):
                if self.lc_hdl.is_in_state("waiting"):
                    self.lc_hdl.try_(self.lc_fsm)
            elif st == "failed":
                S.goto_state("stopped")

        S.on(self.lc_fsm, "stateChanged", on_fsm_state)

        # drain before advertising: go straight to stopped
        S.on(self, "drainAsserted", lambda: S.goto_state("stopped"))

    def state_advertised(self, S: StateScope) -> None:
        S.valid_transitions(["draining", "stopped"])

        def on_hdl_state(st: str) -> None:
            # user may .close() at any time, but .release() only after
            # 'removed' has been emitted (docs/api.adoc; lib/set.js:760-773)
            if st == "closed":
                S.goto_state("stopped")
            if st == "released":
                raise RuntimeError(
                    "The .release() method may not be called on a "
                    'ConnectionSet handle before "removed" has been emitted')

        S.on(self.lc_hdl, "stateChanged", on_hdl_state)

        def on_smgr_state(st: str) -> None:
            if st != "connected":
                S.goto_state("draining")

        S.on(self.lc_smgr, "stateChanged", on_smgr_state)
        S.on(self, "drainAsserted", lambda: S.goto_state("draining"))

        self.lc_set.cs_connections[self.lc_ckey] = self.lc_conn
        self.lc_set.assert_emit("added", self.lc_ckey, self.lc_conn,
                                self.lc_hdl)

    def state_draining(self, S: StateScope) -> None:
        S.valid_transitions(["stopped"])
        self.lc_set.cs_connections.pop(self.lc_ckey, None)

        hdl = self.lc_hdl
        if not hdl.is_in_state("claimed"):
            # Divergence from the reference (bug fix, property suite):
            # the user already relinquished the handle (e.g. close()
            # racing the socket's own death event, both pending in the
            # same spin).  Emitting 'removed' now would hand the
            # consumer a dead handle whose release() throws
            # (lib/set.js:792-811 emits unconditionally).  The
            # connection is already gone: stop directly.
            S.goto_state("stopped")
            return

        def on_hdl_state(st: str) -> None:
            if st in ("closed", "released", "cancelled"):
                S.goto_state("stopped")

        S.on(hdl, "stateChanged", on_hdl_state)
        self.lc_set.assert_emit("removed", self.lc_ckey, self.lc_conn,
                                hdl)

    def state_stopped(self, S: StateScope) -> None:
        S.valid_transitions([])
        self.lc_set.cs_connections.pop(self.lc_ckey, None)
        if self.lc_hdl is not None and (
                self.lc_hdl.is_in_state("waiting")
                or self.lc_hdl.is_in_state("claiming")):
            self.lc_hdl.cancel()
