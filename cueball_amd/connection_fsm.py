"""Connection slot management: SocketMgrFSM, ClaimHandle, ConnectionSlotFSM.

This is the guts of connection management (reference
lib/connection-fsm.js).  Three cooperating Moore machines:

- **SocketMgrFSM** — owns the actual connection object produced by the
  user-supplied ``constructor(backend)``; handles connect timeouts,
  error/close de-duplication, exponential backoff with jitter, and
  "monitor mode" (infinite retries at max backoff, watching a dead
  backend; lib/connection-fsm.js:68-420).
  States: init -> connecting -> connected -> {error, closed} -> backoff
  -> {connecting, failed}.

- **ClaimHandle** — the object handed to pool users; encapsulates the
  claim double-handshake (try -> claim -> accept/reject), the claim
  timeout, cancellation, and the event-listener leak detector
  (lib/connection-fsm.js:422-808).
  States: waiting -> claiming -> claimed -> {released, closed}, plus
  cancelled and failed.

- **ConnectionSlotFSM** — one per pool/set slot; drives the SocketMgr,
  decides when to retry or give up, and reports only the transitions the
  Pool/Set cares about (lib/connection-fsm.js:810-1242).
  States: init -> connecting -> {failed, retrying, idle} ;
  idle <-> busy ; killing/stopping/stopped.

The user Connection interface is the reference's contract
(docs/api.adoc:580-645): an EventEmitter emitting ``connect``, ``close``,
``error`` (and optionally ``timeout``/``connectError``/``connectTimeout``)
with a ``destroy()`` method and optional ``set_unwanted()``/``ref()``/
``unref()``.
"""

from __future__ import annotations

import math
from typing import Any, Callable, Dict, List, Optional

from . import errors as mod_errors
from . import utils as mod_utils
from .events import EventEmitter
from .fsm import FSM, FSMError, StateScope
from .logutil import CueballLogger

__all__ = ["SocketMgrFSM", "ClaimHandle", "ConnectionSlotFSM"]

try:
    import os as _os
    if _os.environ.get("CUEBALL_PURE"):
        _native_count = None
        _SlotKit = None
        _SlotFSMBase = FSM
    else:
        from ._speed import count_listeners as _native_count
        from ._speed import SlotKit as _SlotKit
        # the slot fields of the claim cycle (csf_handle,
        # csf_prev_handle, csf_wanted, csf_monitor, p_idleq_node,
        # p_initq_node) are members of this native FSM subtype; the
        # pure runtime keeps them as plain attributes
        from ._speed import SlotBase as _SlotFSMBase
except ImportError:
    _native_count = None
    _SlotKit = None
    _SlotFSMBase = FSM


def _call_optional(obj: Any, *names: str) -> None:
    for name in names:
        fn = getattr(obj, name, None)
        if callable(fn):
            fn()
            return


class SocketMgrFSM(FSM):
    """Socket lifecycle + retry/backoff engine (1:1 with a slot FSM)."""

    #: loop time at which the current socket entered 'connected' (the
    #: start of its age; see ConnectionPool maxConnectionAge)
    sm_connected_at: Optional[float] = None

    def __init__(self, options: Dict[str, Any]) -> None:
        recovery = options["recovery"]
        connect_recov = recovery["default"]
        initial_recov = recovery["default"]
        if recovery.get("connect") is not None:
            initial_recov = recovery["connect"]
            connect_recov = recovery["connect"]
        if recovery.get("initial") is not None:
            initial_recov = recovery["initial"]
        mod_utils.assert_recovery(connect_recov, "recovery.connect")
        mod_utils.assert_recovery(initial_recov, "recovery.initial")

        self.sm_initial_recov = initial_recov
        self.sm_connect_recov = connect_recov
        self.sm_pool = options["pool"]
        self.sm_backend = options["backend"]
        self.sm_constructor = options["constructor"]
        self.sm_slot = options["slot"]
        log: CueballLogger = options["log"]
        self.sm_log = log.child(
            component="SocketMgrFSM",
            backend=self.sm_backend.get("key"),
            address=self.sm_backend.get("address"),
            port=self.sm_backend.get("port"),
        )
        self.sm_last_error: Optional[BaseException] = None
        self.sm_socket: Optional[EventEmitter] = None
        self.sm_monitor: Optional[bool] = None
        # backoff bookkeeping, filled by reset_backoff()
        self.sm_retries = 0.0
        self.sm_retries_left = 0.0
        self.sm_min_delay = 0.0
        self.sm_delay = 0.0
        self.sm_max_delay = math.inf
        self.sm_timeout = 0.0
        self.sm_max_timeout = math.inf
        self.sm_delay_spread = 0.2

        super().__init__("init", loop=options.get("loop"))
        self.set_monitor(bool(options["monitor"]))

    # -- monitor mode / backoff ---------------------------------------
    def set_monitor(self, value: bool) -> None:
        """In monitor mode: infinite retries, delay/timeout pinned at max
        (lib/connection-fsm.js:175-208)."""
        if not (self.is_in_state("init") or self.is_in_state("connected")):
            raise FSMError("set_monitor only valid in init/connected")
        if value == self.sm_monitor:
            return
        self.sm_monitor = value
        self.reset_backoff()

    def reset_backoff(self) -> None:
        recov = self.sm_initial_recov
        self.sm_retries = recov["retries"]
        self.sm_retries_left = recov["retries"]
        self.sm_min_delay = recov["delay"]
        self.sm_delay = recov["delay"]
        self.sm_max_delay = recov.get("maxDelay") or math.inf
        self.sm_timeout = recov["timeout"]
        self.sm_max_timeout = recov.get("maxTimeout") or math.inf
        # Default only when absent: an explicit delaySpread of 0.0 is a
        # deliberate "no spread" setting and must be preserved
        # (reference defaults only on undefined).
        spread = recov.get("delaySpread")
        self.sm_delay_spread = 0.2 if spread is None else spread

        if self.sm_monitor is True:
            mult = 1 << int(self.sm_retries)
            self.sm_delay = self.sm_max_delay
            if not math.isfinite(self.sm_delay):
                self.sm_delay = recov["delay"] * mult
            self.sm_timeout = self.sm_max_timeout
            if not math.isfinite(self.sm_timeout):
                self.sm_timeout = recov["timeout"] * mult
            # keep retrying a failed backend forever
            self.sm_retries = math.inf
            self.sm_retries_left = math.inf

    def set_unwanted(self) -> None:
        """Forward to the connection if it supports it (advisory only;
        lib/connection-fsm.js:210-221)."""
        if self.sm_socket is not None:
            _call_optional(self.sm_socket, "set_unwanted", "setUnwanted")

    # -- signal functions ---------------------------------------------
    def connect(self) -> None:
        if not (self.is_in_state("init") or self.is_in_state("closed")):
            raise FSMError('SocketMgrFSM.connect only in "init"/"closed" '
                           '(is in "%s")' % self.get_state())
        self.emit("connectAsserted")

    def retry(self) -> None:
        if not (self.is_in_state("closed") or self.is_in_state("error")):
            raise FSMError('SocketMgrFSM.retry only in "closed"/"error" '
                           '(is in "%s")' % self.get_state())
        self.emit("retryAsserted")

    def close(self) -> None:
        if not (self.is_in_state("connected") or self.is_in_state("backoff")):
            raise FSMError('SocketMgrFSM.close only in "connected"/"backoff" '
                           '(is in "%s")' % self.get_state())
        self.emit("closeAsserted")

    def get_last_error(self) -> Optional[BaseException]:
        return self.sm_last_error

    def get_socket(self) -> Any:
        if not self.is_in_state("connected"):
            raise FSMError("get_socket only in connected state")
        return self.sm_socket

    # -- states --------------------------------------------------------
    def state_init(self, S: StateScope) -> None:
        S.valid_transitions(["connecting"])
        S.on(self, "connectAsserted", lambda: S.goto_state("connecting"))

    def state_connecting(self, S: StateScope) -> None:
        S.valid_transitions(["connected", "error"])
        # connect latency: this entry -> the socket's 'connect' event,
        # successful connects only (a pool without latencyStats, or a
        # ConnectionSet, has no p_lat)
        lat = getattr(self.sm_pool, "p_lat", None)
        started = self._loop.time() if lat is not None else 0.0

        def on_timeout() -> None:
            self.sm_last_error = mod_errors.ConnectionTimeoutError(
                self.sm_backend)
            S.goto_state("error")
            self.sm_pool._incr_counter("timeout-during-connect")

        S.timeout(self.sm_timeout, on_timeout)

        self.sm_log.trace("calling constructor to open new connection")
        sock = self.sm_constructor(self.sm_backend)
        if sock is None:
            raise TypeError("connection constructor returned None")
        self.sm_socket = sock
        sock.sm_fsm = self

        def on_connect() -> None:
            if lat is not None:
                lat.connect.record((self._loop.time() - started) * 1000.0)
            S.goto_state("connected")

        S.on(sock, "connect", on_connect)

        def on_error(err: BaseException) -> None:
            self.sm_last_error = mod_errors.ConnectionError_(
                self.sm_backend, "error", "connect", err)
            S.goto_state("error")
            self.sm_log.trace("emitted error while connecting")
            self.sm_pool._incr_counter("error-during-connect")

        on_error._cueball_internal = True  # type: ignore[attr-defined]
        S.on(sock, "error", on_error)

        def on_connect_error(err: BaseException) -> None:
            self.sm_last_error = mod_errors.ConnectionError_(
                self.sm_backend, "connectError", "connect", err)
            S.goto_state("error")
            self.sm_log.trace("emitted connectError while connecting")
            self.sm_pool._incr_counter("error-during-connect")

        S.on(sock, "connectError", on_connect_error)

        def on_close() -> None:
            self.sm_last_error = mod_errors.ConnectionClosedError(
                self.sm_backend)
            S.goto_state("error")
            self.sm_log.trace("closed while connecting")
            self.sm_pool._incr_counter("close-during-connect")

        S.on(sock, "close", on_close)

        def on_sock_timeout() -> None:
            self.sm_last_error = mod_errors.ConnectionTimeoutError(
                self.sm_backend)
            S.goto_state("error")
            self.sm_log.trace("timed out while connecting")
            self.sm_pool._incr_counter("timeout-during-connect")

        S.on(sock, "timeout", on_sock_timeout)
        S.on(sock, "connectTimeout", on_sock_timeout)

    def state_connected(self, S: StateScope) -> None:
        S.valid_transitions(["error", "closed"])
        sock = self.sm_socket
        self.sm_log.trace("connected")
        self.sm_connected_at = self._loop.time()
        self.reset_backoff()

        def on_error(err: BaseException) -> None:
            self.sm_last_error = mod_errors.ConnectionError_(
                self.sm_backend, "error", "operation", err)
            S.goto_state("error")
            self.sm_pool._incr_counter("error-while-connected")
            self.sm_log.trace("emitted error while connected")

        on_error._cueball_internal = True  # type: ignore[attr-defined]
        S.on(sock, "error", on_error)
        S.on(sock, "close", lambda: S.goto_state("closed"))
        S.on(self, "closeAsserted", lambda: S.goto_state("closed"))

    def state_error(self, S: StateScope) -> None:
        S.valid_transitions(["backoff"])
        if self.sm_socket is not None:
            self.sm_socket.destroy()
        self.sm_socket = None
        S.on(self, "retryAsserted", lambda: S.goto_state("backoff"))

    def state_backoff(self, S: StateScope) -> None:
        S.valid_transitions(["failed", "connecting", "closed"])

        # NB: "retries" means "attempts" in the cueball API, so compare
        # to 1 rather than 0 (lib/connection-fsm.js:364-372).
        if self.sm_retries_left != math.inf and self.sm_retries_left <= 1:
            S.goto_state("failed")
            return

        delay = mod_utils.gen_delay(self.sm_delay, self.sm_delay_spread)

        if self.sm_retries != math.inf:
            self.sm_retries_left -= 1
            self.sm_delay *= 2
            self.sm_timeout *= 2
            if self.sm_timeout > self.sm_max_timeout:
                self.sm_timeout = self.sm_max_timeout
            if self.sm_delay > self.sm_max_delay:
                self.sm_delay = self.sm_max_delay

        S.timeout(delay, lambda: S.goto_state("connecting"))
        S.on(self, "closeAsserted", lambda: S.goto_state("closed"))

    def state_closed(self, S: StateScope) -> None:
        S.valid_transitions(["backoff", "connecting"])
        if self.sm_socket is not None:
            self.sm_socket.destroy()
        self.sm_socket = None
        self.sm_log.trace("connection closed")
        S.on(self, "retryAsserted", lambda: S.goto_state("backoff"))
        S.on(self, "connectAsserted", lambda: S.goto_state("connecting"))

    def state_failed(self, S: StateScope) -> None:
        S.valid_transitions([])
        self.sm_log.warn("failed to connect to backend, retries exhausted")
        self.sm_pool._incr_counter("retries-exhausted")


def _report_failure(handle: Any, err: Optional[BaseException]) -> None:
    """ClaimHandle.report_failure(), shared by both claim handles: the
    claimer judged this lease failed at protocol level (say an HTTP 503
    on a healthy socket).  Only a mark on the handle; the pool's outlier
    detection reads it when the lease has ended."""
    if handle._fsm_state != "claimed":
        raise mod_errors.CueballError(
            'ClaimHandle.report_failure() called while in state "%s"'
            % handle.get_state())
    handle.ch_failure_reported = True
    if err is not None:
        handle.ch_log.debug("claimer reported the lease as failed: %r", err)


def _handle_backend(handle: Any) -> Optional[Dict[str, Any]]:
    """ClaimHandle.get_backend(), shared by both claim handles: the
    backend dict of the slot the handle holds a lease on, None when it
    holds none (not claimed yet, or released, closed, cancelled or
    failed since)."""
    slot = handle.ch_slot
    if slot is None or handle._fsm_state != "claimed":
        return None
    return slot.get_backend()


class ClaimHandle(FSM):
    """Handle given to pool users; drives the claim double-handshake.

    Reference: CueBallClaimHandle, lib/connection-fsm.js:422-784.
    """

    # events a connection claimer may leak handlers for
    _LEAK_EVENTS = ("close", "error", "readable", "data")

    # hot-path: immutable defaults live on the class; instances only
    # write them when they change (a claim creates one handle, so every
    # skipped dict store counts)
    ch_slot: Optional["ConnectionSlotFSM"] = None
    ch_release_stack: Optional[List[str]] = None
    ch_connection: Any = None
    ch_cancelled = False
    ch_last_error: Optional[BaseException] = None
    ch_do_release_leak_check = True
    ch_pinger = False
    ch_pre_listeners: Any = None
    #: claim time of a handle whose wait was recorded (None otherwise)
    ch_claimed_at: Optional[float] = None
    #: set by report_failure(): the lease counts as failed for the
    #: pool's outlier detection, however it ends
    ch_failure_reported = False

    def __init__(self, options: Dict[str, Any]) -> None:
        self.ch_claim_timeout = options["claimTimeout"]
        self.ch_pool = options["pool"]
        throw_error = options.get("throwError")
        self.ch_throw_error = True if throw_error is None else bool(throw_error)
        self.ch_claim_stack: List[str] = options["claimStack"]
        self.ch_callback: Callable = options["callback"]
        log: CueballLogger = options["log"]
        # hot path: the pool passes a pre-made child logger
        self.ch_log = log if options.get("_logReady") \
            else log.child(component="ClaimHandle")

        self.ch_lat = getattr(self.ch_pool, "p_lat", None)

        super().__init__("waiting", loop=options.get("loop"))
        self.ch_started = self._loop.time() * 1000.0

    @classmethod
    def fast(cls, pool: Any, claim_stack: List[str], callback: Callable,
             log: CueballLogger, claim_timeout: float,
             loop: Any) -> "ClaimHandle":
        """Positional constructor for the claim hot path (skips the
        options-dict plumbing; behavior identical to __init__)."""
        self = cls.__new__(cls)
        self.ch_claim_timeout = claim_timeout
        self.ch_pool = pool
        self.ch_throw_error = True
        self.ch_claim_stack = claim_stack
        self.ch_callback = callback
        self.ch_log = log
        self.ch_lat = getattr(pool, "p_lat", None)
        FSM.__init__(self, "waiting", loop=loop)
        self.ch_started = self._loop.time() * 1000.0
        return self

    # -- misuse traps (lib/connection-fsm.js:529-557) -------------------
    @property
    def writable(self) -> Any:
        raise mod_errors.ClaimHandleMisusedError()

    @property
    def readable(self) -> Any:
        raise mod_errors.ClaimHandleMisusedError()

    def on(self, event: str, listener: Callable) -> Callable:
        if event in ("readable", "close"):
            raise mod_errors.ClaimHandleMisusedError()
        return super().on(event, listener)

    def once(self, event: str, listener: Callable) -> Callable:
        if event in ("readable", "close"):
            raise mod_errors.ClaimHandleMisusedError()
        return super().once(event, listener)

    def disable_release_leak_check(self) -> None:
        self.ch_do_release_leak_check = False

    # -- signal functions ----------------------------------------------
    #
    # These are direct state-dispatch rather than emit + scoped-listener
    # pairs: the signals are internal to this FSM (nothing ever listens
    # for them externally), and the claim path walks four handle states
    # per claim — the listener churn was the hot spot.  goto_state still
    # defers transitions requested during an entry function, so the
    # observable ordering is identical to the listener formulation.

    def try_(self, slot: "ConnectionSlotFSM") -> None:
        """The pool offers `slot` to this handle (must be idle)."""
        if self._fsm_state != "waiting":
            raise FSMError('ClaimHandle.try_ only in "waiting" (is in "%s")'
                           % self.get_state())
        if not slot.is_in_state("idle"):
            raise FSMError('ClaimHandle.try_ needs an idle slot (is in "%s")'
                           % slot.get_state())
        self.ch_slot = slot
        self.goto_state("claiming")

    def accept(self, connection: Any) -> None:
        if self._fsm_state != "claiming":
            raise FSMError("accept only in claiming")
        self.ch_connection = connection
        self.goto_state("claimed")

    def reject(self) -> None:
        if self._fsm_state != "claiming":
            raise FSMError("reject only in claiming")
        if self.ch_cancelled:
            self.goto_state("cancelled")
        else:
            self.goto_state("waiting")

    def cancel(self) -> None:
        if self._fsm_state == "claimed":
            self.release()
        else:
            self.ch_cancelled = True
            # in "claiming" the cancellation is applied on reject/accept;
            # in "waiting" it takes effect now (lib/connection-fsm.js:580)
            if self._fsm_state == "waiting":
                self.goto_state("cancelled")

    def timeout(self) -> None:
        if self._fsm_state != "waiting":
            raise FSMError("timeout only in waiting")
        self._on_claim_timeout()

    def _on_claim_timeout(self) -> None:
        self.ch_last_error = mod_errors.ClaimTimeoutError(self.ch_pool)
        self.ch_pool._incr_counter("claim-timeout")
        self.goto_state("failed")

    def fail(self, err: BaseException) -> None:
        if self._fsm_state == "waiting":
            self.ch_last_error = err
            self.goto_state("failed")

    def _relinquish(self, state: str) -> None:
        if self._fsm_state != "claimed":
            if self.is_in_state("released") or self.is_in_state("closed"):
                stack = self.ch_release_stack or ["?"]
                # python stacks are innermost-last: the releasing call
                # site sits 2 frames above the capture (release ->
                # _relinquish); node's stack[2] is the same frame
                # counted from the other end (lib/connection-fsm.js:603)
                by = stack[-3] if len(stack) >= 3 else stack[-1]
                raise mod_errors.CueballError(
                    "Connection not claimed by this handle, released by %s"
                    % by)
            raise mod_errors.CueballError(
                'ClaimHandle.release() called while in state "%s"'
                % self.get_state())
        self.ch_release_stack = mod_utils.maybe_capture_stack_trace()
        self.goto_state(state)

    def release(self) -> None:
        self._relinquish("released")

    def close(self) -> None:
        self._relinquish("closed")

    def report_failure(self, err: Optional[BaseException] = None) -> None:
        _report_failure(self, err)

    def get_backend(self) -> Optional[Dict[str, Any]]:
        return _handle_backend(self)

    # -- states ----------------------------------------------------------
    def state_waiting(self, S: StateScope) -> None:
        S.valid_transitions(("claiming", "cancelled", "failed"))
        self.ch_slot = None
        if math.isfinite(self.ch_claim_timeout):
            S.timeout(self.ch_claim_timeout, self._on_claim_timeout)

    def state_claiming(self, S: StateScope) -> None:
        S.valid_transitions(("claimed", "waiting", "cancelled"))
        self.ch_slot.claim(self)

    def _on_claimed_conn_error(self, err: BaseException) -> None:
        conn = self.ch_connection
        if count_listeners(conn, "error") == 0 and self.ch_throw_error:
            # End-user never registered an 'error' listener: surface
            # the failure loudly (lib/connection-fsm.js:697-706).
            raise err
        self.ch_log.warn(
            "connection emitted error while claimed "
            '(for claim callback "%s")',
            getattr(self.ch_callback, "__name__", "?"))
        self.ch_pool._incr_counter("error-while-claimed")

    def state_claimed(self, S: StateScope) -> None:
        S.valid_transitions(("released", "closed"))

        if self.ch_cancelled:
            S.goto_state("released")
            return

        conn = self.ch_connection
        cnt = count_listeners
        self.ch_pre_listeners = (cnt(conn, "close"), cnt(conn, "error"),
                                 cnt(conn, "readable"), cnt(conn, "data"))
        S.on(conn, "error", self._on_claimed_conn_error)
        # the wait ends here, just before the user callback; pinger
        # claims are the pool's own and not counted
        lat = self.ch_lat
        if lat is not None and not self.ch_pinger:
            now = self._loop.time() * 1000.0
            lat.wait.record(now - self.ch_started)
            self.ch_claimed_at = now
        self.ch_callback(None, self, conn)

    def _record_hold(self) -> None:
        """claimed -> released/closed: the lease ends.  Only a handle
        whose wait was recorded has a hold."""
        at = self.ch_claimed_at
        if at is not None:
            self.ch_claimed_at = None
            self.ch_lat.hold.record(self._loop.time() * 1000.0 - at)

    def state_released(self, S: StateScope) -> None:
        S.valid_transitions([])
        self._record_hold()
        if not self.ch_do_release_leak_check:
            return
        conn = self.ch_connection
        pre = self.ch_pre_listeners
        if pre is None:
            return
        cnt = count_listeners
        for i, evt in enumerate(self._LEAK_EVENTS):
            new_count = cnt(conn, evt)
            if new_count > pre[i]:
                self.ch_log.warn(
                    "connection claimer looks like it leaked event "
                    "handlers", event=evt, count_before_claim=pre[i],
                    count_after_release=new_count)

    def state_closed(self, S: StateScope) -> None:
        S.valid_transitions([])
        self._record_hold()
        # no leak check: the connection is being torn down anyway

    def state_cancelled(self, S: StateScope) -> None:
        S.valid_transitions([])
        # Public API: the callback must NOT be called after .cancel().

    def state_failed(self, S: StateScope) -> None:
        S.valid_transitions([])
        # scheduled directly, not through the scope: failed is terminal
        # so the callback can never become stale, and an empty terminal
        # scope lets _fsm_terminal_settled dispose it (cycle break;
        # mirrors the native CH_state_failed)
        self._loop.call_soon(
            lambda: self.ch_callback(self.ch_last_error))

    def _fsm_terminal_settled(self) -> None:
        """Break the per-claim reference cycles once the handle settles
        in a terminal state (pure twin of ch_terminal_cleanup in
        speed.cpp): dispose the empty terminal scope (fsm<->scope) and
        unregister the pool ticket (handle<->ticket).  User listeners
        are untouched and still receive the queued terminal
        stateChanged."""
        wn = getattr(self, "ch_waiter_node", None)
        if wn is not None:
            if wn.linked:
                wn.remove()
            self.ch_waiter_node = None
        sc = self._fsm_scope
        if sc is not None:
            self._fsm_scope = None
            sc._dispose()
        ev = getattr(self, "_events", None)
        if ev is None:
            return
        ls = ev.get("stateChanged")
        if not ls:
            return
        ls[:] = [h for h in ls
                 if not getattr(h, "_cueball_ticket", False)]
        if not ls:
            ev.pop("stateChanged", None)


# the handle's own claimed-state error listener is not a user leak
ClaimHandle._on_claimed_conn_error._cueball_internal = True  # type: ignore[attr-defined]


#: pure-Python claim handle kept importable for the CUEBALL_PURE runtime
PyClaimHandle = ClaimHandle

if _native_count is not None:
    # Native core present: the claim handle's entire hot path (signal
    # methods + the waiting/claiming/claimed/released states) lives in
    # C (cueball_amd/_native/speed.cpp, ClaimHandleBase).  Semantics
    # are identical to PyClaimHandle above — the full test suite runs
    # against both (CUEBALL_PURE=1 selects the Python one).
    from . import _speed as _speed_mod
    from ._speed import ClaimHandleBase as _CHBase

    _speed_mod._set_claim_helpers(
        mod_errors.ClaimTimeoutError,
        mod_errors.CueballError,
        mod_errors.ClaimHandleMisusedError,
        mod_utils.maybe_capture_stack_trace,
    )
    # the core skips that call while stack traces are off
    mod_utils._bind_native_stack_flag(_speed_mod._set_stack_traces)

    class ClaimHandle(_CHBase):  # noqa: F811
        """Claim handle backed by the native core (docs: PyClaimHandle)."""

        def __init__(self, options: Dict[str, Any]) -> None:
            throw_error = options.get("throwError")
            log = options["log"]
            if not options.get("_logReady"):
                log = log.child(component="ClaimHandle")
            self._setup(
                options["pool"],
                options["claimStack"],
                options["callback"],
                log,
                float(options["claimTimeout"]),
                True if throw_error is None else bool(throw_error),
                options.get("loop"),
            )

        @classmethod
        def fast(cls, pool: Any, claim_stack: List[str],
                 callback: Callable, log: CueballLogger,
                 claim_timeout: float, loop: Any) -> "ClaimHandle":
            self = cls.__new__(cls)
            self._setup(pool, claim_stack, callback, log,
                        float(claim_timeout), True, loop)
            return self

        ch_failure_reported = False

        def report_failure(self,
                           err: Optional[BaseException] = None) -> None:
            _report_failure(self, err)

        def get_backend(self) -> Optional[Dict[str, Any]]:
            return _handle_backend(self)


def count_listeners(emitter: Any, event: str) -> int:
    """Count user-registered listeners, ignoring cueball's own internal
    handlers (lib/connection-fsm.js:786-808)."""
    if _native_count is not None and isinstance(emitter, EventEmitter):
        return _native_count(emitter, event)
    # fast path for our own EventEmitter: read the list in place
    ev = getattr(emitter, "_events", None)
    if ev is not None:
        ls = ev.get(event)
    elif hasattr(emitter, "listeners"):
        ls = emitter.listeners(event)
    else:
        return 0
    if not ls:
        return 0
    n = 0
    for h in ls:
        if not callable(h):
            continue
        target = getattr(h, "listener", h)
        if getattr(h, "_cueball_internal", False) or \
                getattr(target, "_cueball_internal", False):
            continue
        n += 1
    return n


class ConnectionSlotFSM(_SlotFSMBase):
    """One pool/set slot: drives a SocketMgrFSM and reports the
    transitions its owner cares about (lib/connection-fsm.js:810-1242)."""

    def __init__(self, options: Dict[str, Any]) -> None:
        self.csf_pool = options["pool"]
        self.csf_backend = options["backend"]
        self.csf_wanted = True
        self.csf_handle: Optional[ClaimHandle] = None
        self.csf_prev_handle: Optional[ClaimHandle] = None
        # busy/idle hot-cycle state (see _busy_* / _idle_* helpers):
        # scopes of the current busy/idle states plus the
        # event-observed smgr state, with the callbacks bound once here
        # instead of allocating closures on every claim.
        self.csf_observed = "connected"
        self.csf_busy_scope: Optional[StateScope] = None
        self.csf_idle_scope: Optional[StateScope] = None
        self._b_busy_smgr = self._busy_smgr_cb
        self._b_busy_hdl = self._busy_hdl_cb
        self._b_idle_smgr = self._idle_smgr_cb
        self._b_idle_unwanted = self._idle_on_unwanted
        self._b_idle_ping = self._idle_ping_cb
        self.csf_monitor = bool(options["monitor"])
        self.csf_checker = options.get("checker")
        self.csf_check_timeout = options.get("checkTimeout")
        log: CueballLogger = options["log"]
        self.csf_log = log.child(
            component="ConnectionSlotFSM",
            backend=self.csf_backend.get("key"),
            address=self.csf_backend.get("address"),
            port=self.csf_backend.get("port"),
        )
        self.csf_smgr = SocketMgrFSM({
            "pool": options["pool"],
            "constructor": options["constructor"],
            "backend": options["backend"],
            "log": options["log"],
            "recovery": options["recovery"],
            "monitor": bool(options["monitor"]),
            "slot": self,
            "loop": options.get("loop"),
        })
        super().__init__("init", loop=options.get("loop"))
        # Native busy/idle hot cycle: with the C core loaded and no
        # health checker configured, state_busy/state_idle and their
        # event callbacks run natively (zero Python allocation per
        # claim cycle); monitor/unwanted idle entries and every other
        # state still use the Python entries above.
        if _SlotKit is not None and self.csf_checker is None:
            self._csf_kit = _SlotKit(self, self.csf_smgr)
            self._set_fast_kit(self._csf_kit)

    # -- signal functions ----------------------------------------------
    def set_unwanted(self) -> None:
        if self.csf_wanted is False:
            return
        self.csf_wanted = False
        self.csf_smgr.set_unwanted()
        self.emit("unwanted")

    def start(self) -> None:
        if not self.is_in_state("init"):
            raise FSMError("start only in init")
        self.emit("startAsserted")

    def claim(self, handle: ClaimHandle) -> None:
        # direct dispatch (hot path; see ClaimHandle signal comment)
        if self._fsm_state != "idle":
            raise FSMError("claim only in idle")
        if self.csf_handle is not None:
            raise FSMError("slot already has a handle")
        self.csf_handle = handle
        self.goto_state("busy")

    def make_child_logger(self, **fields: Any) -> CueballLogger:
        return self.csf_log.child(**fields)

    def get_socket_mgr(self) -> SocketMgrFSM:
        return self.csf_smgr

    def get_backend(self) -> Dict[str, Any]:
        return self.csf_backend

    def is_running_ping(self) -> bool:
        return bool(self.is_in_state("busy") and self.csf_handle is not None
                    and self.csf_handle.ch_pinger)

    # -- states ----------------------------------------------------------
    def state_init(self, S: StateScope) -> None:
        S.on(self, "startAsserted", lambda: S.goto_state("connecting"))

    def state_connecting(self, S: StateScope) -> None:
        S.valid_transitions(["failed", "retrying", "idle"])
        smgr = self.csf_smgr

        def on_smgr_state(st: str) -> None:
            if st in ("init", "connecting"):
                return
            if st == "failed":
                S.goto_state("failed")
            elif st == "error":
                S.goto_state("retrying")
            elif st == "connected":
                S.goto_state("idle")
            else:
                raise FSMError(
                    'Unhandled smgr state transition: .connect() => "%s"'
                    % st)

        S.on(smgr, "stateChanged", on_smgr_state)
        smgr.connect()

    def state_failed(self, S: StateScope) -> None:
        S.valid_transitions([])
        if not self.csf_smgr.is_in_state("failed"):
            raise FSMError("smgr must be failed")

    def state_retrying(self, S: StateScope) -> None:
        S.valid_transitions(["idle", "failed", "retrying", "stopped",
                             "stopping"])
        smgr = self.csf_smgr

        def on_smgr_state(st: str) -> None:
            if st in ("backoff", "connecting"):
                return
            if st == "failed":
                S.goto_state("failed")
            elif st == "error":
                if self.csf_monitor and not self.csf_wanted:
                    S.goto_state("stopped")
                else:
                    S.goto_state("retrying")
            elif st == "connected":
                S.goto_state("idle")
            else:
                raise FSMError(
                    'Unhandled smgr state transition: .retry() => "%s"' % st)

        S.on(smgr, "stateChanged", on_smgr_state)

        def on_unwanted() -> None:
            if self.csf_monitor and smgr.is_in_state("backoff"):
                S.goto_state("stopping")

        S.on(self, "unwanted", on_unwanted)
        smgr.retry()

    _IDLE_VALID = ("retrying", "connecting", "stopping", "stopped",
                   "busy")

    def state_idle(self, S: StateScope) -> None:
        S.valid_transitions(self._IDLE_VALID)
        smgr = self.csf_smgr
        self.csf_idle_scope = S

        if self.csf_handle is not None:
            self.csf_prev_handle = self.csf_handle
        self.csf_handle = None

        # A monitor that connected becomes a normal slot
        # (lib/connection-fsm.js:1053-1057).
        if self.csf_monitor is True:
            self.csf_monitor = False
            if smgr.is_in_state("connected") or smgr.is_in_state("init"):
                smgr.set_monitor(False)
            else:
                # Divergence from the reference (bug fix, property
                # suite): the monitor's socket connected and died in
                # the same loop spin, so the smgr already sits in
                # error/closed — the reference's setMonitor assert
                # (lib/connection-fsm.js:176) would crash here.
                # Convert to a normal slot directly: same outcome as
                # if the events had arrived one spin apart.
                smgr.sm_monitor = False
                smgr.reset_backoff()

        # register the smgr listener in every case — pending smgr events
        # must find a handler even when the slot is already unwanted
        S.on(smgr, "stateChanged", self._b_idle_smgr)

        if not self.csf_wanted:
            self._idle_on_unwanted()
            return
        S.on(self, "unwanted", self._b_idle_unwanted)

        if self.csf_check_timeout is not None and \
                self.csf_checker is not None:
            S.timeout(self.csf_check_timeout, self._b_idle_ping)

    def _idle_on_unwanted(self) -> None:
        S = self.csf_idle_scope
        smgr = self.csf_smgr
        if smgr.is_in_state("connected"):
            S.goto_state("stopping")
        elif smgr.is_in_state("error") or smgr.is_in_state("closed"):
            # Divergence from the reference (bug fix, found by the
            # property suite): a slot flagged unwanted whose socket
            # connected and then died within the same loop spin
            # reaches idle with the smgr already in error/closed.
            # The reference's early-return would leave the slot
            # wedged in idle with no listeners registered
            # (lib/connection-fsm.js:1059-1062 registers nothing
            # when !csf_wanted).  An unwanted slot with a dead
            # socket is simply done.
            S.goto_state("stopped")

    def _idle_smgr_cb(self, st: str) -> None:
        S = self.csf_idle_scope
        if st == "error":
            if self.csf_wanted:
                S.goto_state("retrying")
            else:
                S.goto_state("stopped")
        elif st == "closed":
            if not self.csf_wanted:
                S.goto_state("stopped")
            else:
                S.goto_state("connecting")
        else:
            raise FSMError(
                'Unhandled smgr state transition: connected => "%s"' % st)

    def _idle_ping_cb(self) -> None:
        _do_ping_check(self, self.csf_checker)

    # The busy-state helpers are pre-bound methods (see __init__)
    # rather than per-entry closures: the busy/idle cycle runs once per
    # claim, and closure allocation was a measurable share of the claim
    # path's memory traffic.  csf_busy_scope carries the state scope;
    # a callback whose scope has been exited no-ops in goto_state, the
    # same guard the closures had by capturing S.
    def _busy_smgr_cb(self, st: str) -> None:
        # Track the smgr state as *observed through events*: a
        # transition that happened this same loop spin is still pending
        # delivery, and the exit decision must match what we have
        # actually seen (lib/connection-fsm.js:885-890, :1129-1196).
        self.csf_observed = st

    def _busy_on_release(self) -> None:
        S = self.csf_busy_scope
        st = self.csf_observed
        if st == "connected":
            if self.csf_wanted:
                S.goto_state("idle")
            else:
                S.goto_state("stopping")
        elif st == "closed":
            if self.csf_wanted:
                S.goto_state("connecting")
            else:
                S.goto_state("stopped")
        elif st == "error":
            S.goto_state("retrying")
        else:
            raise FSMError(
                'Handle released while smgr was in unhandled state "%s"'
                % self.csf_smgr.get_state())

    def _busy_on_close(self) -> None:
        S = self.csf_busy_scope
        if self.csf_observed == "connected":
            S.goto_state("killing")
        else:
            S.goto_state("retrying")

    def _busy_hdl_cb(self, st: str) -> None:
        if st == "released":
            self._busy_on_release()
        elif st == "closed":
            self._busy_on_close()

    _BUSY_VALID = ("idle", "stopping", "stopped", "retrying",
                   "killing", "connecting")

    def state_busy(self, S: StateScope) -> None:
        S.valid_transitions(self._BUSY_VALID)
        smgr = self.csf_smgr
        hdl = self.csf_handle
        self.csf_observed = "connected"
        self.csf_busy_scope = S
        S.on(smgr, "stateChanged", self._b_busy_smgr)
        S.on(hdl, "stateChanged", self._b_busy_hdl)

        # The smgr may have left 'connected' before we got here; if we
        # lost the race, treat it like our handle was released.
        if smgr.is_in_state("connected"):
            hdl.accept(smgr.get_socket())
        else:
            hdl.reject()
            self.csf_handle = None
            self._busy_on_release()

    def state_killing(self, S: StateScope) -> None:
        S.valid_transitions(["retrying"])
        smgr = self.csf_smgr

        def on_smgr_state(st: str) -> None:
            if st in ("closed", "error"):
                S.goto_state("retrying")

        S.on(smgr, "stateChanged", on_smgr_state)
        # The socket may already be closed with the event still pending;
        # if so just wait for it (lib/connection-fsm.js:1209-1216).
        if not smgr.is_in_state("closed") and not smgr.is_in_state("error"):
            smgr.close()

    def state_stopping(self, S: StateScope) -> None:
        S.valid_transitions(["stopped"])
        smgr = self.csf_smgr

        def on_smgr_state(st: str) -> None:
            if st in ("closed", "error"):
                S.goto_state("stopped")

        S.on(smgr, "stateChanged", on_smgr_state)
        if not smgr.is_in_state("closed") and not smgr.is_in_state("error"):
            smgr.close()

    def state_stopped(self, S: StateScope) -> None:
        S.valid_transitions([])
        smgr = self.csf_smgr
        if not (smgr.is_in_state("closed") or smgr.is_in_state("error")
                or smgr.is_in_state("failed")):
            raise FSMError("smgr must be stopped")


if _native_count is not None:
    # the native core tests for these two classes by identity before it
    # walks an MRO (cueball_amd/_native/speed.cpp, is_handle/is_slot)
    _speed_mod._set_cycle_classes(ClaimHandle, ConnectionSlotFSM, None)


def _do_ping_check(fsm: ConnectionSlotFSM, checker: Callable) -> None:
    """Health-check an idle slot: claim it internally and run the checker
    (lib/connection-fsm.js:1101-1127)."""

    def ping_check_adapter(err: Optional[BaseException], hdl: ClaimHandle,
                           conn: Any = None) -> None:
        # infinite timeout + no .fail() => err is always None here
        if err is not None:
            raise FSMError("ping check handle failed unexpectedly")
        checker(hdl, conn)

    handle = ClaimHandle({
        "pool": fsm.csf_pool,
        "claimStack": ["claim", "cueball._do_ping_check",
                       "cueball._do_ping_check"],
        "callback": ping_check_adapter,
        "log": fsm.csf_log,
        "claimTimeout": math.inf,
        "loop": fsm._loop,
    })
    handle.ch_pinger = True
    # If the try fails and the handle returns to "waiting", just let go
    # of it entirely.
    handle.try_(fsm)
