"""Request retries for the HTTP agents: policy, retry budget, driver.

The reference leaves retries to its callers (restify's clients retry
above it); this rebuild ships the HTTP client itself, so the retry loop
lives here, where it can do two things a caller's loop cannot: ask the
pool for a *different* backend (``claim({"avoidBackends": ...})``), and
bound retry amplification with a budget shared by every request to a
host (as Finagle and Envoy do).  Opt-in: an agent without the ``retry``
option creates none of this module's objects.

Three parts:

- ``RetryPolicy``: an agent's validated ``retry`` option
  (``utils.assert_retry_policy``) in the form the driver reads.
- ``RetryHost``: what all requests to one host share: the budget's two
  counts, the counters, the requests that wait in a backoff.
- ``RetriedRequest``: the driver, one per request.  It runs one try at
  a time; "start one try" is a callable handed in, so the driver knows
  nothing of agents, pools or sockets.

The try protocol.  ``start_try(avoid)`` is called with a tuple of
backend keys to avoid and returns a *try*: an EventEmitter that emits
``response(resp)`` once headers are in (``resp.status_code``,
``resp.complete``, and an ``end`` event when the body is) or
``error(err)``, and has ``abort()``.  Two attributes tell the driver
where the try ran: ``try_backend``, the key of the backend it was
claimed on (None for as long as it has no real socket), and
``try_handle``, its claim handle (None likewise).  A try that ran on
more than one backend (``hedge.HedgedTry``) also has ``try_backends``,
a tuple of all of them; a failed try's backends are all avoided.
"""

from __future__ import annotations

import math
import random
from typing import Any, Callable, Dict, List, Mapping, Optional, Set

from . import errors as mod_errors
from .events import EventEmitter

__all__ = ["RetryPolicy", "RetryHost", "RetriedRequest", "COUNTERS"]

#: every counter of ``RetryHost.counters``
COUNTERS = ("retry-reset", "retry-timeout", "retry-status",
            "retry-claim-failure", "retry-budget-exhausted",
            "retries-exhausted", "timeout-per-try", "timeout-total")

#: claim errors that say "not now", as opposed to "never again"
_CLAIM_FAILURES = (mod_errors.ClaimTimeoutError, mod_errors.NoBackendsError,
                   mod_errors.PoolFailedError)


class RetryPolicy:
    """A validated ``retry`` mapping, with its lists as sets."""

    __slots__ = ("options", "max_retries", "retry_on", "statuses",
                 "methods", "per_try", "total", "delay", "max_delay",
                 "jitter", "avoid")

    def __init__(self, options: Mapping[str, Any]) -> None:
        self.options = dict(options)
        self.max_retries: int = options["maxRetries"]
        self.retry_on = frozenset(options["retryOn"])
        self.statuses = frozenset(options["retryStatuses"]) \
            if "status" in self.retry_on else frozenset()
        self.methods = frozenset(options["methods"])
        self.per_try: Optional[float] = options["perTryTimeout"]
        self.total: Optional[float] = options["totalTimeout"]
        self.delay: float = options["delay"]
        self.max_delay: float = options["maxDelay"]
        self.jitter: bool = options["jitter"]
        self.avoid: bool = options["avoidFailedBackends"]

    def backoff_cap(self, n: int) -> float:
        """The longest wait before retry `n` (1-based), ms."""
        # 2.0 ** 1024 overflows; nobody waits for retry 1000 either
        return min(self.max_delay, self.delay * 2.0 ** min(n - 1, 1000))

    def backoff(self, n: int, rng: Callable[[], float]) -> float:
        cap = self.backoff_cap(n)
        return rng() * cap if self.jitter else cap


class RetryHost:
    """Shared by every driven request to one host: the budget and the
    counters.  The budget is concurrency-based (Envoy's), so it needs
    no clock: ``active`` counts the requests in flight, a backoff
    included, ``retrying`` those among them that are in, or waiting
    for, a retry."""

    __slots__ = ("host", "percent", "min_concurrency", "active",
                 "retrying", "counters", "backoffs", "on_count")

    def __init__(self, host: str, budget: Optional[Mapping[str, Any]],
                 on_count: Optional[Callable[[str, str], None]] = None
                 ) -> None:
        self.host = host
        self.percent: Optional[float] = None
        self.min_concurrency = 0
        if budget is not None:
            self.percent = budget["percent"]
            self.min_concurrency = budget["minConcurrency"]
        self.active = 0
        self.retrying = 0
        self.counters: Dict[str, int] = {}
        #: the requests that wait in a backoff right now
        self.backoffs: Set["RetriedRequest"] = set()
        #: on_count(host, counter) after every bump (the agent's
        #: Prometheus counters)
        self.on_count = on_count

    def count(self, counter: str) -> None:
        self.counters[counter] = self.counters.get(counter, 0) + 1
        if self.on_count is not None:
            self.on_count(self.host, counter)

    def limit(self) -> Optional[int]:
        """How many requests may be retrying at once, None without a
        budget."""
        if self.percent is None:
            return None
        return max(self.min_concurrency,
                   math.floor(self.percent * self.active / 100.0))

    def allows(self, already_retrying: bool) -> bool:
        """May one more request retry?  Asked when a try fails, with
        the failing request still counted in ``active``.  A request
        that is retrying already holds its place."""
        limit = self.limit()
        if limit is None:
            return True
        others = self.retrying - (1 if already_retrying else 0)
        return others + 1 <= limit

    def stats(self) -> Dict[str, Any]:
        return {"active": self.active, "retrying": self.retrying,
                "limit": self.limit(),
                "counters": {c: self.counters.get(c, 0) for c in COUNTERS}}

    def stop(self, err: BaseException) -> None:
        """End every request that waits in a backoff with `err`."""
        for req in list(self.backoffs):
            req._end_error(err)


class RetriedRequest(EventEmitter):
    """One request under a retry policy.  An EventEmitter with the
    surface callers use on HttpRequest: ``abort()``, ``aborted``, and
    the events ``response``, ``error`` and ``abort``; plus
    ``attempts`` (tries started), ``retry_reasons`` (one per retry) and
    the event ``retry(attempt, reason, delay_ms)``, emitted when retry
    number `attempt` is decided, `delay_ms` before it starts.

    The commit point is the arrival of response headers with a status
    that is not selected for retry: from then on the response has been
    forwarded and nothing is retried.  A response whose status *is*
    selected is held back until its body is complete, so its keep-alive
    connection is released before the next claim; if no retry is left,
    or none is allowed, it is delivered after all.
    """

    # What a request that succeeds on its first try never changes stays
    # on the class: one request, one object, as few stores as possible.
    aborted = False
    attempts = 0
    _done = False
    _committed = False
    _retrying = False
    _try: Any = None
    _held: Any = None               # the response whose 'end' we await
    _try_timer: Any = None
    _total_timer: Any = None
    _backoff_timer: Any = None
    _failed_on: Optional[List[str]] = None

    def __init__(self, loop: Any, policy: RetryPolicy, host: RetryHost,
                 method: str, start_try: Callable[[tuple], Any],
                 is_stopped: Optional[Callable[[], bool]] = None,
                 rng: Optional[Callable[[], float]] = None) -> None:
        super().__init__()
        self.method = method = method.upper()
        self.retry_reasons: List[str] = []
        self._loop = loop
        self._policy = policy
        self._host = host
        self._start_try = start_try
        self._is_stopped = is_stopped
        self._rng = rng
        self._retriable = method in policy.methods

    # -- life cycle -----------------------------------------------------
    def start(self) -> "RetriedRequest":
        """Start the first try.  What `start_try` raises here is
        raised to the caller, as ``Agent.request()`` does."""
        assert self.attempts == 0 and not self._done
        self._host.active += 1
        total = self._policy.total
        if total is not None:
            self._total_timer = self._loop.call_later(
                total / 1000.0, self._on_total_timeout)
        try:
            self._begin_try()
        except BaseException:
            self._finish()
            raise
        return self

    def _finish(self) -> None:
        """Every exit comes through here, once: no timer, listener or
        budget count outlives the request."""
        if self._done:
            return
        self._done = True
        if self._try is not None or self._try_timer is not None:
            self._drop_try(False)
        timer = self._total_timer
        if timer is not None:
            timer.cancel()
            self._total_timer = None
        host = self._host
        timer = self._backoff_timer
        if timer is not None:
            timer.cancel()
            self._backoff_timer = None
            host.backoffs.discard(self)
        host.active -= 1
        if self._retrying:
            self._retrying = False
            host.retrying -= 1

    def _begin_try(self) -> None:
        policy = self._policy
        avoid: tuple = ()
        if self._failed_on is not None and policy.avoid:
            avoid = tuple(self._failed_on)
        self.attempts += 1
        if policy.per_try is not None:
            self._try_timer = self._loop.call_later(
                policy.per_try / 1000.0, self._on_try_timeout)
        t = self._try = self._start_try(avoid)
        t.on("response", self._on_response)
        t.on("error", self._on_error)

    def _drop_try(self, abort: bool) -> None:
        """Stop listening to the current try, and to a response of its
        that we wait for the end of; abort the try if asked to.  A try
        that is dropped cannot reach us again: its listeners are gone,
        and the next try begins on a later turn of the loop."""
        timer = self._try_timer
        if timer is not None:
            timer.cancel()
            self._try_timer = None
        held = self._held
        if held is not None:
            self._held = None
            held.remove_listener("end", self._on_body_end)
        t = self._try
        if t is None:
            return
        self._try = None
        t.remove_listener("response", self._on_response)
        t.remove_listener("error", self._on_error)
        if abort:
            t.abort()

    # -- user API -------------------------------------------------------
    def abort(self) -> None:
        """Abort the current try, or cancel the backoff.  Emits 'abort'
        and nothing further."""
        if self.aborted or self._done:
            return
        self.aborted = True
        self._drop_try(True)
        self._finish()
        self.emit("abort")

    # -- endings ----------------------------------------------------------
    def _end_error(self, err: BaseException) -> None:
        self._drop_try(True)
        self._finish()
        self.emit("error", err)

    def _end_response(self, resp: Any) -> None:
        self._finish()
        self.emit("response", resp)

    # -- events of the current try ----------------------------------------
    def _on_response(self, resp: Any) -> None:
        if self._try is None or self._done:
            return
        if self._retriable and resp.status_code in self._policy.statuses:
            # held back until the body is in: the connection is then
            # released, not closed, and the decision falls with no
            # lease held
            if resp.complete:
                self._try_failed("status", resp, None)
            else:
                self._held = resp
                resp.on("end", self._on_body_end)
            return
        self._committed = True
        self.emit("response", resp)
        if self._done:
            return
        if resp.complete:
            self._finish()
        else:
            self._held = resp
            resp.on("end", self._on_body_end)

    def _on_body_end(self) -> None:
        resp = self._held
        if resp is None or self._done:
            return
        if self._committed:
            self._finish()
        else:
            self._try_failed("status", resp, None)

    def _on_error(self, err: BaseException) -> None:
        t = self._try
        if t is None or self._done:
            return
        if self._committed:
            # forwarded already: surfaces as it always did
            self._finish()
            self.emit("error", err)
            return
        if getattr(t, "try_backend", None) is not None:
            reason: Optional[str] = "reset"
        elif isinstance(err, _CLAIM_FAILURES):
            reason = "claim-failure"
        else:
            # a stopping pool, a stopped agent, or a full claim queue
            # (ClaimQueueFullError): the pool has just said that it is
            # overloaded, so no retry and nothing off the budget
            reason = None
        self._try_failed(reason, None, err)

    def _on_try_timeout(self) -> None:
        self._try_timer = None
        if self._done:
            return
        host = self._host
        host.count("timeout-per-try")
        err = mod_errors.RequestTimeoutError("per-try",
                                             self._policy.per_try)
        t = self._try
        hdl = getattr(t, "try_handle", None)
        if hdl is not None and hdl.is_in_state("claimed"):
            # a backend that hangs: let outlier detection know
            hdl.report_failure(err)
        if self._committed:
            self._end_error(err)
            return
        self._try_failed("timeout", None, err, abort=True)

    def _on_total_timeout(self) -> None:
        self._total_timer = None
        if self._done:
            return
        self._host.count("timeout-total")
        self._end_error(mod_errors.RequestTimeoutError(
            "total", self._policy.total))

    # -- the decision -----------------------------------------------------
    def _try_failed(self, reason: Optional[str], resp: Any,
                    err: Optional[BaseException],
                    abort: bool = False) -> None:
        """The current try ended, before the commit point, with a
        complete response whose status is selected (`resp`) or with
        `err`.  Retry, or end with that outcome."""
        t = self._try
        # a try that ran on more than one backend (hedge.HedgedTry)
        # says so; a plain try ran on one, or on none
        keys = getattr(t, "try_backends", None)
        if keys is None:
            key = getattr(t, "try_backend", None)
            keys = () if key is None else (key,)
        self._drop_try(abort=abort)
        policy = self._policy
        host = self._host
        if self._wants_retry(reason):
            for key in keys:
                if self._failed_on is None:
                    self._failed_on = [key]
                elif key not in self._failed_on:
                    self._failed_on.append(key)
            n = len(self.retry_reasons) + 1
            delay = policy.backoff(n, self._rng or random.random)
            host.count("retry-" + reason)
            self.retry_reasons.append(reason)
            if not self._retrying:
                self._retrying = True
                host.retrying += 1
            host.backoffs.add(self)
            self._backoff_timer = self._loop.call_later(
                delay / 1000.0, self._on_backoff_over)
            self.emit("retry", n, reason, delay)
            return
        if resp is not None:
            self._end_response(resp)
        else:
            self._finish()
            self.emit("error", err)

    def _wants_retry(self, reason: Optional[str]) -> bool:
        policy = self._policy
        if reason is None or not self._retriable or \
                reason not in policy.retry_on:
            return False
        if self._is_stopped is not None and self._is_stopped():
            return False
        if len(self.retry_reasons) >= policy.max_retries:
            self._host.count("retries-exhausted")
            return False
        if not self._host.allows(self._retrying):
            self._host.count("retry-budget-exhausted")
            return False
        return True

    def _on_backoff_over(self) -> None:
        self._backoff_timer = None
        self._host.backoffs.discard(self)
        if self._done:
            return
        try:
            self._begin_try()
        except Exception as e:
            self._end_error(e)
