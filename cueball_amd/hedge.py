"""Request hedging for the HTTP agents: policy, shared state, driver.

The retry driver (cueball_amd.retry) deals with a backend that fails;
this one deals with a backend that is merely slow.  After a delay near
a high percentile of recent response times the same request is sent to
a *different* backend; the first response headers win and the other
attempt is aborted ("The Tail at Scale"; gRPC's and Envoy's hedging).
Opt-in: an agent without the ``hedge`` option creates none of this
module's objects.

Three parts, as in retry.py:

- ``HedgePolicy``: an agent's validated ``hedge`` option
  (``utils.assert_hedge_policy``) in the form the driver reads.
- ``HedgeHost``: what all requests to one host share: the budget's two
  counts, the windowed time-to-headers estimate, the counters.
- ``HedgedTry``: the driver, one per try.  It implements the try
  protocol of retry.py itself and is handed a ``start_try(avoid)``, so
  it knows nothing of agents, pools or sockets, and the retry driver
  can run it as one of its tries.
"""

from __future__ import annotations

import math
from typing import Any, Callable, Dict, Mapping, Optional, Set, Tuple

from . import latency as mod_latency
from .events import EventEmitter

__all__ = ["HedgePolicy", "HedgeHost", "HedgedTry", "COUNTERS"]

#: every counter of ``HedgeHost.counters``
COUNTERS = ("hedge-sent", "hedge-won", "hedge-lost", "hedge-failed",
            "hedge-skipped-budget", "hedge-skipped-no-idle",
            "hedge-skipped-unclaimed", "hedge-skipped-samples")

#: the cached delay estimate is recomputed at most this often (seconds
#: of loop time), and on every rotation of the window
_CACHE_S = 0.1


class HedgePolicy:
    """A validated ``hedge`` mapping, with its list as a set."""

    __slots__ = ("options", "delay", "percentile", "window", "min_samples",
                 "min_delay", "max_delay", "methods")

    def __init__(self, options: Mapping[str, Any]) -> None:
        self.options = dict(options)
        self.delay: Optional[float] = options["delay"]
        self.percentile: float = options["percentile"]
        self.window: float = options["window"]
        self.min_samples: int = options["minSamples"]
        self.min_delay: float = options["minDelay"]
        self.max_delay: float = options["maxDelay"]
        self.methods = frozenset(options["methods"])


class HedgeHost:
    """Shared by every hedged try to one host.

    The budget is concurrency-based like ``RetryHost``'s: ``active``
    counts the tries in flight, ``hedging`` those among them with a
    hedge out.

    The latency window is two histograms.  Samples go to ``current``;
    once ``window`` ms have passed since the last rotation ``previous``
    is emptied and the two swap, so that the estimate always covers
    between one and two windows of history.  Rotation is lazy (checked
    by ``record()`` and ``delay()``), so there is no timer to leak.
    """

    __slots__ = ("host", "policy", "percent", "min_concurrency", "active",
                 "hedging", "counters", "pending", "on_count", "on_delay",
                 "clock", "current", "previous", "_hist", "_rotated_at",
                 "_cache", "_cache_at")

    def __init__(self, host: str, policy: HedgePolicy,
                 clock: Callable[[], float],
                 on_count: Optional[Callable[[str, str], None]] = None,
                 on_delay: Optional[Callable[[str, Optional[float]],
                                             None]] = None,
                 histogram: Optional[Callable[[], Any]] = None) -> None:
        self.host = host
        self.policy = policy
        self.percent: Optional[float] = None
        self.min_concurrency = 0
        budget = policy.options["budget"]
        if budget is not None:
            self.percent = budget["percent"]
            self.min_concurrency = budget["minConcurrency"]
        self.active = 0
        self.hedging = 0
        self.counters: Dict[str, int] = {}
        #: the tries whose hedge timer is armed right now
        self.pending: Set["HedgedTry"] = set()
        #: on_count(host, counter) after every bump, on_delay(host, ms)
        #: after every recomputation of the estimate (the agent's
        #: Prometheus metrics)
        self.on_count = on_count
        self.on_delay = on_delay
        #: seconds, the loop's clock
        self.clock = clock
        # through the module, so that the native histogram is used
        # when it is loaded
        self._hist = histogram or mod_latency.LatencyHistogram
        self.current = self._hist()
        self.previous = self._hist()
        self._rotated_at: Optional[float] = None
        #: percentile -> its value over the merged window, ms
        self._cache: Dict[float, Optional[float]] = {}
        self._cache_at = 0.0

    # -- counters and budget ------------------------------------------------
    def count(self, counter: str) -> None:
        self.counters[counter] = self.counters.get(counter, 0) + 1
        if self.on_count is not None:
            self.on_count(self.host, counter)

    def limit(self) -> Optional[int]:
        """How many tries may have a hedge out at once, None without a
        budget."""
        if self.percent is None:
            return None
        return max(self.min_concurrency,
                   math.floor(self.percent * self.active / 100.0))

    def allows(self) -> bool:
        """May one more try send its hedge?  Asked with the asking try
        counted in ``active``."""
        limit = self.limit()
        return limit is None or self.hedging + 1 <= limit

    # -- the window -----------------------------------------------------------
    def _rotate(self, now: float) -> None:
        last = self._rotated_at
        if last is None:
            self._rotated_at = now
            return
        gone = (now - last) * 1000.0
        window = self.policy.window
        if gone < window:
            return
        self.previous.reset()
        if gone >= 2.0 * window:
            self.current.reset()
        else:
            self.current, self.previous = self.previous, self.current
        self._rotated_at = now
        self._cache.clear()

    def record(self, ms: float, now: Optional[float] = None) -> None:
        """One attempt's time to headers (or, for an attempt aborted
        because the other one won, the time it had been out)."""
        self._rotate(self.clock() if now is None else now)
        self.current.record(ms)

    def samples(self) -> int:
        return self.current.count + self.previous.count

    def _merged(self) -> Any:
        merged = self._hist()
        merged.merge(self.previous)
        merged.merge(self.current)
        return merged

    def delay(self, now: Optional[float] = None,
              policy: Optional[HedgePolicy] = None) -> Optional[float]:
        """The adaptive hedge delay in ms: `policy`'s percentile (the
        host's own policy by default) of the window, clamped to its
        ``[minDelay, maxDelay]``; None with fewer than ``minSamples``
        samples in the window."""
        if now is None:
            now = self.clock()
        if policy is None:
            policy = self.policy
        self._rotate(now)
        if self.samples() < self.policy.min_samples:
            return None
        cache = self._cache
        if cache and now - self._cache_at >= _CACHE_S:
            cache.clear()
        pct = policy.percentile
        value = cache.get(pct)
        if value is None:
            if not cache:
                self._cache_at = now
            value = cache[pct] = self._merged().percentile(pct / 100.0)
            if self.on_delay is not None and policy is self.policy:
                self.on_delay(self.host, min(max(value, policy.min_delay),
                                             policy.max_delay))
        return min(max(value, policy.min_delay), policy.max_delay)

    def stats(self) -> Dict[str, Any]:
        policy = self.policy
        delay = policy.delay if policy.delay is not None else self.delay()
        return {"active": self.active, "hedging": self.hedging,
                "limit": self.limit(), "delayMs": delay,
                "samples": self.samples(),
                "latency": self._merged().snapshot(),
                "counters": {c: self.counters.get(c, 0) for c in COUNTERS}}

    def stop(self) -> None:
        """Cancel every armed hedge timer; the tries carry on as plain
        ones."""
        for t in list(self.pending):
            t._cancel_timer()


class _Attempt:
    """One real try under a HedgedTry."""

    __slots__ = ("t", "started", "role", "failed")

    def __init__(self, t: Any, started: float, role: str) -> None:
        self.t = t
        self.started = started
        self.role = role
        self.failed = False


class _HandleProxy:
    """``try_handle`` of a HedgedTry: what the retry driver does to a
    try's claim handle, done to the handle of every attempt that still
    holds its claim."""

    __slots__ = ("_attempts",)

    def __init__(self, attempts: Tuple[_Attempt, ...]) -> None:
        self._attempts = attempts

    def _claimed(self) -> list:
        out = []
        for a in self._attempts:
            hdl = getattr(a.t, "try_handle", None)
            if hdl is not None and hdl.is_in_state("claimed"):
                out.append(hdl)
        return out

    def is_in_state(self, state: str) -> bool:
        if state == "claimed":
            return bool(self._claimed())
        for a in self._attempts:
            hdl = getattr(a.t, "try_handle", None)
            if hdl is not None and hdl.is_in_state(state):
                return True
        return False

    def report_failure(self, err: Optional[BaseException] = None) -> None:
        for hdl in self._claimed():
            hdl.report_failure(err)


class HedgedTry(EventEmitter):
    """One try that may be sent twice.  A *try* in the sense of
    retry.py (``response``/``error`` events, ``abort()``,
    ``try_backend``, ``try_handle``), so the retry driver can run it;
    on an agent without ``retry`` it is the request object itself, with
    the surface callers use on HttpRequest: ``abort()``, ``aborted``
    and the events ``response``, ``error`` and ``abort``; plus
    ``hedged``, ``winner`` and the event ``hedge(delay_ms)``, emitted
    when the second attempt is sent.

    The first response headers win, whatever the status: that response
    is emitted as it is and the other attempt is aborted.  An attempt
    that fails while the other is still out ends nothing; when both
    have failed, the error of the later one is emitted.
    """

    # as in RetriedRequest: what a try that is never hedged does not
    # change stays on the class
    aborted = False
    hedged = False
    #: "primary" or "hedge" once response headers are in
    winner: Optional[str] = None
    _done = False
    _counted = False                # holds one of host.hedging
    _timer: Any = None
    _delay_ms: Optional[float] = None
    _primary: Optional[_Attempt] = None
    _hedge: Optional[_Attempt] = None
    _delivered: Optional[_Attempt] = None
    _held: Any = None               # the winner's response, body not in

    def __init__(self, loop: Any, policy: HedgePolicy, host: HedgeHost,
                 method: str, start_try: Callable[[tuple], Any],
                 avoid: tuple = (),
                 has_idle: Optional[Callable[[tuple], bool]] = None,
                 is_stopped: Optional[Callable[[], bool]] = None) -> None:
        super().__init__()
        self.method = method = method.upper()
        self._loop = loop
        self._policy = policy
        self._host = host
        self._start_try = start_try
        self._avoid = tuple(avoid)
        self._has_idle = has_idle
        self._is_stopped = is_stopped
        self._hedgeable = method in policy.methods

    # -- the try protocol -------------------------------------------------
    @property
    def try_backend(self) -> Optional[str]:
        """The backend of the attempt whose outcome was delivered; the
        primary's for as long as none was."""
        a = self._delivered or self._primary
        return None if a is None else getattr(a.t, "try_backend", None)

    @property
    def try_backends(self) -> Tuple[str, ...]:
        """Every backend an attempt was claimed on, primary first."""
        out = []
        for a in (self._primary, self._hedge):
            if a is not None:
                key = getattr(a.t, "try_backend", None)
                if key is not None and key not in out:
                    out.append(key)
        return tuple(out)

    @property
    def try_handle(self) -> Optional[_HandleProxy]:
        attempts = tuple(a for a in (self._primary, self._hedge)
                         if a is not None and
                         getattr(a.t, "try_handle", None) is not None)
        return _HandleProxy(attempts) if attempts else None

    # -- life cycle ---------------------------------------------------------
    def start(self) -> "HedgedTry":
        """Start the primary attempt and arm the hedge timer.  What
        `start_try` raises here is raised to the caller."""
        assert self._primary is None and not self._done
        host = self._host
        host.active += 1
        try:
            self._primary = self._begin(self._avoid, "primary")
        except BaseException:
            self._finish()
            raise
        if not self._hedgeable or self._done:
            return self
        policy = self._policy
        delay = policy.delay
        if delay is None:
            delay = host.delay(None, policy)
            if delay is None:
                host.count("hedge-skipped-samples")
                return self
        self._delay_ms = delay
        self._timer = self._loop.call_later(delay / 1000.0, self._on_timer)
        host.pending.add(self)
        return self

    def _begin(self, avoid: tuple, role: str) -> _Attempt:
        a = _Attempt(self._start_try(avoid), self._loop.time(), role)
        if role == "primary":
            a.t.on("response", self._on_primary_response)
            a.t.on("error", self._on_primary_error)
        else:
            a.t.on("response", self._on_hedge_response)
            a.t.on("error", self._on_hedge_error)
        return a

    def _unlisten(self, a: Optional[_Attempt]) -> None:
        if a is None:
            return
        if a.role == "primary":
            a.t.remove_listener("response", self._on_primary_response)
            a.t.remove_listener("error", self._on_primary_error)
        else:
            a.t.remove_listener("response", self._on_hedge_response)
            a.t.remove_listener("error", self._on_hedge_error)

    def _cancel_timer(self) -> None:
        timer = self._timer
        if timer is not None:
            timer.cancel()
            self._timer = None
            self._host.pending.discard(self)

    def _uncount(self) -> None:
        if self._counted:
            self._counted = False
            self._host.hedging -= 1

    def _finish(self) -> None:
        """Every exit comes through here, once: no timer, listener or
        budget count outlives the try."""
        if self._done:
            return
        self._done = True
        self._cancel_timer()
        self._unlisten(self._primary)
        self._unlisten(self._hedge)
        held = self._held
        if held is not None:
            self._held = None
            held.remove_listener("end", self._on_body_end)
        self._uncount()
        self._host.active -= 1

    # -- user API -----------------------------------------------------------
    def abort(self) -> None:
        """Abort both attempts.  Emits 'abort' and nothing further."""
        if self.aborted or self._done:
            return
        self.aborted = True
        self._finish()
        for a in (self._primary, self._hedge):
            if a is not None and not a.failed:
                a.t.abort()
        self.emit("abort")

    # -- the hedge ------------------------------------------------------------
    def _on_timer(self) -> None:
        self._timer = None
        host = self._host
        host.pending.discard(self)
        primary = self._primary
        if self._done or primary is None or primary.failed or \
                self.winner is not None:
            return
        if self._is_stopped is not None and self._is_stopped():
            return
        key = getattr(primary.t, "try_backend", None)
        if key is None:
            # still in the pool's queue: the pool is saturated, and a
            # second claim would only wait behind the first
            host.count("hedge-skipped-unclaimed")
            return
        if not host.allows():
            host.count("hedge-skipped-budget")
            return
        avoid = self._avoid if key in self._avoid else self._avoid + (key,)
        if self._has_idle is not None and not self._has_idle(avoid):
            host.count("hedge-skipped-no-idle")
            return
        try:
            self._hedge = self._begin(avoid, "hedge")
        except Exception:
            # could not be started (a stopping agent): a plain try
            return
        self.hedged = True
        self._counted = True
        host.hedging += 1
        host.count("hedge-sent")
        self.emit("hedge", self._delay_ms)

    # -- events of the attempts ---------------------------------------------
    def _on_primary_response(self, resp: Any) -> None:
        self._on_response(self._primary, self._hedge, resp)

    def _on_hedge_response(self, resp: Any) -> None:
        self._on_response(self._hedge, self._primary, resp)

    def _on_primary_error(self, err: BaseException) -> None:
        self._on_error(self._primary, self._hedge, err)

    def _on_hedge_error(self, err: BaseException) -> None:
        self._on_error(self._hedge, self._primary, err)

    def _on_response(self, a: Optional[_Attempt], other: Optional[_Attempt],
                     resp: Any) -> None:
        if self._done or a is None or self.winner is not None:
            return
        host = self._host
        now = self._loop.time()
        self.winner = a.role
        self._delivered = a
        self._cancel_timer()
        host.record((now - a.started) * 1000.0, now)
        if other is not None:
            self._unlisten(other)
            if a.role == "hedge":
                host.count("hedge-won")
            elif not other.failed:
                host.count("hedge-lost")
            if not other.failed:
                # a censored sample, a lower bound: without it slow
                # answers would drop out of the window and the
                # estimate would ratchet down
                host.record((now - other.started) * 1000.0, now)
                other.t.abort()
            self._uncount()
        self.emit("response", resp)
        if self._done:
            return
        if resp.complete:
            self._finish()
        else:
            # in flight until the body is in; an error under the body
            # surfaces as it does on a plain request
            self._held = resp
            resp.on("end", self._on_body_end)

    def _on_body_end(self) -> None:
        if self._held is not None and not self._done:
            self._finish()

    def _on_error(self, a: Optional[_Attempt], other: Optional[_Attempt],
                  err: BaseException) -> None:
        if self._done or a is None or a.failed:
            return
        a.failed = True
        if self.winner is None and other is not None and not other.failed:
            # the other attempt is still out: it decides
            self._unlisten(a)
            if a.role == "hedge":
                self._host.count("hedge-failed")
                self._uncount()
            return
        # the only attempt, the last of two to fail, or the winner
        # under its body
        self._delivered = a
        self._finish()
        self.emit("error", err)
