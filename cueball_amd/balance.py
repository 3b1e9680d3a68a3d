"""Latency-aware claim balancing: the arithmetic, and nothing else.

A pool created with ``claimBalancing`` asks this module which of its
idle connections a claim should get.  Everything here is a pure
function of what the pool hands in (times in ms on the pool's clock,
per-backend counts); the queue walk, the lease timing and the
bookkeeping live in ``cueball_amd.pool``.

The estimate is a peak-sensitive EWMA, as in Finagle's balancer: a
sample above the stored value replaces it at once, a sample below it
pulls it down only as fast as time has passed.  A backend that turns
slow is noticed after one lease; one that turned fast again has to
prove it.  The stored value also ages while no sample arrives, so that
a backend which was slow once and has been shunned since becomes
eligible again: after ``decay_ms * ln(r)`` it undercuts a backend `r`
times faster.

The cost of a backend is ``estimate * (outstanding + 1)``: what the
next request should expect to wait behind the leases already there.
"""

from __future__ import annotations

import math
from typing import (Any, Dict, Iterable, Mapping, Optional, Sequence,
                    Tuple)

__all__ = ["PeakEwma", "BackendLoad", "POLICIES", "backend_costs", "pick"]

POLICIES = ("peakEwma", "leastLoaded")


class PeakEwma:
    """One latency estimate."""

    __slots__ = ("decay_ms", "value", "last")

    def __init__(self, decay_ms: float) -> None:
        self.decay_ms = float(decay_ms)
        self.value: Optional[float] = None
        self.last = 0.0

    def observe(self, sample_ms: float, now_ms: float) -> None:
        value = self.value
        if value is None or sample_ms > value:
            # the first sample, or a peak
            self.value = sample_ms
        else:
            w = math.exp(-(now_ms - self.last) / self.decay_ms)
            self.value = value * w + sample_ms * (1.0 - w)
        self.last = now_ms

    def get(self, now_ms: float) -> Optional[float]:
        """The estimate aged to `now_ms`; None before the first sample."""
        value = self.value
        if value is None:
            return None
        return value * math.exp(-(now_ms - self.last) / self.decay_ms)


class BackendLoad:
    """What a pool keeps per backend key."""

    __slots__ = ("ewma", "outstanding", "leases", "failed", "picked")

    def __init__(self, decay_ms: float) -> None:
        self.ewma = PeakEwma(decay_ms)
        #: slots handed to a claim or serving a lease
        self.outstanding = 0
        #: leases that ended, the failed ones included
        self.leases = 0
        self.failed = 0
        #: claims the balancer gave to this backend
        self.picked = 0


def backend_costs(loads: Mapping[str, Any], now_ms: float,
                  policy: str = "peakEwma",
                  keys: Optional[Iterable[str]] = None) -> Dict[str, float]:
    """``{key: estimate * (outstanding + 1)}`` for the backends `keys`
    (default: all) of `loads` (key -> an object with ``ewma`` and
    ``outstanding``, every backend of the pool).

    Under ``"leastLoaded"`` the estimate is 1.0 throughout.  Under
    ``"peakEwma"`` it is the backend's aged value; a backend without
    one borrows the lowest aged value among all of `loads` that have one
    (so it ties with the best and gets explored, but is never preferred
    over it), and 1.0 when no backend has one."""
    if keys is None:
        keys = loads
    if policy == "leastLoaded":
        return {k: float(loads[k].outstanding + 1) for k in keys}
    out: Dict[str, float] = {}
    fallback: Optional[float] = None
    for k in keys:
        ld = loads[k]
        est = ld.ewma.get(now_ms)
        if est is None:
            if fallback is None:
                known = [v for v in (o.ewma.get(now_ms)
                                     for o in loads.values())
                         if v is not None]
                fallback = min(known) if known else 1.0
            est = fallback
        out[k] = est * (ld.outstanding + 1)
    return out


def pick(candidates: Sequence[Tuple[Any, float]]) -> Any:
    """The cheapest of `candidates`, ``(item, cost)`` pairs in queue
    order; a tie goes to the earliest.  With equal costs this is the
    head of the queue: plain FIFO."""
    best, best_cost = candidates[0]
    for item, cost in candidates:
        if cost < best_cost:
            best, best_cost = item, cost
    return best
