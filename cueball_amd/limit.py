"""Adaptive concurrency limiting: the arithmetic, and nothing else.

A pool created with ``concurrencyLimit`` asks this module how many
leases it may have in flight.  Everything here is a function of what the
pool hands in (times in ms on the pool's clock): no pool, no loop, no
timers.  The gate, the lease timing and the bookkeeping live in
``cueball_amd.pool``.

The limiter is told when a lease starts (``on_start``) and how it ended:
with a hold time (``on_sample``) or without one (``on_discard``, a lease
that failed: a service that fails fast must not look fast).  All of its
decisions are taken lazily inside ``on_sample``.  Samples are gathered
into windows; a window closes at the first sample for which ``now -
opened >= window`` and ``count >= minSamples``, and the limit moves once
per closed window.

A sample counts only if its lease began under the ``allowed()`` in
force now.  A lease that began before the integer last changed (the
limit moved, a probe began or ended) ran at the load of the old one:
after a back-off those are the slowest leases of all, they arrive
first, and counting them makes the controller answer one overload
twice (what TCP avoids by reducing once per window of data).  Such
samples are dropped, and counted as ``discarded``.

``"aimd"`` compares the window's mean hold time with a threshold the
operator names: over it, the limit is multiplied by ``backoffRatio``;
under it, and only if the window's peak in-flight reached the limit, it
grows by one.  A client that does not use its limit learns nothing about
the service and must not talk itself up.

``"gradient"`` (Envoy's adaptive-concurrency controller, adapted) needs
no threshold: it compares the mean with a *baseline*, the hold time of
the service when it is not loaded, and aims at ``tolerance`` times that.

Why the baseline is probed and not learned as a minimum.  The obvious
baseline is the smallest window mean seen lately (a sliding-window
minimum, as Netflix's gradient limiters keep).  Under exactly the
condition this limiter exists for, a service that stays saturated, every
window in the slide is an inflated one: once the last honest window has
left it, the minimum *is* the saturated latency, the gradient reads 1,
and the limit climbs back to ``maxLimit`` one baseline window after it
came down.  So the baseline is measured instead: the limiter starts in
a *probe* and enters one again every ``probeInterval`` ms, during which
the pool may carry only ``probeLimit`` leases; the mean hold time of
leases that began inside the probe is the new baseline.

What a probe costs: for at most ``window`` ms (less once ``probeSamples``
leases have come back) out of every ``probeInterval`` ms the pool runs
at ``probeLimit`` leases, whatever the limit; claims beyond that wait in
the pool's queue, subject to its bounds, timeouts and CoDel.  With the
defaults that is at most 1 s in 30 s at 3 leases.  ``limit`` itself is
untouched by a probe.  ``probeSpread`` shortens each interval by a
random fraction so that a fleet of clients does not probe in step.
"""

from __future__ import annotations

import math
import random as mod_random
from typing import Any, Mapping, Optional, Tuple

__all__ = ["ConcurrencyLimiter", "ALGORITHMS"]

ALGORITHMS = ("gradient", "aimd")


class ConcurrencyLimiter:
    """One limit.  `cfg` is the validated option, every default filled in
    (``utils.assert_concurrency_limit``)."""

    __slots__ = ("cfg", "algorithm", "limit", "in_flight", "peak",
                 "opened", "win_sum", "win_count", "baseline", "probing",
                 "epoch", "probe_at", "probe_sum", "probe_count",
                 "probe_next", "probe_limit", "last_mean", "windows",
                 "probes", "samples", "discarded", "raised", "lowered",
                 "_rnd")

    def __init__(self, cfg: Mapping[str, Any]) -> None:
        self.cfg = cfg
        self.algorithm = cfg["algorithm"]
        self.limit = float(cfg["initialLimit"])
        #: leases started and not ended, and the most at once this window
        self.in_flight = 0
        self.peak = 0
        #: when the window opened; None until the first lease starts
        self.opened: Optional[float] = None
        self.win_sum = 0.0
        self.win_count = 0
        self.baseline: Optional[float] = None
        self.probing = False
        #: counts the changes of allowed(); a lease's token carries the
        #: value at its start
        self.epoch = 0
        #: when the probe began; None for the first until a lease starts
        self.probe_at: Optional[float] = None
        self.probe_sum = 0.0
        self.probe_count = 0
        self.probe_next = math.inf
        self.probe_limit = 0
        self.last_mean: Optional[float] = None
        self.windows = 0
        self.probes = 0
        self.samples = 0
        self.discarded = 0
        self.raised = 0
        self.lowered = 0
        rnd = cfg.get("random")
        self._rnd = (rnd if rnd is not None else mod_random).random
        if self.algorithm == "gradient":
            self.probe_limit = int(min(max(cfg["probeLimit"],
                                           cfg["minLimit"]),
                                       cfg["maxLimit"]))
            # the limiter starts in a probe: no baseline, no gradient
            self.probing = True
            self.probes = 1

    # -- what the pool reads ------------------------------------------------
    def allowed(self) -> int:
        """The leases a pool may have in flight right now."""
        if self.probing:
            return self.probe_limit
        return int(math.floor(self.limit))

    # -- what the pool reports ----------------------------------------------
    def on_start(self, now_ms: float) -> Tuple[float, int]:
        if self.opened is None:
            self.opened = now_ms
            if self.probing:
                # the first probe's clock starts with the first lease
                self.probe_at = now_ms
                self.probe_next = self._probe_after(now_ms)
        self.in_flight += 1
        if self.in_flight > self.peak:
            self.peak = self.in_flight
        return (now_ms, self.epoch)

    def on_discard(self, token: Tuple[float, int]) -> None:
        self.in_flight -= 1
        self.discarded += 1

    def on_sample(self, token: Tuple[float, int], hold_ms: float,
                  now_ms: float) -> bool:
        """A lease ended well, after `hold_ms`.  Returns whether the
        limit changed (``allowed()`` may change without it, at either
        end of a probe)."""
        self.in_flight -= 1
        fresh = token[1] == self.epoch
        if fresh:
            self.samples += 1
        else:
            # began under another allowed(), at whatever load that made
            self.discarded += 1
        cfg = self.cfg
        if self.probing:
            if fresh:
                self.probe_sum += hold_ms
                self.probe_count += 1
            if self.probe_count >= cfg["probeSamples"] or \
                    now_ms - self.probe_at >= cfg["window"]:
                self._probe_end(now_ms)
            return False
        if fresh:
            self.win_sum += hold_ms
            self.win_count += 1
        changed = False
        if now_ms - self.opened >= cfg["window"] and \
                self.win_count >= cfg["minSamples"]:
            changed = self._window_close(now_ms)
        if now_ms >= self.probe_next:
            self._probe_begin(now_ms)
        return changed

    # -- windows ------------------------------------------------------------
    def _window_open(self, now_ms: float) -> None:
        self.opened = now_ms
        self.win_sum = 0.0
        self.win_count = 0
        self.peak = self.in_flight

    def _window_close(self, now_ms: float) -> bool:
        cfg = self.cfg
        mean = self.win_sum / self.win_count
        peak = self.peak
        limit = self.limit
        self.last_mean = mean
        self.windows += 1
        self._window_open(now_ms)
        if self.algorithm == "aimd":
            if mean > cfg["latencyThreshold"]:
                new = limit * cfg["backoffRatio"]
            elif peak >= math.floor(limit):
                new = limit + 1
            else:
                new = limit
        else:
            g = cfg["tolerance"] * self.baseline / mean if mean > 0 else 1.0
            g = min(max(g, 0.5), 1.0)
            new = limit * g + math.sqrt(limit)
            if new > limit and peak < limit / 2:
                new = limit         # app-limited: nothing was learned
            else:
                s = cfg["smoothing"]
                new = limit * (1 - s) + new * s
        new = min(max(new, float(cfg["minLimit"])), float(cfg["maxLimit"]))
        if new == limit:
            return False
        if new > limit:
            self.raised += 1
        else:
            self.lowered += 1
        self.limit = new
        if math.floor(new) != math.floor(limit):
            self.epoch += 1
        return True

    # -- probes (gradient) --------------------------------------------------
    def _probe_begin(self, now_ms: float) -> None:
        self.probing = True
        self.epoch += 1
        self.probes += 1
        self.probe_at = now_ms
        self.probe_sum = 0.0
        self.probe_count = 0
        self.probe_next = self._probe_after(now_ms)

    def _probe_after(self, now_ms: float) -> float:
        cfg = self.cfg
        return now_ms + cfg["probeInterval"] * \
            (1.0 - cfg["probeSpread"] * self._rnd())

    def _probe_end(self, now_ms: float) -> None:
        if self.probe_count > 0:
            self.baseline = self.probe_sum / self.probe_count
        elif self.baseline is None:
            return                  # at startup: nothing to go by yet
        self.probing = False
        self.epoch += 1
        self._window_open(now_ms)
