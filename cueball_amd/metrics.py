"""Prometheus-style metric collection (artedi equivalent).

The reference counts error events through the artedi collector
(lib/utils.js:395-444) with a fixed label set {hostname, uuid, type,
evt}; consumers may pass in a shared collector (README.adoc:113,137).
This is a small self-contained implementation with Prometheus text
exposition for scraping alongside the kang endpoint.
"""

from __future__ import annotations

import threading
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

__all__ = ["Collector", "Counter", "Gauge", "Histogram",
           "create_collector"]


def _labels_key(labels: Mapping[str, str]) -> Tuple[Tuple[str, str], ...]:
    return tuple(sorted((str(k), str(v)) for k, v in labels.items()))


class _Metric:
    kind = "untyped"

    def __init__(self, name: str, help_: str,
                 static_labels: Mapping[str, str]) -> None:
        self.name = name
        self.help = help_
        self.static_labels = dict(static_labels)
        self._values: Dict[Tuple[Tuple[str, str], ...], float] = {}
        self._lock = threading.Lock()

    def _bump(self, labels: Optional[Mapping[str, str]], delta: float,
              absolute: bool = False) -> None:
        key = _labels_key(labels or {})
        with self._lock:
            if absolute:
                self._values[key] = delta
            else:
                self._values[key] = self._values.get(key, 0.0) + delta

    def value(self, labels: Optional[Mapping[str, str]] = None) -> float:
        return self._values.get(_labels_key(labels or {}), 0.0)

    def expose(self) -> str:
        lines = [
            "# HELP %s %s" % (self.name, self.help),
            "# TYPE %s %s" % (self.name, self.kind),
        ]
        with self._lock:
            items = list(self._values.items())
        for key, val in items:
            labels = dict(self.static_labels)
            labels.update(dict(key))
            if labels:
                lstr = ",".join('%s="%s"' % (k, v)
                                for k, v in sorted(labels.items()))
                lines.append("%s{%s} %s" % (self.name, lstr, _fmt(val)))
            else:
                lines.append("%s %s" % (self.name, _fmt(val)))
        return "\n".join(lines) + "\n"


def _fmt(v: float) -> str:
    return str(int(v)) if float(v).is_integer() else repr(v)


class Counter(_Metric):
    kind = "counter"

    def increment(self, labels: Optional[Mapping[str, str]] = None,
                  delta: float = 1.0) -> None:
        if delta < 0:
            raise ValueError("counter cannot decrease")
        self._bump(labels, delta)

    add = increment


class Gauge(_Metric):
    kind = "gauge"

    def set(self, value: float,
            labels: Optional[Mapping[str, str]] = None) -> None:
        self._bump(labels, value, absolute=True)

    def add(self, delta: float,
            labels: Optional[Mapping[str, str]] = None) -> None:
        self._bump(labels, delta)


#: Prometheus client default bucket bounds
DEFAULT_BUCKETS = (0.005, 0.01, 0.025, 0.05, 0.1, 0.25, 0.5, 1.0, 2.5,
                   5.0, 10.0)


class Histogram(_Metric):
    """Prometheus histogram: per label set, one count per bucket bound
    plus the implicit ``+Inf`` bucket, a sum and a count.

    ``observe()`` counts a value under every bound ``le`` with
    ``value <= le``.  ``set_cumulative()`` replaces a label set's state
    wholesale with already-cumulative counts, for a publisher that
    keeps its own histogram and only exposes a snapshot of it.
    """

    kind = "histogram"

    def __init__(self, name: str, help_: str,
                 static_labels: Mapping[str, str],
                 buckets: Optional[Sequence[float]] = None) -> None:
        super().__init__(name, help_, static_labels)
        bounds = tuple(float(b) for b in
                       (DEFAULT_BUCKETS if buckets is None else buckets))
        if not bounds or any(b != b or b == float("inf") for b in bounds) \
                or any(a >= b for a, b in zip(bounds, bounds[1:])):
            raise ValueError("histogram buckets must be finite and "
                             "strictly increasing")
        self.buckets = bounds
        # key -> [cumulative counts per bound (+Inf excluded), sum, count]
        self._series: Dict[Tuple[Tuple[str, str], ...], list] = {}

    def observe(self, value: float,
                labels: Optional[Mapping[str, str]] = None) -> None:
        key = _labels_key(labels or {})
        value = float(value)
        with self._lock:
            ser = self._series.get(key)
            if ser is None:
                ser = self._series[key] = [[0] * len(self.buckets), 0.0, 0]
            cum = ser[0]
            for i in range(len(cum) - 1, -1, -1):
                if not value <= self.buckets[i]:
                    break
                cum[i] += 1
            ser[1] += value
            ser[2] += 1

    def set_cumulative(self, cumulative: Sequence[int], sum_: float,
                       count: int,
                       labels: Optional[Mapping[str, str]] = None) -> None:
        """Bulk setter: ``cumulative[i]`` is the number of observations
        counted under ``buckets[i]``; ``count`` is the ``+Inf`` value."""
        cum = [int(c) for c in cumulative]
        if len(cum) != len(self.buckets):
            raise ValueError("expected %d cumulative counts, got %d"
                             % (len(self.buckets), len(cum)))
        if any(a > b for a, b in zip(cum, cum[1:] + [int(count)])):
            raise ValueError("cumulative counts must not decrease")
        with self._lock:
            self._series[_labels_key(labels or {})] = \
                [cum, float(sum_), int(count)]

    def value(self, labels: Optional[Mapping[str, str]] = None) -> float:
        """The observation count of one label set."""
        ser = self._series.get(_labels_key(labels or {}))
        return float(ser[2]) if ser is not None else 0.0

    def sum(self, labels: Optional[Mapping[str, str]] = None) -> float:
        ser = self._series.get(_labels_key(labels or {}))
        return ser[1] if ser is not None else 0.0

    def expose(self) -> str:
        lines = [
            "# HELP %s %s" % (self.name, self.help),
            "# TYPE %s %s" % (self.name, self.kind),
        ]
        with self._lock:
            items = [(k, list(v[0]), v[1], v[2])
                     for k, v in self._series.items()]
        for key, cum, total, count in items:
            labels = dict(self.static_labels)
            labels.update(dict(key))
            base = ['%s="%s"' % (k, v) for k, v in sorted(labels.items())]
            bounds: List[Tuple[str, int]] = [
                (repr(b), c) for b, c in zip(self.buckets, cum)]
            bounds.append(("+Inf", count))
            for le, c in bounds:
                lines.append("%s_bucket{%s} %d" % (
                    self.name, ",".join(base + ['le="%s"' % le]), c))
            suffix = "{%s}" % ",".join(base) if base else ""
            lines.append("%s_sum%s %s" % (self.name, suffix, _fmt(total)))
            lines.append("%s_count%s %d" % (self.name, suffix, count))
        return "\n".join(lines) + "\n"


class Collector:
    """Registry of named metrics; ``counter()``/``gauge()``/
    ``histogram()`` are idempotent (lib/utils.js:407-411 relies on
    re-registration being harmless)."""

    def __init__(self, labels: Optional[Mapping[str, str]] = None) -> None:
        self.labels = dict(labels or {})
        self._metrics: Dict[str, _Metric] = {}
        self._lock = threading.Lock()

    def _register(self, cls, name: str, help_: str, **kw) -> _Metric:
        with self._lock:
            m = self._metrics.get(name)
            if m is not None:
                if not isinstance(m, cls):
                    raise ValueError("metric %r already registered with a "
                                     "different type" % name)
                return m
            m = cls(name, help_, self.labels, **kw)
            self._metrics[name] = m
            return m

    def counter(self, *, name: str, help: str = "") -> Counter:
        return self._register(Counter, name, help)  # type: ignore[return-value]

    def gauge(self, *, name: str, help: str = "") -> Gauge:
        return self._register(Gauge, name, help)  # type: ignore[return-value]

    def histogram(self, *, name: str, help: str = "",
                  buckets: Optional[Sequence[float]] = None) -> Histogram:
        """The first registration fixes the buckets; later calls with
        the same name return that histogram unchanged."""
        return self._register(Histogram, name, help,  # type: ignore[return-value]
                              buckets=buckets)

    def get_collector(self, name: str) -> _Metric:
        return self._metrics[name]

    def collect(self) -> str:
        """Prometheus text exposition of every metric."""
        return "".join(m.expose() for m in self._metrics.values())


def create_collector(labels: Optional[Mapping[str, str]] = None) -> Collector:
    return Collector(labels=labels)
