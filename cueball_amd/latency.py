"""Claim-latency histograms.

``LatencyHistogram`` is a fixed-layout log-linear histogram over integer
microseconds: values 0..15 us get a bucket each, and above that every
octave ``[2**e, 2**(e+1))`` is cut into 8 equal sub-buckets, so a bucket
is at most 12.5 % wide.  272 regular buckets cover ``[0, 2**36)`` us
(about 19 hours); one overflow bucket takes the rest (larger values,
``nan``, ``inf``), which saturate at ``2**36`` us in ``sum``/``min``/
``max``.  Recording is O(1) and never allocates.

Input is milliseconds (the unit of ``ClaimHandle.ch_started``),
converted once with round-to-nearest; negative values clamp to 0.  All
state is integer, so the native core (``_speed.LatencyHistogram``,
arithmetic in ``_native/lathist.h``) and the pure class here agree
exactly.

``PoolLatency`` bundles the three per-pool histograms (claim wait,
claim hold, connect) with the clock the claim handle reads.
"""

from __future__ import annotations

import asyncio
import math
import os as _os
from typing import Any, Dict, List, Optional

__all__ = ["LatencyHistogram", "PoolLatency", "bucket_index",
           "bucket_lower_bound", "EXPOSITION_BOUNDS_US", "NBUCKETS",
           "OVERFLOW_INDEX"]

_LINEAR = 16
_MAX_BITS = 36
_LIMIT_US = 1 << _MAX_BITS
#: regular buckets (272) + the overflow bucket
NBUCKETS = _LINEAR + (_MAX_BITS - 4) * 8 + 1
OVERFLOW_INDEX = NBUCKETS - 1

#: Prometheus ``le`` bounds published by the pool: 4**k us, k = 2..13
#: (16 us .. ~67 s).  Each one is an internal bucket boundary, so the
#: exposed cumulative counts are exact.
EXPOSITION_BOUNDS_US = tuple(4 ** k for k in range(2, 14))


def bucket_index(us: int) -> int:
    """Bucket of an integer microsecond value (negative clamps to 0)."""
    if us < _LINEAR:
        return us if us > 0 else 0
    if us >= _LIMIT_US:
        return OVERFLOW_INDEX
    e = us.bit_length() - 1
    return _LINEAR + (e - 4) * 8 + ((us >> (e - 3)) & 7)


def bucket_lower_bound(idx: int) -> int:
    """Inclusive lower edge (us) of bucket ``idx``; for the overflow
    index this is ``2**36``, the upper edge of the last regular one."""
    if idx < _LINEAR:
        return idx
    k = idx - _LINEAR
    return (8 + k % 8) << (k // 8 + 1)


def _to_us(ms: float) -> int:
    if not math.isfinite(ms):
        return _LIMIT_US
    x = ms * 1000.0
    if x <= 0.0:
        return 0
    if not x < _LIMIT_US:
        return _LIMIT_US
    # round half away from zero, like llround (x - f is exact)
    f = math.floor(x)
    us = int(f) + (1 if x - f >= 0.5 else 0)
    return us if us < _LIMIT_US else _LIMIT_US


class LatencyHistogram:
    __slots__ = ("_counts", "_count", "_sum_us", "_min_us", "_max_us")

    def __init__(self) -> None:
        self._counts = [0] * NBUCKETS
        self._count = 0
        self._sum_us = 0
        self._min_us = 0
        self._max_us = 0

    def record(self, ms: float) -> None:
        us = _to_us(ms)
        self._counts[bucket_index(us)] += 1
        if self._count == 0 or us < self._min_us:
            self._min_us = us
        if us > self._max_us:
            self._max_us = us
        self._count += 1
        self._sum_us += us

    @property
    def count(self) -> int:
        return self._count

    @property
    def sum_us(self) -> int:
        return self._sum_us

    @property
    def sum_ms(self) -> float:
        return self._sum_us / 1000.0

    @property
    def min_ms(self) -> Optional[float]:
        return self._min_us / 1000.0 if self._count else None

    @property
    def max_ms(self) -> Optional[float]:
        return self._max_us / 1000.0 if self._count else None

    def counts(self) -> List[int]:
        return list(self._counts)

    def percentile(self, q: float) -> Optional[float]:
        """Nearest rank: the exclusive upper edge (ms) of the first
        bucket whose cumulative count reaches ``ceil(q*count)``, clamped
        to ``max_ms``; ``None`` when empty."""
        n = self._count
        if n == 0:
            return None
        q = float(q)
        if not q > 0.0:
            q = 0.0
        if q > 1.0:
            q = 1.0
        rank = int(math.ceil(q * float(n)))
        rank = min(max(rank, 1), n)
        cum = 0
        counts = self._counts
        for i in range(OVERFLOW_INDEX):
            cum += counts[i]
            if cum >= rank:
                return min(bucket_lower_bound(i + 1), self._max_us) / 1000.0
        return self._max_us / 1000.0

    def cumulative(self, bounds_us) -> List[int]:
        """For each bound (us, a bucket boundary): how many samples have
        a rounded microsecond value strictly below it."""
        counts = self._counts
        return [sum(counts[:bucket_index(int(b))]) for b in bounds_us]

    def merge(self, other: "LatencyHistogram") -> None:
        oc = other.counts()
        n = other.count
        if n == 0:
            return
        omin = _to_us(other.min_ms)
        omax = _to_us(other.max_ms)
        for i in range(NBUCKETS):
            self._counts[i] += oc[i]
        if self._count == 0 or omin < self._min_us:
            self._min_us = omin
        if omax > self._max_us:
            self._max_us = omax
        self._count += n
        self._sum_us += other.sum_us

    def reset(self) -> None:
        self.__init__()

    def snapshot(self) -> Dict[str, Any]:
        return {
            "count": self._count,
            "sumMs": self.sum_ms,
            "minMs": self.min_ms,
            "maxMs": self.max_ms,
            "p50": self.percentile(0.5),
            "p90": self.percentile(0.9),
            "p99": self.percentile(0.99),
            "p999": self.percentile(0.999),
        }


class PoolLatency:
    """The three histograms of one pool plus the claim handle's clock.

    ``direct`` is decided once per pool: when the loop's ``time`` is the
    stock ``asyncio.BaseEventLoop.time`` the native claim handle reads
    the monotonic clock itself instead of calling into Python; any
    other loop (virtual clocks, foreign loops) is asked via
    ``loop.time()``.
    """

    __slots__ = ("wait", "hold", "connect", "loop", "direct")

    def __init__(self, loop: Any) -> None:
        self.wait = LatencyHistogram()
        self.hold = LatencyHistogram()
        self.connect = LatencyHistogram()
        self.loop = loop
        self.direct = stock_clock(loop)


def stock_clock(loop: Any) -> bool:
    """True when ``loop.time`` is asyncio's own monotonic-clock read."""
    return (getattr(type(loop), "time", None) is asyncio.BaseEventLoop.time
            and "time" not in getattr(loop, "__dict__", ()))


# ---------------------------------------------------------------------------
# Native core: _speed.LatencyHistogram / _speed.PoolLatency replace the
# pure classes above when the extension is built (same arithmetic, from
# _native/lathist.h; CUEBALL_PURE=1 forces the Python classes).
PurePythonLatencyHistogram = LatencyHistogram
PurePythonPoolLatency = PoolLatency

if not _os.environ.get("CUEBALL_PURE"):
    try:
        from ._speed import LatencyHistogram  # type: ignore # noqa: F811
        from ._speed import PoolLatency as _NativePoolLatency

        def PoolLatency(loop: Any):  # type: ignore # noqa: F811
            return _NativePoolLatency(loop, stock_clock(loop))
    except ImportError:
        pass
