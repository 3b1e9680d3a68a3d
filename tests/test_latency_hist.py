"""LatencyHistogram (pure and native) and the generic metrics.Histogram.

The bucket layout is fixed, so every expectation here is worked out from
the layout itself: values 0..15 us one bucket each, then 8 sub-buckets
per octave up to 2**36 us, then one overflow bucket.
"""

import math
import random

import pytest

from cueball_amd import latency
from cueball_amd import metrics
from cueball_amd.latency import (NBUCKETS, OVERFLOW_INDEX,
                                 PurePythonLatencyHistogram, bucket_index,
                                 bucket_lower_bound)
from cueball_amd.testing import VirtualLoop

try:
    from cueball_amd import _speed
except ImportError:  # pragma: no cover
    _speed = None

IMPLS = [PurePythonLatencyHistogram]
if _speed is not None:
    IMPLS.append(_speed.LatencyHistogram)

impl = pytest.mark.parametrize(
    "Hist", IMPLS, ids=lambda c: "native" if c.__module__.endswith("_speed")
    else "pure")


def only_bucket(h):
    """Index of the single occupied bucket."""
    counts = h.counts()
    assert len(counts) == NBUCKETS == 273
    assert sum(counts) == 1
    return counts.index(1)


def test_layout_round_trip():
    assert OVERFLOW_INDEX == 272
    for i in range(OVERFLOW_INDEX):
        assert bucket_index(bucket_lower_bound(i)) == i
        assert bucket_index(bucket_lower_bound(i + 1) - 1) == i
    assert bucket_lower_bound(OVERFLOW_INDEX) == 2 ** 36
    # at most 12.5 % wide above the linear range
    for i in range(16, OVERFLOW_INDEX):
        lo, hi = bucket_lower_bound(i), bucket_lower_bound(i + 1)
        assert (hi - lo) * 8 <= lo


@impl
def test_recorded_round_trip(Hist):
    """The same round trip through record(): both edges of every
    regular bucket land in it."""
    h = Hist()
    for i in range(OVERFLOW_INDEX):
        h.record(bucket_lower_bound(i) / 1000.0)
        h.record((bucket_lower_bound(i + 1) - 1) / 1000.0)
    counts = h.counts()
    # buckets 0..15 are one value wide: both edges are the same value
    assert counts == [2] * OVERFLOW_INDEX + [0]


SPOTS = [
    (0, 0), (1, 1), (15, 15), (16, 16), (17, 16), (30, 23), (31, 23),
    (32, 24), (2 ** 36 - 1, 271), (2 ** 36, 272),
]


@impl
@pytest.mark.parametrize("us,idx", SPOTS)
def test_spot_values(Hist, us, idx):
    assert bucket_index(us) == idx
    h = Hist()
    h.record(us / 1000.0)
    assert only_bucket(h) == idx


@impl
def test_negative_nan_inf(Hist):
    h = Hist()
    h.record(-5.0)
    assert only_bucket(h) == 0
    assert h.min_ms == 0.0 and h.max_ms == 0.0 and h.sum_ms == 0.0
    for bad in (float("nan"), float("inf"), 1e300):
        h = Hist()
        h.record(bad)
        assert only_bucket(h) == OVERFLOW_INDEX
        assert h.count == 1
        # overflow samples saturate at 2**36 us
        assert h.max_ms == 2 ** 36 / 1000.0
        assert h.percentile(0.5) == h.max_ms


@impl
def test_rounds_to_nearest(Hist):
    """Virtual-clock times near 1e9 ms are not exact in binary; the
    conversion must round, not truncate."""
    b3000 = bucket_index(3000)
    assert bucket_lower_bound(b3000) <= 3000 < bucket_lower_bound(b3000 + 1)

    h = Hist()
    h.record(1_000_000_003.0 - 1_000_000_000.0)
    assert only_bucket(h) == b3000
    assert h.sum_ms == 3.0

    # the virtual-clock analogue: seconds near 1e6, scaled to ms
    def vt_elapsed_ms(seconds):
        loop = VirtualLoop()
        try:
            t0 = loop.time()
            loop._vt_set(t0 + seconds)
            return (loop.time() - t0) * 1000.0
        finally:
            loop.close()

    ms = vt_elapsed_ms(0.003)
    assert ms != 3.0                    # inexact in binary
    h = Hist()
    h.record(ms)
    assert only_bucket(h) == b3000
    assert h.sum_ms == 3.0              # rounded to 3000 us

    # 4 ms comes out a hair under: truncation would store 3999 us
    ms = vt_elapsed_ms(0.004)
    assert ms < 4.0 and int(ms * 1000.0) == 3999
    h = Hist()
    h.record(ms)
    assert only_bucket(h) == bucket_index(4000)
    assert h.sum_ms == 4.0 and h.max_ms == 4.0


QS = (0.5, 0.9, 0.99, 0.999, 1.0)


def log_uniform_ms(n, seed=0):
    rng = random.Random(seed)
    lo, hi = math.log(1e-3), math.log(1e5)   # 1 us .. 100 s, in ms
    return [math.exp(rng.uniform(lo, hi)) for _ in range(n)]


@pytest.mark.skipif(_speed is None, reason="native core not built")
def test_native_pure_parity():
    a = PurePythonLatencyHistogram()
    b = _speed.LatencyHistogram()
    for ms in log_uniform_ms(10_000):
        a.record(ms)
        b.record(ms)
    assert a.counts() == b.counts()
    assert a.count == b.count == 10_000
    assert a.sum_ms == b.sum_ms
    assert a.min_ms == b.min_ms
    assert a.max_ms == b.max_ms
    for q in QS:
        assert a.percentile(q) == b.percentile(q)
    assert a.snapshot() == b.snapshot()
    bounds = latency.EXPOSITION_BOUNDS_US
    assert a.cumulative(bounds) == b.cumulative(bounds)


@impl
def test_percentile_rules(Hist):
    h = Hist()
    assert h.percentile(0.5) is None
    assert h.min_ms is None and h.max_ms is None
    assert h.snapshot() == {"count": 0, "sumMs": 0.0, "minMs": None,
                            "maxMs": None, "p50": None, "p90": None,
                            "p99": None, "p999": None}
    # one sample: that sample, whatever q
    h.record(3.3)
    for q in (0.0, 0.001, 0.5, 0.999, 1.0):
        assert h.percentile(q) == 3.3

    # nearest rank over a known set: 100 samples, 1..100 ms
    h = Hist()
    for ms in range(1, 101):
        h.record(float(ms))
    assert h.count == 100 and h.sum_ms == 5050.0
    assert h.min_ms == 1.0 and h.max_ms == 100.0
    assert h.percentile(1.0) == h.max_ms == 100.0
    for q in (0.01, 0.5, 0.9, 0.99):
        # the rank-th smallest sample is rank ms; the answer is its
        # bucket's exclusive upper edge
        rank = math.ceil(q * 100)
        us = rank * 1000
        want = bucket_lower_bound(bucket_index(us) + 1) / 1000.0
        got = h.percentile(q)
        assert got == min(want, 100.0)
        assert us / 1000.0 < got <= us / 1000.0 * 1.125


@impl
def test_merge_and_reset(Hist):
    vals = log_uniform_ms(2000, seed=1)
    whole, left, right = Hist(), Hist(), Hist()
    for i, ms in enumerate(vals):
        whole.record(ms)
        (left if i < 1000 else right).record(ms)
    left.merge(right)
    assert left.counts() == whole.counts()
    assert left.count == whole.count
    assert left.sum_ms == whole.sum_ms
    assert left.min_ms == whole.min_ms and left.max_ms == whole.max_ms
    for q in QS:
        assert left.percentile(q) == whole.percentile(q)
    # merging an empty one changes nothing, merging into an empty one
    # copies
    left.merge(Hist())
    assert left.snapshot() == whole.snapshot()
    empty = Hist()
    empty.merge(whole)
    assert empty.snapshot() == whole.snapshot()
    whole.reset()
    assert whole.count == 0 and sum(whole.counts()) == 0
    assert whole.percentile(0.5) is None


def test_selected_implementation(monkeypatch):
    """latency.LatencyHistogram is the native type whenever the core is
    built and CUEBALL_PURE is unset (the queue.py/codel.py rule)."""
    import os
    if _speed is not None and not os.environ.get("CUEBALL_PURE"):
        assert latency.LatencyHistogram is _speed.LatencyHistogram
    else:
        assert latency.LatencyHistogram is PurePythonLatencyHistogram


# -- generic Prometheus histogram -----------------------------------------

def bucket_lines(text, name):
    out = []
    for line in text.splitlines():
        if line.startswith(name + "_bucket{"):
            le = line.split('le="')[1].split('"')[0]
            out.append((le, int(line.rsplit(" ", 1)[1])))
    return out


def test_histogram_exposition():
    c = metrics.create_collector()
    h = c.histogram(name="req_seconds", help="request time",
                    buckets=[0.1, 1.0, 10.0])
    h.observe(0.05)
    h.observe(0.5)
    h.observe(20.0)
    text = c.collect()
    assert "# TYPE req_seconds histogram" in text
    assert "# HELP req_seconds request time" in text
    assert bucket_lines(text, "req_seconds") == [
        ("0.1", 1), ("1.0", 2), ("10.0", 2), ("+Inf", 3)]
    lines = text.splitlines()
    assert "req_seconds_count 3" in lines
    assert "req_seconds_sum 20.55" in lines
    assert lines.index('req_seconds_bucket{le="+Inf"} 3') < \
        lines.index("req_seconds_sum 20.55") < \
        lines.index("req_seconds_count 3")

    # idempotent registration; a type clash raises
    assert c.histogram(name="req_seconds") is h
    with pytest.raises(ValueError):
        c.counter(name="req_seconds")
    c.counter(name="hits")
    with pytest.raises(ValueError):
        c.histogram(name="hits")


def test_histogram_labels_and_bulk_set():
    c = metrics.create_collector({"svc": "x"})
    h = c.histogram(name="t_seconds", buckets=[1.0, 2.0])
    h.observe(1.0, {"pool": "a"})       # le is inclusive in observe()
    h.observe(1.5, {"pool": "b"})
    h.set_cumulative([4, 6], 9.5, 7, {"pool": "a"})   # replaces pool=a
    lines = c.collect().splitlines()
    assert 't_seconds_bucket{pool="a",svc="x",le="1.0"} 4' in lines
    assert 't_seconds_bucket{pool="a",svc="x",le="2.0"} 6' in lines
    assert 't_seconds_bucket{pool="a",svc="x",le="+Inf"} 7' in lines
    assert 't_seconds_sum{pool="a",svc="x"} 9.5' in lines
    assert 't_seconds_count{pool="a",svc="x"} 7' in lines
    assert 't_seconds_bucket{pool="b",svc="x",le="1.0"} 0' in lines
    assert 't_seconds_bucket{pool="b",svc="x",le="2.0"} 1' in lines
    assert h.value({"pool": "a"}) == 7
    with pytest.raises(ValueError):
        h.set_cumulative([1], 0.0, 1)           # wrong length
    with pytest.raises(ValueError):
        h.set_cumulative([3, 2], 0.0, 3)        # not cumulative
    with pytest.raises(ValueError):
        c.histogram(name="bad", buckets=[2.0, 1.0])
