"""``HedgeHost``'s windowed latency estimate, on an injected clock:
the percentile and its clamp, ``minSamples``, the lazy rotation of the
two half-windows, and the cache of the percentile walk."""

import pytest

from cueball_amd import latency as mod_latency
from cueball_amd.hedge import COUNTERS, HedgeHost
from hedge_kit import policy_of


class Clock:
    """Seconds, like a loop's; kept in whole microseconds so that a
    tick of exactly one window is exactly one window."""

    def __init__(self):
        self.us = 100 * 1000000

    def __call__(self):
        return self.us / 1e6

    @property
    def now(self):
        return self()

    def tick(self, ms):
        self.us += round(ms * 1000)


def host_of(clock=None, histogram=None, **hedge):
    clock = clock or Clock()
    return HedgeHost("svc", policy_of(**hedge), clock,
                     histogram=histogram), clock


#: 1..200 ms, shuffled by a fixed stride
VALUES = [((i * 37) % 200) + 1 for i in range(200)]


def reference(values, q):
    h = mod_latency.LatencyHistogram()
    for v in values:
        h.record(v)
    return h.percentile(q)


@pytest.mark.parametrize("pct", [50, 95, 99.9])
def test_delay_is_the_percentile_of_the_recorded_values(pct):
    host, clock = host_of(percentile=pct)
    for v in VALUES:
        host.record(v)
    want = reference(VALUES, pct / 100.0)
    assert 1 < want < 1000
    assert host.delay() == want
    assert host.delay(clock.now) == want
    assert host.samples() == len(VALUES)
    st = host.stats()
    assert st["delayMs"] == want and st["samples"] == len(VALUES)
    assert st["latency"]["count"] == len(VALUES)
    assert st["latency"]["maxMs"] == 200.0
    assert st["counters"] == dict.fromkeys(COUNTERS, 0)


def test_delay_is_clamped():
    want = reference(VALUES, 0.95)
    host, _ = host_of(minDelay=want + 50, maxDelay=want + 60)
    for v in VALUES:
        host.record(v)
    assert host.delay() == want + 50
    host, _ = host_of(minDelay=2, maxDelay=want - 50)
    for v in VALUES:
        host.record(v)
    assert host.delay() == want - 50


def test_a_per_call_policy_reads_the_same_window():
    host, _ = host_of(percentile=95)
    for v in VALUES:
        host.record(v)
    p50 = policy_of(percentile=50, maxDelay=80)
    assert host.delay(None, p50) == min(80, reference(VALUES, 0.5))
    assert host.delay() == reference(VALUES, 0.95)


def test_none_below_min_samples():
    host, _ = host_of(minSamples=5)
    assert host.delay() is None and host.stats()["delayMs"] is None
    for n in range(4):
        host.record(10)
        assert host.delay() is None
    host.record(10)
    assert host.delay() == reference([10] * 5, 0.95)


def test_a_fixed_delay_is_what_stats_report():
    host, _ = host_of(delay=20)
    assert host.stats()["delayMs"] == 20
    assert host.stats()["limit"] == 1


def test_rotation():
    """window 1000: a sample counts for at least one window and at
    most two."""
    host, clock = host_of(window=1000, minSamples=1)
    host.record(500)                        # t = 0, the slow one
    clock.tick(400)
    assert host.delay() == reference([500], 0.95)
    clock.tick(600)                         # t = 1000: first rotation
    host.record(10)
    assert host.samples() == 2
    assert host.previous.count == 1 and host.current.count == 1
    # older than the window, and it still counts
    clock.tick(500)                         # t = 1500
    assert host.delay() == reference([500, 10], 0.95)
    assert host.delay() == 500
    clock.tick(500)                         # t = 2000: second rotation
    assert host.delay() == reference([10], 0.95)
    assert host.samples() == 1
    assert host.previous.count == 1 and host.current.count == 0
    clock.tick(1000)                        # t = 3000: third
    assert host.delay() is None and host.samples() == 0


def test_everything_is_gone_after_two_windows_without_a_call():
    host, clock = host_of(window=1000, minSamples=1)
    host.record(500)
    clock.tick(999)
    host.record(400)
    clock.tick(1001)                        # 2 x window since the start
    assert host.samples() == 2              # nobody has looked yet
    assert host.delay() is None
    assert host.samples() == 0
    host.record(7)                          # and the window starts over
    assert host.current.count == 1 and host.previous.count == 0
    clock.tick(150)
    assert host.delay() == 7


def test_record_rotates_too():
    host, clock = host_of(window=1000, minSamples=1)
    host.record(500)
    clock.tick(1000)
    host.record(10)
    assert host.previous.count == 1 and host.current.count == 1
    clock.tick(1000)
    host.record(20)
    assert host.previous.count == 1 and host.current.count == 1
    assert host.delay() == reference([10, 20], 0.95)


class CountingHistogram(mod_latency.PurePythonLatencyHistogram):
    """Counts the percentile walks of all its instances."""

    walks = 0

    def percentile(self, q):
        CountingHistogram.walks += 1
        return super().percentile(q)


def test_the_percentile_walk_is_cached():
    CountingHistogram.walks = 0
    host, clock = host_of(histogram=CountingHistogram, window=1000,
                          minSamples=1)
    for v in VALUES:
        host.record(v)
    want = reference(VALUES, 0.95)
    # a burst within 100 ms: one walk, new samples or not
    for n in range(50):
        assert host.delay() == want
        host.record(900)
        clock.tick(1.5)
    assert CountingHistogram.walks == 1
    clock.tick(30)                          # 105 ms after the walk
    fresh = host.delay()
    assert CountingHistogram.walks == 2
    assert fresh == reference(VALUES + [900] * 50, 0.95) and fresh > want
    assert host.delay() == fresh and CountingHistogram.walks == 2
    # a rotation drops the cache at once
    clock.tick(50)
    assert host.delay() == fresh and CountingHistogram.walks == 2
    clock.tick(900)                         # past the window
    host.record(5)
    assert host.delay() == fresh            # all of it still counts
    assert CountingHistogram.walks == 3
    # another policy's percentile is cached next to it
    p50 = policy_of(percentile=50)
    first = host.delay(None, p50)
    assert CountingHistogram.walks == 4
    assert host.delay(None, p50) == first and host.delay() == fresh
    assert CountingHistogram.walks == 4


def test_the_native_histogram_is_used_when_loaded():
    host, _ = host_of()
    assert type(host.current) is mod_latency.LatencyHistogram
    assert type(host.previous) is mod_latency.LatencyHistogram


def test_on_delay_reports_each_recomputation():
    seen = []
    clock = Clock()
    host = HedgeHost("svc", policy_of(minSamples=1), clock,
                     on_delay=lambda h, ms: seen.append((h, ms)))
    host.record(10)
    host.delay()
    host.delay()
    assert seen == [("svc", 10)]
    clock.tick(101)
    host.delay()
    assert seen == [("svc", 10), ("svc", 10)]


def test_budget_limit():
    host, _ = host_of(budget={"percent": 20, "minConcurrency": 0})
    assert host.limit() == 0 and not host.allows()
    host.active = 9
    assert host.limit() == 1 and host.allows()
    host.hedging = 1
    assert not host.allows()
    host.active = 10
    assert host.limit() == 2 and host.allows()
    host, _ = host_of(budget={"percent": 0, "minConcurrency": 2})
    host.hedging = 1
    assert host.allows()
    host.hedging = 2
    assert not host.allows()
    host, _ = host_of(budget=None)
    host.hedging = 1000
    assert host.limit() is None and host.allows()
