"""cueball_amd.limit alone: every figure here is computed by hand from
the documented formulas, no pool."""

import math

import pytest

from limit_kit import closed_loop, limiter

AIMD = {"algorithm": "aimd", "latencyThreshold": 75, "window": 100,
        "minSamples": 4}


def window(lim, t0, hold, n, peak, gap=40.0):
    """One window: `peak` leases start at `t0`, and `n` samples of
    `hold` ms come back `gap` ms apart from ``t0 + gap`` on, each lease
    replaced as it ends.  Returns the time of the last sample."""
    tokens = [lim.on_start(t0) for _ in range(peak)]
    now = t0
    for i in range(n):
        now = t0 + gap * (i + 1)
        lim.on_sample(tokens.pop(0), hold, now)
        if i < n - 1:
            tokens.append(lim.on_start(now))
    for tok in tokens:
        lim.on_discard(tok)
    return now


# -- aimd ---------------------------------------------------------------

def test_aimd_a_window_over_threshold_multiplies_by_the_ratio():
    lim = limiter(dict(AIMD, initialLimit=10))
    assert lim.allowed() == 10 and lim.limit == 10.0
    tok = [lim.on_start(0.0) for _ in range(4)]
    assert lim.on_sample(tok[0], 80.0, 30.0) is False
    assert lim.on_sample(tok[1], 80.0, 60.0) is False
    assert lim.on_sample(tok[2], 80.0, 90.0) is False
    # the fourth sample, 100 ms after the window opened, closes it
    assert lim.on_sample(tok[3], 80.0, 100.0) is True
    assert lim.limit == 10 * 0.9 and lim.allowed() == 9
    assert (lim.windows, lim.lowered, lim.raised) == (1, 1, 0)
    assert lim.last_mean == 80.0


def test_aimd_backoff_ratio_is_the_option():
    lim = limiter(dict(AIMD, initialLimit=10, backoffRatio=0.5))
    window(lim, 0.0, 76.0, 4, 1)
    assert lim.limit == 5.0


def test_aimd_under_threshold_at_peak_adds_one():
    lim = limiter(dict(AIMD, initialLimit=4.5))
    assert lim.allowed() == 4
    # the mean equals the threshold: not over it; peak 4 == floor(4.5)
    window(lim, 0.0, 75.0, 4, 4)
    assert lim.limit == 5.5 and lim.raised == 1


def test_aimd_under_threshold_below_peak_leaves_the_limit_alone():
    lim = limiter(dict(AIMD, initialLimit=4.5))
    window(lim, 0.0, 10.0, 4, 3)
    assert lim.limit == 4.5
    assert (lim.windows, lim.raised, lim.lowered) == (1, 0, 0)


def test_aimd_clamps_at_both_ends():
    lim = limiter(dict(AIMD, initialLimit=16))
    window(lim, 0.0, 10.0, 4, 16)
    assert lim.limit == 16.0 and lim.raised == 0
    lim = limiter(dict(AIMD, minLimit=2, initialLimit=2.1))
    window(lim, 0.0, 100.0, 4, 2)
    assert lim.limit == 2.0 and lim.lowered == 1
    window(lim, 1000.0, 100.0, 4, 2)
    assert lim.limit == 2.0 and lim.lowered == 1
    lim = limiter(dict(AIMD, maxLimit=8, initialLimit=7.5))
    window(lim, 0.0, 10.0, 4, 7)
    assert lim.limit == 8.0


def test_aimd_a_window_with_its_time_but_not_its_samples_stays_open():
    lim = limiter(dict(AIMD, initialLimit=10))
    tok = [lim.on_start(0.0) for _ in range(4)]
    lim.on_sample(tok[0], 80.0, 500.0)
    lim.on_sample(tok[1], 80.0, 600.0)
    lim.on_sample(tok[2], 80.0, 700.0)
    assert lim.windows == 0 and lim.limit == 10.0
    lim.on_sample(tok[3], 80.0, 701.0)
    assert lim.windows == 1 and lim.limit == 9.0
    # and one with its samples but not its time
    tok = [lim.on_start(701.0) for _ in range(5)]
    for i, t in enumerate(tok[:4]):
        lim.on_sample(t, 80.0, 710.0 + i)
    assert lim.windows == 1
    lim.on_sample(tok[4], 80.0, 801.0)
    assert lim.windows == 2


def test_a_failed_lease_leaves_no_sample():
    lim = limiter(dict(AIMD, initialLimit=10))
    tok = [lim.on_start(0.0) for _ in range(6)]
    assert lim.in_flight == 6
    lim.on_discard(tok[0])
    lim.on_discard(tok[1])
    assert lim.in_flight == 4 and lim.discarded == 2 and lim.samples == 0
    for i, t in enumerate(tok[2:]):
        lim.on_sample(t, 10.0, 200.0 + i)
    assert lim.samples == 4 and lim.windows == 1 and lim.in_flight == 0
    assert lim.last_mean == 10.0


def test_a_lease_begun_under_another_allowed_leaves_no_sample():
    lim = limiter(dict(AIMD, initialLimit=10))
    stale = [lim.on_start(0.0) for _ in range(3)]
    window(lim, 0.0, 80.0, 4, 4)
    # (the helper discards the three leases it leaves open)
    assert lim.allowed() == 9 and lim.discarded == 3
    # 10 -> 9: what began under 10 ran at the load of 10
    for i, t in enumerate(stale):
        lim.on_sample(t, 500.0, 300.0 + i)
    assert lim.discarded == 6 and lim.samples == 4 and lim.windows == 1
    window(lim, 400.0, 10.0, 4, 9)
    assert lim.last_mean == 10.0 and lim.limit == 10.0


# -- gradient -----------------------------------------------------------

GRAD = {"window": 100, "minSamples": 4, "probeSpread": 0,
        "probeInterval": 5000}


def probed(cl, baseline=50.0, t0=0.0):
    """A limiter whose first probe has measured `baseline`; returns it
    and the time the probe ended."""
    lim = limiter(cl)
    assert lim.probing
    now = window(lim, t0, baseline, lim.cfg["probeSamples"], 1, gap=10.0)
    assert not lim.probing and lim.baseline == baseline
    return lim, now


def test_gradient_one_update_by_the_five_steps():
    lim, t = probed(dict(GRAD, initialLimit=10))
    window(lim, t, 120.0, 4, 10)
    limit = 10.0
    g = min(max(1.5 * 50.0 / 120.0, 0.5), 1.0)
    new = limit * g + math.sqrt(limit)
    want = limit * (1 - 0.2) + new * 0.2
    assert g == 0.625 and new < limit
    assert lim.limit == want
    assert lim.allowed() == math.floor(want) == 9
    assert lim.last_mean == 120.0 and lim.lowered == 1


def test_gradient_tolerance_and_smoothing_are_the_options():
    lim, t = probed(dict(GRAD, initialLimit=10, tolerance=1.0,
                         smoothing=1.0))
    window(lim, t, 80.0, 4, 10)
    assert lim.limit == 10.0 * (1.0 * 50.0 / 80.0) + math.sqrt(10.0)


@pytest.mark.parametrize("mean,g", [(1000.0, 0.5), (20.0, 1.0)])
def test_gradient_g_is_clamped(mean, g):
    lim, t = probed(dict(GRAD, initialLimit=9))
    window(lim, t, mean, 4, 9)
    new = 9.0 * g + 3.0
    assert lim.limit == 9.0 * (1 - 0.2) + new * 0.2


def test_gradient_clamps_the_limit():
    lim, t = probed(dict(GRAD, initialLimit=16))
    window(lim, t, 20.0, 4, 16)
    assert lim.limit == 16.0
    lim, t = probed(dict(GRAD, minLimit=4, maxLimit=8, initialLimit=4,
                         smoothing=1.0, probeLimit=4))
    window(lim, t, 1000.0, 4, 4)
    assert 4.0 * 0.5 + 2.0 == 4.0 and lim.limit == 4.0
    window(lim, t + 1000, 20.0, 4, 4)
    assert lim.limit == 6.0
    window(lim, t + 2000, 20.0, 4, 6)
    assert lim.limit == 8.0             # 6 + sqrt(6), clamped


def test_gradient_app_limited_keeps_the_limit():
    lim, t = probed(dict(GRAD, initialLimit=10))
    # new > limit, and the peak of 4 is below 10 / 2
    window(lim, t, 50.0, 4, 4)
    assert lim.limit == 10.0 and lim.windows == 1
    # at a peak of 5 it is not
    window(lim, t + 1000, 50.0, 4, 5)
    assert lim.limit == 10.0 * 0.8 + (10.0 + math.sqrt(10.0)) * 0.2
    # and a decrease is never held back
    lim, t = probed(dict(GRAD, initialLimit=10))
    window(lim, t, 150.0, 4, 1)
    assert lim.limit == 10.0 * 0.8 + (10.0 * 0.5 + math.sqrt(10.0)) * 0.2


def test_gradient_starts_in_a_probe_that_waits_for_a_sample():
    lim = limiter(dict(GRAD, initialLimit=10))
    assert lim.probing and lim.probes == 1
    assert lim.allowed() == 3 and lim.limit == 10.0
    tok = [lim.on_start(1000.0) for _ in range(3)]
    lim.on_discard(tok[0])
    lim.on_discard(tok[1])
    assert lim.probing and lim.baseline is None
    # long past `window`, the probe is still waiting for its sample
    assert lim.on_sample(tok[2], 42.0, 9000.0) is False
    assert not lim.probing and lim.baseline == 42.0
    assert lim.allowed() == 10 and lim.limit == 10.0


def test_probe_limit_is_clipped_to_the_limits():
    assert limiter(dict(GRAD, probeLimit=2)).allowed() == 2
    assert limiter(dict(GRAD, minLimit=5)).allowed() == 5
    assert limiter(dict(GRAD, maxLimit=2)).allowed() == 2


def test_a_probe_begins_every_probe_interval_and_ends_on_its_samples():
    lim, t = probed(dict(GRAD, initialLimit=10))
    assert t == 40.0
    tok = lim.on_start(t)
    lim.on_sample(tok, 50.0, 4999.0)
    assert not lim.probing
    before = [lim.on_start(4999.0) for _ in range(2)]
    lim.on_sample(before[0], 50.0, 5000.0)      # 5000 ms after the first
    assert lim.probing and lim.probes == 2 and lim.allowed() == 3
    limit = lim.limit
    # a lease that began before the probe is not one of its samples
    lim.on_sample(before[1], 900.0, 5001.0)
    assert lim.probing and lim.probe_count == 0
    inside = [lim.on_start(5001.0) for _ in range(3)]
    for i, tok in enumerate(inside):
        lim.on_sample(tok, 60.0 + i, 5010.0 + i)
    assert lim.probing
    tok = lim.on_start(5013.0)
    lim.on_sample(tok, 63.0, 5020.0)            # the fourth: probeSamples
    assert not lim.probing
    assert lim.baseline == (60.0 + 61.0 + 62.0 + 63.0) / 4
    assert lim.limit == limit and lim.allowed() == math.floor(limit)
    # the next one is due 5000 ms after this one began
    tok = lim.on_start(5020.0)
    lim.on_sample(tok, 50.0, 9999.0)
    assert not lim.probing
    tok = lim.on_start(9999.0)
    lim.on_sample(tok, 50.0, 10000.0)
    assert lim.probing and lim.probes == 3


def test_a_probe_ends_when_it_is_a_window_old():
    lim, t = probed(dict(GRAD, initialLimit=10, probeSamples=50))
    tok = lim.on_start(t)
    lim.on_sample(tok, 50.0, 6000.0)
    assert lim.probing
    a, b, c = (lim.on_start(6000.0) for _ in range(3))
    lim.on_sample(a, 70.0, 6050.0)
    lim.on_sample(b, 80.0, 6099.0)
    assert lim.probing
    lim.on_sample(c, 90.0, 6100.0)              # `window` ms old
    assert not lim.probing and lim.baseline == 80.0


def test_a_probe_without_a_sample_keeps_the_baseline():
    lim, t = probed(dict(GRAD, initialLimit=10))
    stale = [lim.on_start(t) for _ in range(2)]
    lim.on_sample(stale[0], 50.0, 5000.0)
    assert lim.probing
    # the only sample to arrive began before the probe
    lim.on_sample(stale[1], 700.0, 5200.0)
    assert not lim.probing and lim.baseline == 50.0


def test_probe_spread_is_drawn_from_the_injected_random():
    class Fixed:
        draws = 0

        def random(self):
            self.draws += 1
            return 0.5

    rnd = Fixed()
    lim, t = probed(dict(GRAD, initialLimit=10, probeSpread=0.2,
                         random=rnd))
    assert rnd.draws == 1
    # 5000 * (1 - 0.2 * 0.5) = 4500 ms after the first probe began
    tok = lim.on_start(t)
    lim.on_sample(tok, 50.0, 4499.0)
    assert not lim.probing
    tok = lim.on_start(4499.0)
    lim.on_sample(tok, 50.0, 4500.0)
    assert lim.probing and rnd.draws == 2


# -- closed loop ----------------------------------------------------------

@pytest.mark.parametrize("initial", [16, 1])
def test_aimd_settles_into_a_sawtooth_of_6_and_7(initial):
    """Threshold 75 against base 50 at capacity 4: 6 leases take 75 ms,
    which is not over it, and 7 take 87.5, which is."""
    lim = limiter({"algorithm": "aimd", "latencyThreshold": 75,
                   "initialLimit": initial})
    floors = closed_loop(lim, 60)
    print(initial, floors)
    assert set(floors[15:]) == {6, 7}


def test_gradient_holds_its_fixed_point_of_9():
    """``L = tolerance * C + sqrt(L)``: 6 + 3 = 9.  Window 400 is past a
    dozen probes and long past where a baseline that drifts would have
    let go."""
    lim = limiter({"probeSpread": 0})
    floors = closed_loop(lim, 400)
    print(floors[:45], floors[-5:], lim.probes, lim.baseline)
    assert all(8 <= f <= 10 for f in floors[39:])
    assert 8 <= floors[399] <= 10
    assert lim.probes >= 10 and lim.baseline == 50.0
