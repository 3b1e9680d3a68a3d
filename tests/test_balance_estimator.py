"""cueball_amd.balance: the peak-sensitive EWMA, the cost of a backend
and the pick among candidates.  Pure arithmetic, no pool; expected
values are computed here with math.exp."""

import math

import pytest

from cueball_amd.balance import (BackendLoad, PeakEwma, backend_costs,
                                 pick)

REL = 1e-12


def load(decay=1000.0, sample=None, at=0.0, outstanding=0):
    ld = BackendLoad(decay)
    if sample is not None:
        ld.ewma.observe(sample, at)
    ld.outstanding = outstanding
    return ld


def test_no_estimate_before_the_first_sample():
    e = PeakEwma(1000.0)
    assert e.get(0.0) is None
    assert e.get(123456.0) is None


def test_first_sample_sets_the_value():
    e = PeakEwma(1000.0)
    e.observe(40.0, 500.0)
    assert e.value == 40.0 and e.last == 500.0
    assert e.get(500.0) == pytest.approx(40.0, rel=REL)


def test_a_larger_sample_jumps():
    e = PeakEwma(1000.0)
    e.observe(10.0, 0.0)
    e.observe(100.0, 250.0)
    assert e.value == 100.0 and e.last == 250.0
    # however long ago the last one was
    e.observe(100.5, 250.0)
    assert e.value == 100.5


def test_a_smaller_sample_decays_by_the_formula():
    e = PeakEwma(1000.0)
    e.observe(100.0, 0.0)
    e.observe(10.0, 300.0)
    w = math.exp(-300.0 / 1000.0)
    want = 100.0 * w + 10.0 * (1.0 - w)
    assert e.value == pytest.approx(want, rel=REL)
    assert e.last == 300.0
    # and again, from the new value and the new time
    e.observe(10.0, 1000.0)
    w2 = math.exp(-700.0 / 1000.0)
    assert e.value == pytest.approx(want * w2 + 10.0 * (1.0 - w2), rel=REL)
    # no time passed: the old value stands
    before = e.value
    e.observe(1.0, 1000.0)
    assert e.value == pytest.approx(before, rel=REL)


def test_get_ages_without_changing_the_estimate():
    e = PeakEwma(2000.0)
    e.observe(100.0, 1000.0)
    for now in (1000.0, 1500.0, 3000.0, 21000.0):
        assert e.get(now) == pytest.approx(
            100.0 * math.exp(-(now - 1000.0) / 2000.0), rel=REL)
    assert e.value == 100.0 and e.last == 1000.0
    # after decay * ln(r) it undercuts a backend r times faster
    r = 10.0
    at = 1000.0 + 2000.0 * math.log(r)
    assert e.get(at - 1.0) > 10.0 > e.get(at + 1.0)


def test_cost_is_estimate_times_outstanding_plus_one():
    loads = {"a": load(sample=10.0, outstanding=0),
             "b": load(sample=10.0, outstanding=2),
             "c": load(sample=30.0, outstanding=1)}
    now = 200.0
    w = math.exp(-0.2)
    costs = backend_costs(loads, now)
    assert costs["a"] == pytest.approx(10.0 * w, rel=REL)
    assert costs["b"] == pytest.approx(10.0 * w * 3, rel=REL)
    assert costs["c"] == pytest.approx(30.0 * w * 2, rel=REL)


def test_a_backend_without_an_estimate_borrows_the_lowest_known():
    loads = {"slow": load(decay=500.0, sample=80.0, at=0.0),
             "fast": load(sample=20.0, at=400.0),
             "new": load(outstanding=0),
             "new-busy": load(outstanding=1)}
    now = 500.0
    lowest = 20.0 * math.exp(-0.1)
    assert 80.0 * math.exp(-1.0) > lowest
    costs = backend_costs(loads, now)
    assert costs["fast"] == pytest.approx(lowest, rel=REL)
    # ties with the best one: explored, never preferred
    assert costs["new"] == costs["fast"]
    assert costs["new-busy"] == pytest.approx(2 * lowest, rel=REL)
    # the lowest *aged* value: an old high estimate may be it
    later = 3000.0
    costs = backend_costs(loads, later)
    assert 80.0 * math.exp(-6.0) < 20.0 * math.exp(-2.6)
    assert costs["new"] == pytest.approx(80.0 * math.exp(-6.0), rel=REL)


def test_no_estimate_anywhere_counts_as_one():
    loads = {"a": load(), "b": load(outstanding=3)}
    assert backend_costs(loads, 0.0) == {"a": 1.0, "b": 4.0}
    assert backend_costs({}, 0.0) == {}


def test_least_loaded_ignores_estimates():
    loads = {"slow": load(sample=500.0, outstanding=0),
             "fast": load(sample=1.0, outstanding=1),
             "new": load(outstanding=2)}
    assert backend_costs(loads, 50.0, "leastLoaded") == {
        "slow": 1.0, "fast": 2.0, "new": 3.0}


def test_pick_takes_the_lowest_cost():
    assert pick([("a", 3.0), ("b", 1.0), ("c", 2.0)]) == "b"
    assert pick([("a", 3.0)]) == "a"
    assert pick([("a", 0.5), ("b", 1.0)]) == "a"


def test_a_tie_keeps_queue_order():
    assert pick([("a", 2.0), ("b", 2.0), ("c", 2.0)]) == "a"
    assert pick([("a", 3.0), ("b", 2.0), ("c", 2.0)]) == "b"
    # equal costs throughout: the head of the queue, which is FIFO
    queue = [("s%d" % i, 1.0) for i in range(8)]
    while queue:
        assert pick(queue) == queue[0][0]
        queue.pop(0)
