"""plan_rebalance with SRV ranks: tiers and weighted spread.

The contract under test: with every key carrying the same (priority,
weight) the ranked planner reproduces the unranked plan exactly; within
one tier connections follow the weights (exactly at multiples of the
tier's total weight, monotonically in between); only the lowest
reachable priority carries load while dead lower-numbered tiers keep one
monitor each; and the number of key-source steps never depends on the
size of the weights.
"""

import math
import random

import pytest

from cueball_amd import utils

WEIGHTS = (0, 1, 10, 65535)

# (connections, dead, target, maximum, singleton): the shapes of the
# 21-case spec table in tests/test_utils.py
TABLE = [
    ({"b1": []}, {}, 4, 10, False),
    ({"b1": [], "b2": []}, {}, 5, 10, False),
    ({"b1": ["c1"], "b2": ["c2"]}, {}, 4, 10, False),
    ({"b1": ["c1", "c3"], "b2": ["c2", "c4"]}, {}, 4, 10, False),
    ({"b1": ["c1", "c2", "c3"], "b2": ["c4"]}, {}, 4, 10, False),
    ({"b1": ["c1", "c2", "c3"], "b2": ["c4"]}, {}, 6, 10, False),
    ({"b1": ["c1", "c2", "c3"], "b2": ["c4", "c5", "c6"]}, {}, 4, 10, False),
    ({"b1": ["c1", "c2", "c3", "c4"], "b2": [], "b3": [], "b4": [],
      "b5": [], "b6": [], "b7": []}, {}, 5, 10, False),
    ({"b3": [], "b1": [], "b2": [], "b4": [],
      "b5": ["c1", "c2", "c3", "c4"], "b6": [], "b7": []}, {}, 6, 10, False),
    ({"b3": ["c1"], "b1": ["c2"], "b2": ["c3"], "b4": ["c4"],
      "b5": ["c5"], "b6": ["c6"], "b7": []}, {}, 3, 10, False),
    ({"b3": ["c1"], "b1": [], "b2": []}, {}, 4, 10, False),
    ({"b2": [], "b1": ["c1"], "b3": ["c2"]}, {}, 2, 10, False),
    ({"b1": [], "b2": [], "b3": []}, {"b1": True}, 2, 10, False),
    ({"b1": ["c1", "c3"], "b2": ["c2"], "b3": []}, {"b1": True}, 3, 10,
     False),
    ({"b1": ["c1"], "b2": ["c2"]}, {"b1": True}, 1, 2, False),
    ({"b1": [], "b2": ["c2"], "b3": [], "b4": []},
     {"b1": True, "b3": True}, 2, 10, False),
    ({"b1": [], "b2": ["c2"], "b3": [], "b4": []},
     {"b1": True, "b3": True}, 2, 3, False),
    ({"b1": ["c1"]}, {"b1": True}, 2, 10, False),
    ({"b1": ["c1"], "b2": []}, {"b1": True}, 3, 10, False),
    ({"k1": ["c1"], "k2": ["c2"], "k3": [], "k4": []},
     {"k2": True, "k1": True, "k4": True, "k3": True}, 3, 4, False),
    ({"b1": [], "b2": [], "b3": []}, {}, 5, 10, True),
    ({"b1": [], "b2": []}, {"b1": True}, 2, 10, True),
]


def counts(conns, plan):
    """Per-key connection counts once ``plan`` has been carried out."""
    out = {k: len(v) for k, v in conns.items()}
    owner = {c: k for k, v in conns.items() for c in v}
    for c in plan["remove"]:
        out[owner[c]] -= 1
    for k in plan["add"]:
        out[k] += 1
    return out


def spread(weights, target, maximum=None, dead=(), singleton=False,
           prios=None):
    keys = ["b%d" % i for i in range(len(weights))]
    prios = prios or [0] * len(weights)
    ranks = {k: (p, w) for k, p, w in zip(keys, prios, weights)}
    conns = {k: [] for k in keys}
    plan = utils.plan_rebalance(
        conns, {keys[i]: True for i in dead}, target,
        target if maximum is None else maximum, singleton, ranks=ranks)
    assert plan["remove"] == []
    c = counts(conns, plan)
    return [c[k] for k in keys]


# -- equivalence with the unranked planner ---------------------------------

@pytest.mark.parametrize("case", range(len(TABLE)))
def test_uniform_ranks_reproduce_spec_table(case):
    conns, dead, target, maximum, singleton = TABLE[case]
    base = utils.plan_rebalance(conns, dead, target, maximum, singleton)
    for prio in (0, 7):
        for w in WEIGHTS:
            ranks = {k: (prio, w) for k in conns}
            assert utils.plan_rebalance(conns, dead, target, maximum,
                                        singleton, ranks=ranks) == base


def test_uniform_ranks_reproduce_random_plans():
    rng = random.Random(2782)
    for n in range(4000):
        nkeys = rng.randint(1, 6)
        keys = ["b%d" % i for i in range(nkeys)]
        rng.shuffle(keys)
        maximum = rng.randint(0, 10)
        target = rng.randint(0, maximum)
        singleton = bool(n & 1)
        conns = {}
        serial = 0
        for k in keys:
            have = rng.randint(0, 1 if singleton else 4)
            conns[k] = ["c%d" % (serial + i) for i in range(have)]
            serial += have
        dead = {k: True for k in keys if rng.random() < 0.35}
        rank = (rng.choice((0, 3, 10)), rng.choice(WEIGHTS))
        ranks = {k: rank for k in keys}
        base = utils.plan_rebalance(conns, dead, target, maximum, singleton)
        got = utils.plan_rebalance(conns, dead, target, maximum, singleton,
                                   ranks=ranks)
        assert got == base, (conns, dead, target, maximum, singleton, rank)


def test_no_ranks_never_touches_rank_data():
    class Untouchable(dict):
        def _no(self, *a, **kw):
            raise AssertionError("rank data was read")
        __getitem__ = get = __contains__ = __iter__ = _no
        keys = items = values = __len__ = _no

    conns, dead, target, maximum, singleton = TABLE[13]
    base = utils.plan_rebalance(conns, dead, target, maximum, singleton)
    assert utils.plan_rebalance(conns, dead, target, maximum, singleton,
                                ranks=None) == base
    # and the guard itself does guard
    with pytest.raises(AssertionError):
        utils.plan_rebalance(conns, dead, target, maximum, singleton,
                             ranks=Untouchable())


# -- weighted spread within one tier ----------------------------------------

def eff(weights):
    raw = [max(w, 1) for w in weights]
    g = math.gcd(*raw)
    return [w // g for w in raw]


def test_exact_proportion_examples():
    assert spread([3, 1], 8) == [6, 2]
    assert spread([0, 10], 11) == [1, 10]
    assert spread([30, 10], 4) == [3, 1]
    assert spread([10, 30], 4) == [1, 3]


@pytest.mark.parametrize("weights", [
    [3, 1], [1, 3], [0, 10], [2, 3, 5], [5, 1, 1], [4, 6], [1, 1, 1],
    [0, 0, 7], [10, 20, 30, 40],
])
def test_exact_at_multiples_monotone_between(weights):
    e = eff(weights)
    tot = sum(e)
    prev = [0] * len(weights)
    for mult in range(1, 4):
        at = spread(weights, mult * tot)
        assert at == [mult * x for x in e]
        for target in range((mult - 1) * tot + 1, mult * tot):
            got = spread(weights, target)
            assert sum(got) == target
            for lo, g, hi in zip(prev, got, at):
                assert lo <= g <= hi, (weights, target, got)
        prev = at


def test_weighted_spread_is_interleaved_not_bursty():
    # smooth round-robin: the light backend is not starved until the end
    assert spread([3, 1], 3) == [2, 1]
    # 5,1,1 by hand: a a b a c a a
    assert spread([5, 1, 1], 3) == [2, 1, 0]
    assert spread([5, 1, 1], 5) == [3, 1, 1]


# -- tiers ---------------------------------------------------------------------

TIER_W = [3, 1, 1, 1]
TIER_P = [0, 0, 10, 10]


def tier_plan(conns, dead, target, maximum, singleton=False):
    keys = ["p1", "p2", "s1", "s2"]
    ranks = {k: (p, w) for k, p, w in zip(keys, TIER_P, TIER_W)}
    full = {k: list(conns.get(k, ())) for k in keys}
    plan = utils.plan_rebalance(full, dead, target, maximum, singleton,
                                ranks=ranks)
    c = counts(full, plan)
    return plan, [c[k] for k in keys]


def test_tiers_all_alive_nothing_on_standbys():
    plan, c = tier_plan({}, {}, 6, 8)
    assert c == [5, 1, 0, 0]
    # connections already on the standbys are removed
    plan, c = tier_plan({"p1": ["a"], "s1": ["x", "y"], "s2": ["z"]}, {},
                        6, 8)
    assert c == [5, 1, 0, 0]
    assert plan["remove"] == ["z", "x", "y"]


def test_tiers_primaries_dead_monitors_plus_standby_spread():
    plan, c = tier_plan({}, {"p1": True, "p2": True}, 6, 8)
    assert c == [1, 1, 3, 3]


def test_tiers_heavy_primary_dead_share_flows_to_sibling():
    plan, c = tier_plan({}, {"p1": True}, 6, 8)
    assert c == [1, 6, 0, 0]


def test_tiers_cap_keeps_a_slot_for_the_active_tier():
    plan, c = tier_plan({}, {"p1": True, "p2": True}, 2, 2)
    assert sum(c[:2]) == 1          # one monitor only
    assert sum(c[2:]) == 1          # never zero on the active tier
    assert c == [1, 0, 1, 0]        # handed out in preference order


def test_tiers_everything_dead_stays_on_lowest_priority():
    dead = {k: True for k in ("p1", "p2", "s1", "s2")}
    plan, c = tier_plan({}, dead, 2, 8)
    assert c[2:] == [0, 0]
    assert c[:2] == [1, 1]


def test_monitors_in_priority_then_preference_order():
    keys = ["c", "a", "b", "z"]
    ranks = {"a": (0, 1), "b": (5, 1), "c": (5, 1), "z": (9, 1)}
    conns = {k: [] for k in keys}
    dead = {"a": True, "b": True, "c": True}
    plan = utils.plan_rebalance(conns, dead, 2, 3, ranks=ranks)
    assert plan["add"] == ["c", "a", "z"]   # monitors: a, then c (not b)


def test_active_priority_helper():
    ranks = {"a": (0, 1), "b": (0, 1), "c": (10, 1)}
    keys = list(ranks)
    assert utils.active_priority(keys, {}, ranks) == 0
    assert utils.active_priority(keys, {"a": True}, ranks) == 0
    assert utils.active_priority(keys, {"a": True, "b": True}, ranks) == 10
    assert utils.active_priority(
        keys, {"a": True, "b": True, "c": True}, ranks) == 0
    assert utils.active_priority([], {}, ranks) is None
    # unknown keys rank as (0, 0)
    assert utils.active_priority(["x"], {}, {}) == 0


# -- singleton -----------------------------------------------------------------

def test_singleton_prefers_heavier_backends():
    assert spread([1, 5, 2], 2, maximum=4, singleton=True) == [0, 1, 1]
    # equal weights keep the preference order
    assert spread([2, 2, 2], 2, maximum=4, singleton=True) == [1, 1, 0]


def test_singleton_never_picks_standby_while_primary_alive():
    assert spread([1, 1, 1], 3, maximum=5, singleton=True,
                  prios=[0, 0, 10]) == [1, 1, 0]
    assert spread([1, 1, 1], 3, maximum=5, singleton=True,
                  prios=[0, 0, 10], dead=[0]) == [1, 1, 0]
    assert spread([1, 1, 1], 3, maximum=5, singleton=True,
                  prios=[0, 0, 10], dead=[0, 1]) == [1, 1, 1]


# -- bounded work ----------------------------------------------------------------

def steps(monkeypatch, weights, **kw):
    calls = [0]
    real = utils._WeightedCycle.next

    def counting(self):
        calls[0] += 1
        return real(self)

    with monkeypatch.context() as m:
        m.setattr(utils._WeightedCycle, "next", counting)
        result = spread(weights, **kw)
    return calls[0], result


@pytest.mark.parametrize("kw", [
    dict(target=4, maximum=8, dead=[0]),
    dict(target=4, maximum=8),
    dict(target=2, maximum=4, singleton=True),
    dict(target=2, maximum=4, singleton=True, dead=[0]),
], ids=["heavy-dead", "alive", "singleton", "singleton-heavy-dead"])
def test_steps_do_not_depend_on_weight_size(monkeypatch, kw):
    big, big_counts = steps(monkeypatch, [65535, 1], **kw)
    small, small_counts = steps(monkeypatch, [2, 1], **kw)
    assert big == small
    assert 0 < big <= 4 * kw["maximum"]
    assert sum(big_counts) <= kw["maximum"]


def test_argument_checks_hold_with_ranks():
    with pytest.raises(ValueError):
        utils.plan_rebalance({"a": []}, {}, -1, 2, ranks={"a": (0, 1)})
    with pytest.raises(ValueError):
        utils.plan_rebalance({"a": []}, {}, 3, 2, ranks={"a": (0, 1)})
    assert utils.plan_rebalance({}, {}, 2, 2, ranks={}) == \
        {"add": [], "remove": []}
