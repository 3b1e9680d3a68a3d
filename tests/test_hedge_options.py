"""The ``hedge`` option: validation, defaults, the per-call override."""

import gc
import math

import pytest

from cueball_amd import utils as mod_utils
from cueball_amd.agent import HttpAgent
from cueball_amd.hedge import HedgePolicy
from conftest import run_vt

RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50}}

DEFAULTS = {
    "delay": None, "percentile": 95, "window": 10000, "minSamples": 50,
    "minDelay": 1, "maxDelay": 1000, "methods": ["GET", "HEAD", "OPTIONS"],
    "budget": {"percent": 10, "minConcurrency": 1},
}


def check(hedge):
    return mod_utils.assert_hedge_policy({"hedge": hedge})


def test_off_without_the_option():
    assert mod_utils.assert_hedge_policy({}) is None
    assert check(None) is None


def test_defaults_are_filled_in():
    assert check({}) == DEFAULTS
    policy = HedgePolicy(check({}))
    assert policy.delay is None and policy.percentile == 95
    assert policy.window == 10000 and policy.min_samples == 50
    assert (policy.min_delay, policy.max_delay) == (1, 1000)
    assert policy.methods == frozenset(("GET", "HEAD", "OPTIONS"))


def test_given_values_are_kept():
    given = {"delay": 12.5, "percentile": 99.9, "window": 500,
             "minSamples": 1, "minDelay": 2, "maxDelay": 2,
             "methods": ["put"],
             "budget": {"percent": 0, "minConcurrency": 0}}
    want = dict(given, methods=["PUT"])
    assert check(given) == want
    # maxDelay follows a minDelay beyond its default
    assert check({"minDelay": 3000})["maxDelay"] == 3000


def test_methods_are_upper_cased_and_deduplicated():
    out = check({"methods": ("get", "GET", "Head", "get")})
    assert out["methods"] == ["GET", "HEAD"]
    assert check({"methods": []})["methods"] == []


def test_budget_none_is_accepted():
    assert check({"budget": None})["budget"] is None
    assert check({"budget": {}})["budget"] == DEFAULTS["budget"]
    assert check({"budget": {"percent": 50}})["budget"] == \
        {"percent": 50, "minConcurrency": 1}


@pytest.mark.parametrize("hedge", [
    [], "x", 5, True,
    {"delay": "5"}, {"delay": True},
    {"percentile": "95"}, {"percentile": [95]}, {"percentile": True},
    {"window": "1"}, {"window": False},
    {"minSamples": 5.0}, {"minSamples": True}, {"minSamples": "5"},
    {"minDelay": "1"}, {"maxDelay": "1"}, {"maxDelay": True},
    {"methods": "GET"}, {"methods": {"GET": 1}}, {"methods": 5},
    {"methods": [5]}, {"methods": [None]},
    {"budget": []}, {"budget": 5}, {"budget": {"percent": "1"}},
    {"budget": {"percent": True}}, {"budget": {"minConcurrency": 1.0}},
    {"budget": {"minConcurrency": True}},
])
def test_type_errors(hedge):
    with pytest.raises(TypeError):
        check(hedge)


@pytest.mark.parametrize("hedge", [
    {"delay": 0}, {"delay": -1}, {"delay": math.inf}, {"delay": math.nan},
    {"percentile": 0}, {"percentile": 100}, {"percentile": -5},
    {"percentile": math.nan},
    {"window": 0}, {"window": -1}, {"window": math.inf},
    {"minSamples": 0}, {"minSamples": -1},
    {"minDelay": 0}, {"minDelay": math.inf},
    {"maxDelay": 0.5}, {"maxDelay": math.inf}, {"maxDelay": math.nan},
    {"minDelay": 10, "maxDelay": 5},
    {"methods": [""]},
    {"budget": {"percent": -1}}, {"budget": {"percent": 101}},
    {"budget": {"minConcurrency": -1}},
])
def test_range_errors(hedge):
    with pytest.raises(ValueError):
        check(hedge)


@pytest.mark.parametrize("hedge", [
    {"delays": 5}, {"maxRetries": 1}, {5: 1},
    {"budget": {"percent": 10, "ttl": 1}},
])
def test_unknown_keys_are_rejected(hedge):
    with pytest.raises(ValueError, match="unknown keys"):
        check(hedge)


def test_override():
    base = check({"delay": 20})
    out = mod_utils.override_hedge_policy(base, {"delay": 5,
                                                 "methods": ["post"]})
    assert out == dict(base, delay=5, methods=["POST"])
    assert base["delay"] == 20                  # a copy
    # back to adaptive for one call
    assert mod_utils.override_hedge_policy(base, {"delay": None})["delay"] \
        is None
    assert mod_utils.override_hedge_policy(base, {}) == base
    for shared in ("budget", "window", "minSamples"):
        with pytest.raises(ValueError, match=shared):
            mod_utils.override_hedge_policy(base, {shared: None})
    # the override is validated like the option
    with pytest.raises(ValueError):
        mod_utils.override_hedge_policy(base, {"delay": -1})
    with pytest.raises(ValueError, match="unknown keys"):
        mod_utils.override_hedge_policy(base, {"nope": 1})
    with pytest.raises(TypeError):
        mod_utils.override_hedge_policy(base, {"percentile": "high"})
    with pytest.raises(TypeError):
        mod_utils.override_hedge_policy(base, True)
    with pytest.raises(ValueError):
        mod_utils.override_hedge_policy(None, {"delay": 5})


def instance_vars(agent):
    """vars(agent); the native runtime's objects keep their instance
    dict without a ``__dict__`` attribute, so there it is found among
    the object's referents."""
    try:
        return vars(agent)
    except TypeError:
        for ref in gc.get_referents(agent):
            if isinstance(ref, dict) and "cba_stopped" in ref:
                return ref
        raise


def make_agent(loop, **opts):
    base = {"recovery": RECOVERY, "spares": 1, "maximum": 2, "loop": loop}
    base.update(opts)
    return HttpAgent(base)


def test_the_agent_validates_at_construction():
    async def body(loop):
        with pytest.raises(TypeError):
            make_agent(loop, hedge=[])
        with pytest.raises(ValueError):
            make_agent(loop, hedge={"percentile": 100})
        agent = make_agent(loop, hedge={})
        assert agent.cba_hedge == DEFAULTS
        assert agent.get_hedge_stats() == {}
    run_vt(body)


def test_an_agent_without_the_option_is_unchanged():
    async def body(loop):
        plain = make_agent(loop)
        assert plain.get_hedge_stats() == {}
        assert not [k for k in instance_vars(plain) if "hedge" in k]
        hedged = make_agent(loop, hedge={})
        new = set(instance_vars(hedged)) - set(instance_vars(plain))
        assert new == {"cba_hedge", "cba_hedge_policy", "cba_hedge_hosts",
                       "_hedge_metrics"}
        names = plain.collector.collect()
        assert "cueball_agent_hedge" not in names
        assert "cueball_agent_hedges_total" in hedged.collector.collect()
    run_vt(body)


def test_hedge_per_call_needs_the_option():
    async def body(loop):
        plain = make_agent(loop)
        with pytest.raises(ValueError, match="options.hedge"):
            plain.request("svc.example", hedge={"delay": 5})
        with pytest.raises(ValueError, match="options.hedge"):
            plain.request("svc.example", hedge={})
        with pytest.raises(TypeError):
            plain.request("svc.example", hedge=True)
        with pytest.raises(ValueError, match="options.hedge"):
            await plain.request_async("svc.example", hedge={"delay": 5})
        # nothing was started for any of them
        assert plain.pools == {}

        hedged = make_agent(loop, hedge={})
        for bad in ({"budget": None}, {"window": 5}, {"minSamples": 5},
                    {"delay": 0}):
            with pytest.raises(ValueError):
                hedged.request("svc.example", hedge=bad)
        with pytest.raises(TypeError):
            hedged.request("svc.example", hedge=True)
        assert hedged.pools == {} and hedged.get_hedge_stats() == {}
    run_vt(body)


def test_a_foreign_collector_gets_no_hedge_metrics():
    class Foreign:
        """Counters only, as the agent's error metrics need them."""

        def __init__(self):
            from cueball_amd.metrics import Collector
            self.inner = Collector()

        def counter(self, **kw):
            return self.inner.counter(**kw)

    async def body(loop):
        agent = make_agent(loop, hedge={}, collector=Foreign())
        assert agent._hedge_metrics is None
        agent._hedge_counted("h", "hedge-sent")        # and no harm done
        agent._hedge_delay_changed("h", 5.0)
    run_vt(body)
