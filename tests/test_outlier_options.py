"""``outlierDetection``: validation and defaults on pools and agents,
forwarding from an agent to its pools, and a pool without the option
staying exactly what it was."""

import math

import pytest

from cueball_amd import utils as mod_utils
from cueball_amd.agent import HttpAgent, HttpsAgent
from cueball_amd.errors import CueballError
from cueball_amd.testing import advance, settle
from conftest import run_vt
from outlier_kit import Kit, instance_vars

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 0}}

#: the instance variables of a pool created without any opt-in feature,
#: as they were before outlier detection existed
PLAIN_POOL_VARS = {
    "_gauge", "_gauge_labels", "_lat_metrics", "p_backends", "p_busy_hwm",
    "p_check_timeout", "p_checker", "p_claim_log", "p_codel",
    "p_collector", "p_connections", "p_constructor", "p_counters",
    "p_dead", "p_demand_hwm", "p_domain", "p_idleq", "p_in_rebalance",
    "p_initq", "p_keys", "p_last_error", "p_last_rebal_clamped",
    "p_last_rebalance", "p_lastrate", "p_lat", "p_log", "p_lp_timer",
    "p_lpf", "p_max", "p_maxrate", "p_noop_census", "p_rate_delay_timer",
    "p_rebal_scheduled", "p_rebal_timer", "p_recovery", "p_resolver",
    "p_resolver_custom", "p_shuffle_timer", "p_spares",
    "p_started_resolver", "p_total_conns", "p_uuid", "p_waiters"}

BAD_TYPE = [
    5, "on", [("consecutiveFailures", 2)], True,
    {"consecutiveFailures": 2.0}, {"consecutiveFailures": "2"},
    {"consecutiveFailures": True},
    {"baseEjectionTime": "1000"}, {"baseEjectionTime": True},
    {"maxEjectionTime": [1]}, {"maxEjectionTime": False},
    {"maxEjectionPercent": "50"}, {"maxEjectionPercent": True},
    {"countClose": 1}, {"countClose": "yes"},
    {"countSocketClose": 0}, {"countSocketClose": "no"},
]
BAD_VALUE = [
    {"consecutiveFailures": 0}, {"consecutiveFailures": -1},
    {"baseEjectionTime": 0}, {"baseEjectionTime": -1},
    {"baseEjectionTime": math.inf}, {"baseEjectionTime": math.nan},
    {"maxEjectionTime": math.inf}, {"maxEjectionTime": math.nan},
    {"baseEjectionTime": 1000, "maxEjectionTime": 999},
    {"maxEjectionTime": 29_999},          # below the default base
    {"maxEjectionPercent": 0}, {"maxEjectionPercent": -1},
    {"maxEjectionPercent": 100.5}, {"maxEjectionPercent": math.nan},
    {"consecutiveFailure": 2}, {"enabled": True},
]


async def stop_pools(loop, *pools):
    """No test may leave a pool behind: it would stay registered with
    the process-wide monitor."""
    for pool in pools:
        if not pool.is_in_state("stopped"):
            pool.stop()
    await advance(loop, 30.0)
    for pool in pools:
        assert pool.is_in_state("stopped")


def make_agent(loop, cls=HttpAgent, **opts):
    base = {"spares": 1, "maximum": 2, "recovery": RECOVERY, "loop": loop}
    base.update(opts)
    return cls(base)


def makers(loop):
    return [
        ("pool", lambda od: Kit(loop, od=None, outlierDetection=od)),
        ("http agent", lambda od: make_agent(loop, outlierDetection=od)),
        ("https agent", lambda od: make_agent(loop, HttpsAgent,
                                              outlierDetection=od)),
    ]


def test_validation_matrix():
    async def body(loop):
        for what, make in makers(loop):
            for bad in BAD_TYPE:
                with pytest.raises(TypeError):
                    make(bad)
            for bad in BAD_VALUE:
                with pytest.raises(ValueError):
                    make(bad)
        await settle(loop)
    run_vt(body)


def test_defaults_of_a_pool():
    async def body(loop):
        kit = Kit(loop, od={})
        assert kit.pool.p_od == {
            "consecutiveFailures": 5, "baseEjectionTime": 30000,
            "maxEjectionTime": 300000, "maxEjectionPercent": 50,
            "countClose": True, "countSocketClose": True}
        assert kit.pool.get_outlier_stats()["enabled"] is True
        given = {"consecutiveFailures": 1, "baseEjectionTime": 0.5,
                 "maxEjectionTime": 0.5, "maxEjectionPercent": 100,
                 "countClose": False, "countSocketClose": False}
        full = Kit(loop, od=given)
        assert full.pool.p_od == given
        # the caller's dict is not the pool's
        assert full.pool.p_od is not given
        off = Kit(loop, od=None, outlierDetection=None)
        assert off.pool.p_od is None
        await stop_pools(loop, kit.pool, full.pool, off.pool)
    run_vt(body)


def test_defaults_differ_for_agent_pools():
    assert mod_utils.assert_outlier_detection({}) is None
    od = mod_utils.assert_outlier_detection(
        {"outlierDetection": {}}, count_default=False)
    assert od["countClose"] is False and od["countSocketClose"] is False
    od = mod_utils.assert_outlier_detection(
        {"outlierDetection": {"countClose": True}}, count_default=False)
    assert od["countClose"] is True and od["countSocketClose"] is False


@pytest.mark.parametrize("cls", [HttpAgent, HttpsAgent])
def test_agent_pools_receive_the_option(cls):
    async def body(loop):
        agent = make_agent(loop, cls, initialDomains=["127.0.0.1"],
                           outlierDetection={"consecutiveFailures": 3,
                                             "baseEjectionTime": 400})
        agent.create_pool("127.0.0.2")
        for host in ("127.0.0.1", "127.0.0.2"):
            pool = agent.get_pool(host)
            assert pool.p_od == {
                "consecutiveFailures": 3, "baseEjectionTime": 400,
                "maxEjectionTime": 300000, "maxEjectionPercent": 50,
                "countClose": False, "countSocketClose": False}
            assert pool.get_outlier_stats()["enabled"] is True
        assert sorted(agent.get_outlier_stats()) == ["127.0.0.1",
                                                     "127.0.0.2"]

        explicit = make_agent(loop, cls, initialDomains=["127.0.0.1"],
                              outlierDetection={"countClose": True})
        pool = explicit.get_pool("127.0.0.1")
        assert pool.p_od["countClose"] is True
        assert pool.p_od["countSocketClose"] is False

        plain = make_agent(loop, cls, initialDomains=["127.0.0.1"])
        pool = plain.get_pool("127.0.0.1")
        assert plain.get_outlier_stats() == {"127.0.0.1": {
            "enabled": False, "ejected": 0, "backends": {}}}
        assert not any("_od" in k for k in instance_vars(pool))

        # forwarding: unknown hosts are an error, unknown keys are not
        assert agent.eject_backend("127.0.0.1", "nope", 1000) is False
        assert agent.reinstate_backend("127.0.0.1", "nope") is False
        with pytest.raises(CueballError):
            agent.eject_backend("no.such.host", "nope", 1000)
        with pytest.raises(CueballError):
            agent.reinstate_backend("no.such.host", "nope")
        with pytest.raises(ValueError):
            plain.eject_backend("127.0.0.1", "nope")
        pools = [p for a in (agent, explicit, plain)
                 for p in a.pools.values()]
        for a in (agent, explicit, plain):
            a.stop()
        await stop_pools(loop, *pools)
    run_vt(body)


def test_agent_forwards_to_the_hosts_pool():
    async def body(loop):
        agent = make_agent(loop, initialDomains=["127.0.0.1", "127.0.0.2"])
        calls = []
        for host in ("127.0.0.1", "127.0.0.2"):
            pool = agent.get_pool(host)
            pool.eject_backend = lambda key, ms=None, host=host: \
                calls.append(("eject", host, key, ms)) or True
            pool.reinstate_backend = lambda key, host=host: \
                calls.append(("reinstate", host, key)) or True
        assert agent.eject_backend("127.0.0.2", "k", 250) is True
        assert agent.eject_backend("127.0.0.1", "k") is True
        assert agent.reinstate_backend("127.0.0.2", "k") is True
        assert calls == [("eject", "127.0.0.2", "k", 250),
                         ("eject", "127.0.0.1", "k", None),
                         ("reinstate", "127.0.0.2", "k")]
        pools = list(agent.pools.values())
        agent.stop()
        await stop_pools(loop, *pools)
    run_vt(body)


def test_pool_without_the_option_is_unchanged():
    async def body(loop):
        kit = Kit(loop, od=None)
        pool = kit.pool
        await settle(loop)
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert pool.get_outlier_stats() == {
            "enabled": False, "ejected": 0, "backends": {
                k: {"consecutiveFailures": 0, "failures": 0,
                    "successes": 0, "ejected": False, "ejections": 0,
                    "ejectedForMs": None, "reinstatesInMs": None}
                for k in ("b1", "b2", "b3")}}
        # leases fail all day long: nothing is watched, counted or set
        for _ in range(8):
            box = await kit.claim()
            await kit.end(box, "close")
        box = await kit.claim()
        box["hdl"].report_failure()
        await kit.end(box, "release")
        await advance(loop, 60.0)
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert kit.events == [] and kit.ejected() == []
        counters = pool.get_stats()["counters"]
        for name in ("backend-ejected", "backend-reinstated",
                     "ejection-refused"):
            assert name not in counters
        assert "cueball_pool_ejected_backends" not in \
            pool.p_collector.collect()
        for slot in kit.slots("b1") + kit.slots("b2") + kit.slots("b3"):
            assert len(slot.listeners("stateChanged")) == 1
        await kit.stop()
    run_vt(body)
