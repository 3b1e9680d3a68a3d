"""``claimBalancing``: validation and defaults on pools and agents,
forwarding from an agent to its pools, and a pool or agent without the
option staying exactly what it was."""

import math
import random

import pytest

from cueball_amd import utils as mod_utils
from cueball_amd.agent import HttpAgent, HttpsAgent
from cueball_amd.errors import CueballError
from cueball_amd.pool import ConnectionPool
from cueball_amd.testing import advance, settle
from conftest import run_vt
from balance_kit import PLAIN_POOL_VARS, RECOVERY, Kit, instance_vars

#: the instance variables of an agent created without any opt-in
#: feature, as they were before claim balancing existed
PLAIN_AGENT_VARS = {
    "_loop", "cba_conn_age_spread", "cba_err_on_empty",
    "cba_latency_stats", "cba_max_conn_age", "cba_outlier", "cba_ping",
    "cba_ping_interval", "cba_recovery", "cba_srv_ranking", "cba_stopped",
    "collector", "default_port", "keep_alive", "log", "maximum",
    "pool_external_resolvers", "pool_resolvers", "pools", "protocol",
    "resolvers", "service", "spares", "tcp_ka_delay"}

BAD_TYPE = [
    5, "on", True, [("choices", 2)],
    {"policy": 1}, {"policy": True}, {"policy": ["peakEwma"]},
    {"choices": 2.0}, {"choices": True}, {"choices": [2]},
    {"decayTime": "1000"}, {"decayTime": True}, {"decayTime": [1]},
    {"rng": 7}, {"rng": random}, {"rng": random.random}, {"rng": "seed"},
]
BAD_VALUE = [
    {"policy": "roundRobin"}, {"policy": "peakewma"}, {"policy": ""},
    {"choices": 1}, {"choices": 0}, {"choices": -2}, {"choices": "ALL"},
    {"choices": "2"},
    {"decayTime": 0}, {"decayTime": -1}, {"decayTime": math.inf},
    {"decayTime": math.nan},
    {"choice": 2}, {"enabled": True}, {"decay": 100},
]


async def stop_pools(loop, *pools):
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
        ("pool", lambda lb: Kit(loop, lb=lb)),
        ("http agent", lambda lb: make_agent(loop, claimBalancing=lb)),
        ("https agent", lambda lb: make_agent(loop, HttpsAgent,
                                              claimBalancing=lb)),
    ]


def test_validation_matrix():
    async def body(loop):
        for what, make in makers(loop):
            for bad in BAD_TYPE:
                with pytest.raises(TypeError):
                    make(bad)
                    pytest.fail("%s accepted %r" % (what, bad))
            for bad in BAD_VALUE:
                with pytest.raises(ValueError):
                    make(bad)
                    pytest.fail("%s accepted %r" % (what, bad))
        await settle(loop)
    run_vt(body)


def test_defaults_of_a_pool():
    async def body(loop):
        kit = Kit(loop, lb={})
        assert kit.pool.p_lb == {"policy": "peakEwma", "choices": 2,
                                 "decayTime": 10000, "rng": None}
        st = kit.pool.get_balancing_stats()
        assert st == {"enabled": True, "policy": "peakEwma", "choices": 2,
                      "decayTimeMs": 10000, "backends": {}}
        rng = random.Random(5)
        given = {"policy": "leastLoaded", "choices": "all",
                 "decayTime": 0.5, "rng": rng}
        full = Kit(loop, lb=given)
        assert full.pool.p_lb == given
        assert full.pool.p_lb["rng"] is rng
        # the caller's dict is not the pool's
        assert full.pool.p_lb is not given
        many = Kit(loop, lb={"choices": 7})
        assert many.pool.p_lb["choices"] == 7
        off = Kit(loop, claimBalancing=None)
        assert off.pool.p_lb is None
        assert off.pool.get_balancing_stats() == {"enabled": False}
        await stop_pools(loop, kit.pool, full.pool, many.pool, off.pool)
    run_vt(body)


def test_the_validator_itself():
    assert mod_utils.assert_claim_balancing({}) is None
    assert mod_utils.assert_claim_balancing({"claimBalancing": None}) is None
    assert mod_utils.assert_claim_balancing({"claimBalancing": {}}) == {
        "policy": "peakEwma", "choices": 2, "decayTime": 10000,
        "rng": None}


@pytest.mark.parametrize("cls", [HttpAgent, HttpsAgent])
def test_agent_pools_receive_a_copy(cls):
    async def body(loop):
        rng = random.Random(3)
        agent = make_agent(loop, cls, initialDomains=["127.0.0.1"],
                           claimBalancing={"choices": "all",
                                           "decayTime": 400, "rng": rng})
        agent.create_pool("127.0.0.2")
        want = {"policy": "peakEwma", "choices": "all", "decayTime": 400,
                "rng": rng}
        assert agent.cba_balancing == want
        seen = []
        for host in ("127.0.0.1", "127.0.0.2"):
            pool = agent.get_pool(host)
            assert pool.p_lb == want
            assert pool.p_lb is not agent.cba_balancing
            assert all(pool.p_lb is not other for other in seen)
            seen.append(pool.p_lb)
            st = agent.get_balancing_stats(host)
            assert st["enabled"] is True and st["choices"] == "all"
            assert st == pool.get_balancing_stats()
        with pytest.raises(CueballError):
            agent.get_balancing_stats("no.such.host")

        plain = make_agent(loop, cls, initialDomains=["127.0.0.1"])
        assert plain.get_balancing_stats("127.0.0.1") == {"enabled": False}
        pool = plain.get_pool("127.0.0.1")
        assert not any("_lb" in k for k in instance_vars(pool))
        pools = [p for a in (agent, plain) for p in a.pools.values()]
        for a in (agent, plain):
            a.stop()
        await stop_pools(loop, *pools)
    run_vt(body)


@pytest.mark.parametrize("cls", [HttpAgent, HttpsAgent])
def test_an_agent_without_the_option_is_unchanged(cls):
    async def body(loop):
        plain = make_agent(loop, cls)
        have = set(instance_vars(plain, "cba_stopped"))
        # the pure runtime keeps its emitter's state in the dict too
        assert PLAIN_AGENT_VARS <= have
        assert all(k.startswith("_e") for k in have - PLAIN_AGENT_VARS), \
            have - PLAIN_AGENT_VARS
        assert not [k for k in have if "balanc" in k]
        balanced = make_agent(loop, cls, claimBalancing={})
        assert set(instance_vars(balanced, "cba_stopped")) - have == \
            {"cba_balancing"}
        await settle(loop)
    run_vt(body)


def test_a_pool_without_the_option_is_unchanged():
    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert pool.get_balancing_stats() == {"enabled": False}
        # claim() is the class's, not an instance attribute
        assert "claim" not in instance_vars(pool)
        on = await Kit(loop, lb={}).up()
        assert set(instance_vars(on.pool)) - PLAIN_POOL_VARS == {
            "claim", "p_lb", "p_lb_backends", "p_lb_handed", "p_lb_open",
            "p_lb_last", "_lb_gauges"}
        assert pool.get_stats().keys() == on.pool.get_stats().keys() == {
            "counters", "totalConnections", "idleConnections",
            "pendingConnections", "waiterCount"}
        for _ in range(6):
            await kit.lease(10)
            await on.lease(10)
        await advance(loop, 1.0)        # several gauge samples
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        counters = pool.get_stats()["counters"]
        assert "balanced-claim" not in counters
        assert "balanced-reordered" not in counters
        assert on.pool.get_stats()["counters"]["balanced-claim"] == 6
        assert "cueball_pool_backend_" not in pool.p_collector.collect()
        text = on.pool.p_collector.collect()
        assert "cueball_pool_backend_latency_seconds{" in text
        assert "cueball_pool_backend_outstanding{" in text
        for fsms in pool.p_connections.values():
            for slot in fsms:
                assert len(slot.listeners("stateChanged")) == 1
        assert isinstance(pool, ConnectionPool)
        await kit.stop()
        await on.stop()
    run_vt(body)
