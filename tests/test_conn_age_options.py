"""``maxConnectionAge`` / ``connectionAgeSpread``: validation on pools
and agents, forwarding from an agent to its pools, and a pool without
the options staying exactly what it was."""

import math

import pytest

from cueball_amd.agent import HttpAgent, HttpsAgent
from cueball_amd.errors import CueballError
from cueball_amd.testing import advance, settle
from conftest import run_vt
from test_conn_age_pool import Kit, instance_vars, leap

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 0}}

BAD_TYPE = (True, False, "60000", [60000], {})
BAD_AGE = (0, -1, -0.5, math.inf, -math.inf, math.nan)
BAD_SPREAD = (-0.1, 1, 1.5, math.inf, math.nan)


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
        ("pool", lambda **o: Kit(loop, **o)),
        ("http agent", lambda **o: make_agent(loop, **o)),
        ("https agent", lambda **o: make_agent(loop, HttpsAgent, **o)),
    ]


def test_validation_matrix():
    async def body(loop):
        for what, make in makers(loop):
            for bad in BAD_TYPE:
                with pytest.raises(TypeError):
                    make(maxConnectionAge=bad)
                with pytest.raises(TypeError):
                    make(maxConnectionAge=1000, connectionAgeSpread=bad)
            for bad in BAD_AGE:
                with pytest.raises(ValueError):
                    make(maxConnectionAge=bad)
            for bad in BAD_SPREAD:
                with pytest.raises(ValueError):
                    make(maxConnectionAge=1000, connectionAgeSpread=bad)
            # a spread needs an age
            with pytest.raises(ValueError):
                make(connectionAgeSpread=0.2)
            with pytest.raises(ValueError):
                make(maxConnectionAge=None, connectionAgeSpread=0)
        await settle(loop)
    run_vt(body)


def test_valid_values_and_defaults():
    async def body(loop):
        kit = Kit(loop)
        pools = [kit.pool]
        assert kit.pool.get_connection_ages() == {
            "maxAgeMs": None, "oldestMs": None, "connections": []}
        assert kit.pool.p_age_max is None

        kit = Kit(loop, maxConnectionAge=None)
        pools.append(kit.pool)
        assert kit.pool.get_connection_ages()["maxAgeMs"] is None

        # the spread defaults to 0.2; 0 and an int age are fine
        from cueball_amd.pool import ConnectionPool
        from cueball_amd.resolver import ResolverFSM
        from cueball_amd.testing import DummyConnection, DummyResolver
        pool = ConnectionPool({
            "constructor": DummyConnection, "recovery": RECOVERY,
            "loop": loop, "domain": "foobar", "spares": 1, "maximum": 1,
            "resolver": ResolverFSM(DummyResolver(), {"loop": loop}),
            "maxConnectionAge": 1500})
        assert pool.get_connection_ages()["maxAgeMs"] == 1500
        assert pool.p_age_spread == 0.2

        kit = Kit(loop, maxConnectionAge=0.5, connectionAgeSpread=0.999)
        assert kit.pool.p_age_max == 0.5
        assert kit.pool.p_age_spread == 0.999
        await stop_pools(loop, pool, kit.pool, *pools)
    run_vt(body)


def test_ages_report_per_connection():
    async def body(loop):
        kit = Kit(loop, spares=2, maximum=2, maxConnectionAge=60_000)
        await settle(loop)
        t0 = loop.time()
        kit.conns[0].connect()
        await kit.to(t0 + 1)
        ages = kit.pool.get_connection_ages()
        assert ages["maxAgeMs"] == 60_000
        assert ages["oldestMs"] == 1000
        by_state = {c["state"]: c for c in ages["connections"]}
        assert by_state["idle"] == {
            "backend": "b1", "state": "idle", "ageMs": 1000,
            "expiresInMs": 59_000, "recycling": False}
        assert by_state["connecting"] == {
            "backend": "b1", "state": "connecting", "ageMs": None,
            "expiresInMs": None, "recycling": False}
        await kit.stop()
    run_vt(body)


@pytest.mark.parametrize("cls", [HttpAgent, HttpsAgent])
def test_agent_pools_receive_both_options(cls):
    async def body(loop):
        agent = make_agent(loop, cls, maxConnectionAge=90_000,
                           connectionAgeSpread=0.4,
                           initialDomains=["127.0.0.1"])
        agent.create_pool("127.0.0.2")
        for host in ("127.0.0.1", "127.0.0.2"):
            pool = agent.get_pool(host)
            assert pool.p_age_max == 90_000
            assert pool.p_age_spread == 0.4
            assert pool.get_connection_ages()["maxAgeMs"] == 90_000

        plain = make_agent(loop, cls, initialDomains=["127.0.0.1"])
        pool = plain.get_pool("127.0.0.1")
        assert pool.get_connection_ages()["maxAgeMs"] is None
        assert not any(k.startswith("p_age_") for k in instance_vars(pool))

        # nothing connected yet: nothing to mark
        assert agent.recycle() == 0
        assert agent.recycle("127.0.0.1") == 0
        with pytest.raises(CueballError):
            agent.recycle("no.such.host")
        pools = list(agent.pools.values()) + list(plain.pools.values())
        agent.stop()
        plain.stop()
        await stop_pools(loop, *pools)
    run_vt(body)


def test_agent_recycle_sums_over_pools():
    async def body(loop):
        agent = make_agent(loop, initialDomains=["127.0.0.1", "127.0.0.2"])
        calls = []
        for n, host in enumerate(("127.0.0.1", "127.0.0.2"), 2):
            pool = agent.get_pool(host)
            pool.recycle = lambda n=n, host=host: calls.append(host) or n
        assert agent.recycle("127.0.0.2") == 3
        assert agent.recycle() == 5
        assert calls == ["127.0.0.2", "127.0.0.1", "127.0.0.2"]
        pools = list(agent.pools.values())
        agent.stop()
        await stop_pools(loop, *pools)
    run_vt(body)


def test_pool_without_the_options_is_unchanged():
    async def body(loop):
        kit = Kit(loop, spares=4, maximum=8)
        pool = kit.pool
        await settle(loop)
        await kit.connect_new()
        assert len(kit.conns) == 4
        assert not any(k.startswith("p_age_") for k in instance_vars(pool))
        assert pool.p_age_timer is None

        # a day goes by: ten minutes sample by sample, the rest hour
        # by hour
        await advance(loop, 600.0)
        for _ in range(24):
            await leap(loop, 3600.0)
        assert kit.dead() == []
        assert len(kit.conns) == 4
        assert pool.get_stats()["idleConnections"] == 4
        assert not any(k.startswith("p_age_") for k in instance_vars(pool))
        counters = pool.get_stats()["counters"]
        assert "recycled-age" not in counters
        assert "recycled-manual" not in counters
        assert kit.events == []
        ages = pool.get_connection_ages()
        assert ages["maxAgeMs"] is None
        assert [c["expiresInMs"] for c in ages["connections"]] == [None] * 4
        assert ages["oldestMs"] == pytest.approx(87_000_000)
        await kit.stop()
    run_vt(body)
