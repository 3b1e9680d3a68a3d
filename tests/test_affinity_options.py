"""``claimAffinity`` and ``affinityKey``: validation and defaults on
pools and agents, and a pool without the option staying exactly what it
was."""

import math

import pytest

from cueball_amd import affinity as mod_affinity
from cueball_amd import utils as mod_utils
from cueball_amd.agent import HttpAgent, HttpsAgent
from cueball_amd.testing import advance, settle
from conftest import run_vt
from balance_kit import PLAIN_POOL_VARS, RECOVERY, Kit, instance_vars

BAD_TYPE = [
    5, "on", True, 1.25, [("loadFactor", 2)],
    {"loadFactor": "1.25"}, {"loadFactor": True}, {"loadFactor": [2]},
    {"loadFactor": (5, 4)},
]
BAD_VALUE = [
    {"loadFactor": 0.99}, {"loadFactor": 0}, {"loadFactor": -2},
    {"loadFactor": math.inf}, {"loadFactor": math.nan},
    {"loadfactor": 2}, {"enabled": True}, {"loadFactor": 2, "bound": 3},
]
GOOD = [
    ({}, 1.25),
    ({"loadFactor": 1.25}, 1.25),
    ({"loadFactor": 1}, 1),
    ({"loadFactor": 1.0}, 1.0),
    ({"loadFactor": 3}, 3),
    ({"loadFactor": None}, None),
]


def make_agent(loop, cls=HttpAgent, **opts):
    base = {"spares": 1, "maximum": 2, "recovery": RECOVERY, "loop": loop}
    base.update(opts)
    return cls(base)


def makers(loop):
    return [
        ("pool", lambda af: Kit(loop, claimAffinity=af)),
        ("http agent", lambda af: make_agent(loop, claimAffinity=af)),
        ("https agent", lambda af: make_agent(loop, HttpsAgent,
                                              claimAffinity=af)),
    ]


async def stop_pools(loop, *pools):
    for pool in pools:
        if not pool.is_in_state("stopped"):
            pool.stop()
    await advance(loop, 30.0)
    for pool in pools:
        assert pool.is_in_state("stopped")


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


def test_defaults_and_accepted_values():
    async def body(loop):
        pools = []
        for given, factor in GOOD:
            kit = Kit(loop, claimAffinity=given)
            pools.append(kit.pool)
            st = kit.pool.get_affinity_stats()
            assert st["enabled"] is True
            assert st["loadFactor"] == factor
            assert (st["claims"], st["hits"], st["spilledBusy"],
                    st["spilledLoad"], st["queued"]) == (0, 0, 0, 0, 0)
            assert st["backends"] == {}
            assert kit.pool.get_affinity_order(b"k0") == []
            agent = make_agent(loop, claimAffinity=given)
            assert agent.cba_affinity["loadFactor"] == factor
        await stop_pools(loop, *pools)
    run_vt(body)


def test_the_validated_option():
    assert mod_utils.assert_claim_affinity({}) is None
    assert mod_utils.assert_claim_affinity({"claimAffinity": None}) is None
    af = mod_utils.assert_claim_affinity({"claimAffinity": {}})
    assert af == {"loadFactor": 1.25, "loadFraction": (5, 4)}
    assert mod_affinity.DEFAULT_LOAD_FACTOR == 1.25
    af = mod_utils.assert_claim_affinity(
        {"claimAffinity": {"loadFactor": 1.1}})
    assert af["loadFraction"] == (11, 10)
    af = mod_utils.assert_claim_affinity(
        {"claimAffinity": {"loadFactor": None}})
    assert af == {"loadFactor": None, "loadFraction": None}


def test_a_plain_pool_is_what_it_was():
    async def body(loop):
        kit = await Kit(loop, per=1).up()
        pool = kit.pool
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert pool.get_affinity_stats() == {"enabled": False}
        with pytest.raises(ValueError):
            pool.get_affinity_order(b"k0")
        with pytest.raises(ValueError):
            pool.get_affinity_order("k0")
        with pytest.raises(TypeError):
            pool.get_affinity_order(7)
        for key in (b"k0", "k0", b"", ""):
            with pytest.raises(ValueError):
                pool.claim({"affinityKey": key}, lambda *a: None)
        for bad in (7, 1.5, ("k0",), bytearray(b"k0"), True):
            with pytest.raises(TypeError):
                pool.claim({"affinityKey": bad}, lambda *a: None)
        # nothing was counted, linked or handed out on the way
        assert kit.counter("claim") == 0
        assert pool.get_stats()["idleConnections"] == 2
        # None is no key
        assert await kit.lease(1, {"affinityKey": None}) == "b1"
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert "cueball_pool_affinity_hit_ratio" not in \
            pool.p_collector.collect()
        await kit.stop()
    run_vt(body)


def test_key_types_on_an_opted_in_pool():
    async def body(loop):
        kit = await Kit(loop, per=1, claimAffinity={}).up()
        pool = kit.pool
        for bad in (7, 1.5, ("k0",), bytearray(b"k0"), True, ["k0"]):
            with pytest.raises(TypeError):
                pool.claim({"affinityKey": bad}, lambda *a: None)
            with pytest.raises(TypeError):
                pool.get_affinity_order(bad)
        assert kit.counter("claim") == 0
        # the empty key is a key
        assert pool.get_affinity_order(b"") == pool.get_affinity_order("")
        assert sorted(pool.get_affinity_order(b"")) == ["b1", "b2"]
        got = await kit.lease(1, {"affinityKey": b""})
        assert got == pool.get_affinity_order(b"")[0]
        assert kit.counter("affinity-claim") == 1
        await kit.stop()
    run_vt(body)


def test_only_the_option_adds_instance_variables():
    async def body(loop):
        kit = Kit(loop, claimAffinity={})
        extra = set(instance_vars(kit.pool)) - PLAIN_POOL_VARS
        assert extra == {"p_af", "p_af_hashes", "p_af_placed", "claim",
                         "_af_gauge"}
        both = Kit(loop, lb={}, claimAffinity={})
        assert both.pool.claim.__func__ is \
            type(both.pool)._claim_balanced
        await stop_pools(loop, kit.pool, both.pool)
    run_vt(body)
