"""``claimQueue`` and the claim option ``priority``: validation and
defaults on pools and agents, forwarding from an agent to its pools, and
a pool without the option staying exactly what it was."""

import math

import pytest

import cueball_amd
from cueball_amd import errors as mod_errors
from cueball_amd import utils as mod_utils
from cueball_amd.agent import HttpAgent, HttpsAgent
from cueball_amd.errors import ClaimQueueFullError, CueballError
from cueball_amd.testing import advance, settle
from conftest import run_vt
from balance_kit import PLAIN_POOL_VARS, RECOVERY, Kit, instance_vars
from claim_queue_kit import QueueKit

DEFAULTS = {"maxQueued": None, "priorities": 1, "defaultPriority": 0,
            "order": "fifo", "lifoAfter": None}

BAD_TYPE = [
    5, "on", True, [("maxQueued", 2)],
    {"maxQueued": 2.0}, {"maxQueued": True}, {"maxQueued": "4"},
    {"priorities": 2.0}, {"priorities": True}, {"priorities": "2"},
    {"priorities": 2, "defaultPriority": 1.0},
    {"priorities": 2, "defaultPriority": True},
    {"defaultPriority": "0"},
    {"order": 1}, {"order": True}, {"order": ["fifo"]},
    {"order": "adaptive", "lifoAfter": "100"},
    {"order": "adaptive", "lifoAfter": True},
    {"order": "adaptive", "lifoAfter": [100]},
]
BAD_VALUE = [
    {"maxQueued": 0}, {"maxQueued": -1},
    {"priorities": 0}, {"priorities": 9}, {"priorities": -1},
    {"defaultPriority": 1}, {"defaultPriority": -1},
    {"priorities": 3, "defaultPriority": 3},
    {"order": "random"}, {"order": "LIFO"}, {"order": ""},
    {"order": "adaptive"},                    # lifoAfter is required
    {"order": "adaptive", "lifoAfter": -1},
    {"order": "adaptive", "lifoAfter": math.inf},
    {"order": "adaptive", "lifoAfter": math.nan},
    {"lifoAfter": 100}, {"order": "fifo", "lifoAfter": 100},
    {"order": "lifo", "lifoAfter": 100},
    {"maxQueue": 2}, {"enabled": True}, {"priority": 1},
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
        ("pool", lambda cq: QueueKit(loop, claimQueue=cq)),
        ("http agent", lambda cq: make_agent(loop, claimQueue=cq)),
        ("https agent", lambda cq: make_agent(loop, HttpsAgent,
                                              claimQueue=cq)),
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


def test_the_validator_itself():
    check = mod_utils.assert_claim_queue
    assert check({}) is None
    assert check({"claimQueue": None}) is None
    assert check({"claimQueue": {}}) == DEFAULTS
    assert check({"claimQueue": {"maxQueued": None}}) == DEFAULTS
    for n in range(1, 9):
        got = check({"claimQueue": {"priorities": n,
                                    "defaultPriority": n - 1}})
        assert got["priorities"] == n and got["defaultPriority"] == n - 1
    assert check({"claimQueue": {"order": "adaptive", "lifoAfter": 0}}
                 )["lifoAfter"] == 0
    # under "adaptive", targetClaimDelay is the default of lifoAfter
    got = check({"targetClaimDelay": 250,
                 "claimQueue": {"order": "adaptive"}})
    assert got["lifoAfter"] == 250 and got["order"] == "adaptive"
    got = check({"targetClaimDelay": 250,
                 "claimQueue": {"order": "adaptive", "lifoAfter": 40}})
    assert got["lifoAfter"] == 40
    # and only there
    assert check({"targetClaimDelay": 250, "claimQueue": {"order": "lifo"}}
                 )["lifoAfter"] is None


def test_defaults_of_a_pool():
    async def body(loop):
        kit = QueueKit(loop, {})
        assert kit.pool.p_cq == DEFAULTS
        assert kit.pool.get_queue_stats() == {
            "enabled": True, "maxQueued": None, "priorities": 1,
            "order": "fifo", "lifo": False, "queued": [0], "rejected": 0,
            "shed": 0, "lifoPlaced": 0}
        given = {"maxQueued": 7, "priorities": 3, "defaultPriority": 2,
                 "order": "adaptive", "lifoAfter": 50}
        full = QueueKit(loop, given)
        assert full.pool.p_cq == given
        assert full.pool.p_cq is not given
        st = full.pool.get_queue_stats()
        assert st["maxQueued"] == 7 and st["priorities"] == 3
        assert st["order"] == "adaptive" and st["queued"] == [0, 0, 0]
        assert st["lifo"] is False
        newest = QueueKit(loop, {"order": "lifo"})
        assert newest.pool.get_queue_stats()["lifo"] is True
        off = QueueKit(loop, claimQueue=None)
        assert off.pool.p_cq is None
        assert off.pool.get_queue_stats() == {"enabled": False}
        await stop_pools(loop, kit.pool, full.pool, newest.pool, off.pool)
    run_vt(body)


def test_the_error_class():
    assert cueball_amd.ClaimQueueFullError is ClaimQueueFullError
    assert "ClaimQueueFullError" in cueball_amd.__all__
    assert "ClaimQueueFullError" in mod_errors.__all__
    assert issubclass(ClaimQueueFullError, CueballError)
    pool = object()
    err = ClaimQueueFullError(pool)
    assert err.pool is pool and err.displaced is False
    assert ClaimQueueFullError(pool, True).displaced is True
    assert "full" in str(err)


def test_a_pool_without_the_option_is_unchanged():
    async def body(loop):
        kit = await QueueKit(loop).up()
        pool = kit.pool
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert pool.get_queue_stats() == {"enabled": False}
        assert "claim" not in instance_vars(pool)
        on = await QueueKit(loop, {"maxQueued": 1}).up()
        assert set(instance_vars(on.pool)) - PLAIN_POOL_VARS == {
            "claim", "p_cq", "p_cq_since", "_cq_gauge"}
        many = QueueKit(loop, {"priorities": 2})
        assert set(instance_vars(many.pool)) - PLAIN_POOL_VARS == {
            "claim", "p_cq", "p_cq_since", "p_cq_last", "_cq_gauge"}
        assert pool.get_stats().keys() == on.pool.get_stats().keys() == {
            "counters", "totalConnections", "idleConnections",
            "pendingConnections", "waiterCount"}
        # a plain pool queues, times out and serves as it always did
        for k in (kit, on):
            await k.busy()
            await k.queue_all(["a", "b"])
        assert kit.order() == ["a", "b"] and on.order() == ["a"]
        assert on.errors["b"].displaced is False
        await advance(loop, 1.0)        # several gauge samples
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        counters = pool.get_stats()["counters"]
        assert not [c for c in counters if c.startswith("queue-")]
        assert counters["queued-claim"] == 2
        assert on.pool.get_stats()["counters"]["queue-rejected"] == 1
        assert "cueball_pool_queued_claims" not in pool.p_collector.collect()
        text = on.pool.p_collector.collect()
        assert "cueball_pool_queued_claims{" in text
        assert 'priority="0"' in text
        assert await kit.serve_all() == ["a", "b"]
        assert await on.serve_all() == ["a"]
        await stop_pools(loop, kit.pool, on.pool, many.pool)
    run_vt(body)


def test_priority_on_a_plain_pool_raises():
    async def body(loop):
        kit = await QueueKit(loop).up()
        before = dict(kit.pool.get_stats()["counters"])
        for bad in (0, 1):
            with pytest.raises(ValueError):
                kit.pool.claim({"priority": bad}, lambda *a: None)
        for bad in (True, False, 0.0, "0", [0]):
            with pytest.raises(TypeError):
                kit.pool.claim({"priority": bad}, lambda *a: None)
        # None names no class
        box = kit.claim({"priority": None})
        await settle(loop)
        assert box["err"] is None
        box["hdl"].release()
        await settle(loop)
        assert kit.pool.get_stats()["counters"].get("claim", 0) == \
            before.get("claim", 0) + 1
        await kit.stop()
    run_vt(body)


def test_priority_on_a_pool_with_claim_balancing_alone_raises():
    """Such a pool has its own claim() on the instance; the rule is the
    plain pool's."""
    async def body(loop):
        kit = await QueueKit(loop, lb={"choices": "all"}).up()
        assert kit.pool.p_cq is None and kit.pool.p_lb is not None
        assert "claim" in instance_vars(kit.pool)
        before = dict(kit.pool.get_stats()["counters"])
        for bad in (0, 1):
            with pytest.raises(ValueError):
                kit.pool.claim({"priority": bad}, lambda *a: None)
        for bad in (True, False, "0", 0.0, "x", [0]):
            with pytest.raises(TypeError):
                kit.pool.claim({"priority": bad}, lambda *a: None)
        assert kit.pool.get_stats()["counters"] == before
        box = kit.claim({"priority": None})
        await settle(loop)
        assert box["err"] is None
        box["hdl"].release()
        await settle(loop)
        # with both options the class is read
        both = await QueueKit(loop, {"priorities": 2},
                              lb={"choices": "all"}).up()
        with pytest.raises(ValueError):
            both.pool.claim({"priority": 2}, lambda *a: None)
        with pytest.raises(TypeError):
            both.pool.claim({"priority": True}, lambda *a: None)
        hdl = both.pool.claim({"priority": 1}, lambda *a: None)
        assert hdl.ch_priority == 1
        hdl.cancel()
        await settle(loop)
        await stop_pools(loop, kit.pool, both.pool)
    run_vt(body)


def test_the_shared_validator_of_priority():
    check = mod_utils.assert_claim_priority
    cq = mod_utils.assert_claim_queue({"claimQueue": {"priorities": 3}})
    assert [check(p, cq) for p in (0, 1, 2)] == [0, 1, 2]
    for bad in (3, -1):
        with pytest.raises(ValueError):
            check(bad, cq)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError):
            check(bad, cq)
    with pytest.raises(ValueError, match="priority= needs an agent"):
        check(0, None, "priority=", "an agent")
    with pytest.raises(ValueError, match="options.priority needs a pool"):
        check(0, None)
    with pytest.raises(TypeError):
        check(True, None)


def test_priority_on_an_opted_in_pool():
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 3,
                                    "defaultPriority": 1}).up()
        for bad in (3, -1, 8):
            with pytest.raises(ValueError):
                kit.pool.claim({"priority": bad}, lambda *a: None)
        for bad in (True, False, 1.0, "1", [1]):
            with pytest.raises(TypeError):
                kit.pool.claim({"priority": bad}, lambda *a: None)
        with pytest.raises(TypeError):
            kit.pool.claim({"priority": 1})
        boxes = [kit.queue("p%s" % p, p) for p in (0, 1, 2, None)]
        assert [b["waiter"].ch_priority for b in boxes] == [0, 1, 2, 1]
        # claim(cb) and claim({}, cb) take the default class too
        hdl = kit.pool.claim(lambda *a: None)
        assert hdl.ch_priority == 1
        hdl.cancel()
        for b in boxes:
            b["waiter"].cancel()
        # a single class still takes its one name
        one = await QueueKit(loop, {}).up()
        only = one.queue("x", 0)["waiter"]
        assert only.ch_priority == 0
        only.cancel()
        with pytest.raises(ValueError):
            one.pool.claim({"priority": 1}, lambda *a: None)
        await settle(loop)
        await kit.stop()
        await one.stop()
    run_vt(body)


@pytest.mark.parametrize("cls", [HttpAgent, HttpsAgent])
def test_agent_pools_receive_a_copy(cls):
    async def body(loop):
        agent = make_agent(loop, cls, initialDomains=["127.0.0.1"],
                           claimQueue={"maxQueued": 5, "priorities": 2})
        agent.create_pool("127.0.0.2")
        want = dict(DEFAULTS, maxQueued=5, priorities=2)
        assert agent.cba_queue == want
        seen = []
        for host in ("127.0.0.1", "127.0.0.2"):
            pool = agent.get_pool(host)
            assert pool.p_cq == want
            assert pool.p_cq is not agent.cba_queue
            assert all(pool.p_cq is not other for other in seen)
            seen.append(pool.p_cq)
            st = agent.get_queue_stats(host)
            assert st["enabled"] is True and st["maxQueued"] == 5
            assert st == pool.get_queue_stats()
        with pytest.raises(CueballError):
            agent.get_queue_stats("no.such.host")
        # an agent has no targetClaimDelay to fall back on
        with pytest.raises(ValueError):
            make_agent(loop, cls, claimQueue={"order": "adaptive"})
        adaptive = make_agent(loop, cls, initialDomains=["127.0.0.1"],
                              claimQueue={"order": "adaptive",
                                          "lifoAfter": 30})
        assert adaptive.get_pool("127.0.0.1").p_cq["lifoAfter"] == 30

        plain = make_agent(loop, cls, initialDomains=["127.0.0.1"])
        assert plain.get_queue_stats("127.0.0.1") == {"enabled": False}
        assert "cba_queue" not in instance_vars(plain, "cba_stopped")
        assert set(instance_vars(agent, "cba_stopped")) - \
            set(instance_vars(plain, "cba_stopped")) == {"cba_queue"}
        pool = plain.get_pool("127.0.0.1")
        assert not any("_cq" in k for k in instance_vars(pool))

        # priority= is checked at the call
        for bad in (2, -1):
            with pytest.raises(ValueError):
                agent.request("127.0.0.1", priority=bad)
        for bad in (True, 1.0, "1"):
            with pytest.raises(TypeError):
                agent.request("127.0.0.1", priority=bad)
        with pytest.raises(ValueError):
            plain.request("127.0.0.1", priority=0)
        agents = (agent, adaptive, plain)
        pools = [p for a in agents for p in a.pools.values()]
        for a in agents:
            a.stop()
        await stop_pools(loop, *pools)
    run_vt(body)
