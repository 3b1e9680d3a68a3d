"""``claim({"avoidBackends": [...]})`` and ``ClaimHandle.get_backend()``:
a soft preference among the idle slots, on a VirtualLoop with fake
connections.  Smallest shape: two backends, spares 2, one idle slot
each."""

import pytest

from cueball_amd.errors import ClaimTimeoutError
from cueball_amd.pool import ConnectionPool
from cueball_amd.resolver import ResolverFSM
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)
from conftest import run_vt
from retry_kit import idle_keys

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 0}}


async def make_pool(loop, avoid_growth=True, **opts):
    """Two backends, one idle slot each.  `maximum` 2 keeps the pool
    from opening more when both are claimed."""
    resolver = DummyResolver()
    rfsm = ResolverFSM(resolver, {"loop": loop})

    def constructor(backend):
        c = DummyConnection(backend)
        c.key = backend["key"]
        loop.call_soon(c.connect)
        return c

    base = {"constructor": constructor, "recovery": RECOVERY, "loop": loop,
            "domain": "foobar", "spares": 2,
            "maximum": 2 if avoid_growth else 4, "resolver": rfsm}
    base.update(opts)
    pool = ConnectionPool(base)
    rfsm.start()
    resolver.add("b1", {"address": "10.0.0.1", "port": 80})
    resolver.add("b2", {"address": "10.0.0.2", "port": 80})
    await settle(loop)
    await advance(loop, 0.01)
    assert sorted(idle_keys(pool)) == ["b1", "b2"]
    return pool


def claim(pool, options):
    box = {}

    def cb(err, hdl=None, conn=None):
        box.update(err=err, hdl=hdl, conn=conn,
                   key=None if conn is None else conn.key)

    box["waiter"] = pool.claim(options, cb)
    return box


async def stop(loop, pool):
    pool.stop()
    await advance(loop, 10.0)
    assert pool.is_in_state("stopped")


def test_avoiding_the_head_yields_the_other_slot():
    async def body(loop):
        pool = await make_pool(loop)
        head = pool.p_idleq.peek()
        head_key, other_key = idle_keys(pool)
        box = claim(pool, {"avoidBackends": [head_key]})
        await settle(loop)
        assert box["err"] is None and box["key"] == other_key
        # the head was passed over, not moved
        assert pool.p_idleq.peek() is head
        assert idle_keys(pool) == [head_key]
        assert head.p_idleq_node is not None and head.is_in_state("idle")
        box["hdl"].release()
        await settle(loop)
        assert idle_keys(pool) == [head_key, other_key]
        await stop(loop, pool)
    run_vt(body)


def test_avoiding_every_idle_backend_yields_the_head():
    async def body(loop):
        pool = await make_pool(loop)
        head_key, other_key = idle_keys(pool)
        # any iterable of keys will do
        box = claim(pool, {"avoidBackends": {head_key, other_key}})
        await settle(loop)
        assert box["err"] is None and box["key"] == head_key
        assert idle_keys(pool) == [other_key]
        assert pool.get_stats()["counters"].get("queued-claim", 0) == 0
        box["hdl"].release()
        await settle(loop)
        await stop(loop, pool)
    run_vt(body)


def test_nothing_idle_queues_and_is_served_by_whatever_frees_up():
    async def body(loop):
        pool = await make_pool(loop)
        first = claim(pool, {})
        second = claim(pool, {})
        await settle(loop)
        assert {first["key"], second["key"]} == {"b1", "b2"}
        assert idle_keys(pool) == []

        waiting = claim(pool, {"avoidBackends": ["b1", "b2"],
                               "timeout": 500})
        await settle(loop)
        assert "err" not in waiting
        st = pool.get_stats()
        assert st["waiterCount"] == 1
        assert st["counters"]["queued-claim"] == 1
        # the first slot freed serves it, avoided or not
        first["hdl"].release()
        await settle(loop)
        assert waiting["err"] is None and waiting["key"] == first["key"]
        assert pool.get_stats()["waiterCount"] == 0

        # and it still obeys its timeout
        late = claim(pool, {"avoidBackends": [second["key"]],
                            "timeout": 500})
        await advance(loop, 0.4)
        assert "err" not in late
        await advance(loop, 0.2)
        assert isinstance(late["err"], ClaimTimeoutError)
        assert pool.get_stats()["waiterCount"] == 0
        assert pool.get_stats()["counters"]["claim-timeout"] == 1

        waiting["hdl"].release()
        second["hdl"].release()
        await settle(loop)
        await stop(loop, pool)
    run_vt(body)


def test_a_stale_entry_ahead_of_the_match_is_unlinked():
    async def body(loop):
        pool = await make_pool(loop, avoid_growth=False)
        head = pool.p_idleq.peek()
        head_key, other_key = idle_keys(pool)
        seen = {}
        box = claim(pool, {"avoidBackends": [head_key]})

        def probe(st):
            # runs right after the claim's ticket, in the same emit
            if st == "waiting" and not seen:
                seen["node"] = head.p_idleq_node
                seen["idle"] = idle_keys(pool)
                seen["pool_heard"] = \
                    head not in pool.p_connections.get(head_key, ())

        box["waiter"].on("stateChanged", probe)
        # The head stops being idle now; the pool hears of it only
        # after the claim's first look at the queue.
        head.set_unwanted()
        assert not head.is_in_state("idle")
        assert head.p_idleq_node is not None
        await settle(loop)
        assert seen == {"node": None, "idle": [], "pool_heard": False}
        assert box["err"] is None and box["key"] == other_key
        await advance(loop, 0.01)
        box["hdl"].release()
        await settle(loop)
        await stop(loop, pool)
    run_vt(body)


def test_unknown_keys_are_ignored_and_empty_is_no_option():
    async def body(loop):
        pool = await make_pool(loop)
        head_key, other_key = idle_keys(pool)
        for avoid in (["nope"], ["nope", "neither"], [], (), None, set()):
            box = claim(pool, {"avoidBackends": avoid})
            await settle(loop)
            assert box["err"] is None and box["key"] == head_key, avoid
            box["hdl"].release()
            await settle(loop)
            # released slots go to the tail
            head_key, other_key = other_key, head_key
            assert idle_keys(pool) == [head_key, other_key]
        # an unknown key next to a known one
        box = claim(pool, {"avoidBackends": ["nope", head_key]})
        await settle(loop)
        assert box["key"] == other_key
        box["hdl"].release()
        await settle(loop)
        await stop(loop, pool)
    run_vt(body)


@pytest.mark.parametrize("bad", ["b1", b"b1", 7, {"b1": True}, [1], [None],
                                 ["b1", 2], True])
def test_bad_types_raise(bad):
    async def body(loop):
        pool = await make_pool(loop)
        with pytest.raises(TypeError):
            pool.claim({"avoidBackends": bad}, lambda *a: None)
        assert pool.get_stats()["counters"].get("claim", 0) == 0
        await stop(loop, pool)
    run_vt(body)


def test_on_a_target_claim_delay_pool():
    async def body(loop):
        pool = await make_pool(loop, targetClaimDelay=500)
        head = pool.p_idleq.peek()
        head_key, other_key = idle_keys(pool)
        box = claim(pool, {"avoidBackends": [head_key]})
        await settle(loop)
        assert box["err"] is None and box["key"] == other_key
        assert pool.p_idleq.peek() is head
        with pytest.raises(ValueError):
            pool.claim({"avoidBackends": [head_key], "timeout": 100},
                       lambda *a: None)
        box["hdl"].release()
        await settle(loop)
        await stop(loop, pool)
    run_vt(body)


def test_get_backend():
    async def body(loop):
        pool = await make_pool(loop)
        head_key, other_key = idle_keys(pool)
        box = claim(pool, {"avoidBackends": [head_key]})
        assert box["waiter"].get_backend() is None      # still waiting
        await settle(loop)
        hdl = box["hdl"]
        assert hdl is box["waiter"]
        assert hdl.get_backend() is pool.p_backends[other_key]
        assert hdl.get_backend()["key"] == other_key
        hdl.release()
        assert hdl.get_backend() is None
        await settle(loop)

        # a plain claim's handle has it too, and loses it on close
        box = claim(pool, {})
        await settle(loop)
        assert box["hdl"].get_backend()["key"] == box["key"]
        box["hdl"].close()
        assert box["hdl"].get_backend() is None
        await settle(loop)

        # a handle that never held a slot
        box = claim(pool, {})
        box["waiter"].cancel()
        await settle(loop)
        assert box["waiter"].get_backend() is None and "err" not in box
        await stop(loop, pool)
    run_vt(body)


def test_a_claim_without_the_option_is_a_plain_claim():
    """Same claims on two pools, one of which has also served avoiding
    claims: what the plain claims count is the same."""
    async def body(loop):
        plain = await make_pool(loop)
        mixed = await make_pool(loop)

        async def plain_round(pool):
            a = claim(pool, {})
            b = claim(pool, {"errorOnEmpty": False})
            c = claim(pool, {"timeout": 300})
            await settle(loop)
            assert "err" not in c               # queued
            a["hdl"].release()
            await settle(loop)
            assert c["err"] is None
            for box in (b, c):
                box["hdl"].release()
            await settle(loop)

        await plain_round(plain)
        before = dict(mixed.get_stats()["counters"])
        assert before == {}
        box = claim(mixed, {"avoidBackends": [idle_keys(mixed)[0]]})
        await settle(loop)
        box["hdl"].release()
        await settle(loop)
        # an avoiding claim served from the idle queue counts one claim
        assert mixed.get_stats()["counters"] == {"claim": 1}
        await plain_round(mixed)

        want = dict(plain.get_stats()["counters"])
        assert want["claim"] == 3 and want["queued-claim"] == 1
        got = dict(mixed.get_stats()["counters"])
        got["claim"] -= 1
        assert got == want
        assert plain.get_stats().keys() == mixed.get_stats().keys()
        await stop(loop, plain)
        await stop(loop, mixed)
    run_vt(body)
