"""``ConnectionPool.has_idle_connection()``: a read-only look at the
idle queue, on a VirtualLoop with fake connections.  Smallest shape:
two backends, one idle slot each."""

import pytest

from cueball_amd.testing import advance, settle
from conftest import run_vt
from retry_kit import idle_keys
from test_claim_avoid import claim, make_pool, stop


def test_with_and_without_avoid_backends():
    async def body(loop):
        pool = await make_pool(loop)
        head = pool.p_idleq.peek()
        head_key, other_key = idle_keys(pool)
        assert pool.has_idle_connection() is True
        assert pool.has_idle_connection(None) is True
        assert pool.has_idle_connection([head_key]) is True
        assert pool.has_idle_connection((other_key,)) is True
        # any iterable of keys, as for claim()
        assert pool.has_idle_connection({head_key, other_key}) is False
        assert pool.has_idle_connection(
            k for k in (other_key, head_key)) is False
        # keys the pool does not know avoid nothing
        assert pool.has_idle_connection(["nope"]) is True
        assert pool.has_idle_connection([]) is True
        # nothing was moved, unlinked or counted
        assert idle_keys(pool) == [head_key, other_key]
        assert pool.p_idleq.peek() is head
        assert pool.get_stats()["counters"] == {}

        box = claim(pool, {"avoidBackends": [head_key]})
        await settle(loop)
        assert box["key"] == other_key
        assert pool.has_idle_connection() is True
        assert pool.has_idle_connection([other_key]) is True
        assert pool.has_idle_connection([head_key]) is False
        second = claim(pool, {})
        await settle(loop)
        assert pool.has_idle_connection() is False
        assert pool.has_idle_connection([other_key]) is False
        box["hdl"].release()
        second["hdl"].release()
        await settle(loop)
        assert pool.has_idle_connection([other_key]) is True
        await stop(loop, pool)
        assert pool.has_idle_connection() is False
    run_vt(body)


def test_stale_entries_are_not_counted_and_not_unlinked():
    async def body(loop):
        pool = await make_pool(loop, avoid_growth=False)
        head = pool.p_idleq.peek()
        head_key, other_key = idle_keys(pool)
        # The head stops being idle now; its entry stays in the queue
        # until the pool hears of it, a loop turn later.
        head.set_unwanted()
        assert not head.is_in_state("idle")
        node = head.p_idleq_node
        assert node is not None
        assert pool.has_idle_connection([other_key]) is False
        assert pool.has_idle_connection([head_key]) is True
        assert pool.has_idle_connection() is True
        # read-only: the stale entry is where it was
        assert head.p_idleq_node is node
        assert pool.p_idleq.peek() is head
        assert idle_keys(pool) == [head_key, other_key]
        await settle(loop)
        await advance(loop, 0.01)
        await stop(loop, pool)
    run_vt(body)


@pytest.mark.parametrize("bad", ["b1", b"b1", 7, {"b1": True}, [1], [None],
                                 ["b1", 2], True])
def test_bad_types_raise(bad):
    async def body(loop):
        pool = await make_pool(loop)
        with pytest.raises(TypeError):
            pool.has_idle_connection(bad)
        await stop(loop, pool)
    run_vt(body)
