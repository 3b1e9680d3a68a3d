"""A pool with ``claimQueue`` on a VirtualLoop with fake connections:
one backend with two connections, both claimed before each case, so
that every further claim has to wait."""

import pytest

from cueball_amd.errors import (ClaimQueueFullError, ClaimTimeoutError,
                                PoolFailedError, PoolStoppingError)
from cueball_amd.testing import advance, settle
from conftest import run_vt
from claim_queue_kit import QueueKit


def counters(kit):
    return kit.pool.get_stats()["counters"]


def test_fifo_bound_rejects_the_newcomer():
    async def body(loop):
        kit = await QueueKit(loop, {"maxQueued": 3}).up()
        await kit.busy()
        await kit.queue_all(["a", "b", "c", "d"])
        assert kit.log == [("d", "ClaimQueueFullError")]
        err = kit.errors["d"]
        assert isinstance(err, ClaimQueueFullError)
        assert err.displaced is False and err.pool is kit.pool
        assert kit.order() == ["a", "b", "c"]
        st = kit.queue_stats()
        assert st["queued"] == [3] and st["rejected"] == 1
        assert st["shed"] == 0 and st["lifoPlaced"] == 0
        assert counters(kit)["queue-rejected"] == 1
        assert "queue-shed" not in counters(kit)
        assert "queue-lifo" not in counters(kit)
        # the rejected claim was never linked, nor counted as queued
        assert counters(kit)["queued-claim"] == 3
        assert counters(kit)["max-claim-queue"] == 3
        assert getattr(kit.boxes["d"]["waiter"], "ch_waiter_node",
                       None) is None
        assert await kit.serve_all() == ["a", "b", "c"]
        # room again
        await kit.busy()
        await kit.queue_all(["e"])
        assert kit.order() == ["e"]
        assert await kit.serve_all() == ["e"]
        assert kit.queue_stats()["queued"] == [0]
        assert all(b["fired"] == 1 for b in kit.boxes.values())
        await kit.stop()
    run_vt(body)


def test_two_classes_are_served_in_class_then_arrival_order():
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 2}).up()
        await kit.busy()
        await kit.queue_all([("a", 1), ("b", 1), ("c", 0), ("d", 1),
                             ("e", 0)])
        assert kit.order() == ["c", "e", "a", "b", "d"]
        assert kit.queue_stats()["queued"] == [2, 3]
        assert await kit.serve_all() == ["c", "e", "a", "b", "d"]
        assert kit.queue_stats()["queued"] == [0, 0]
        assert not [c for c in counters(kit) if c.startswith("queue-")]
        await kit.stop()
    run_vt(body)


def test_default_priority_names_the_class_of_plain_claims():
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 3,
                                    "defaultPriority": 1}).up()
        await kit.busy()
        await kit.queue_all(["a", ("b", 2), ("c", 0), "d", ("e", 1)])
        assert kit.order() == ["c", "a", "d", "e", "b"]
        assert kit.queue_stats()["queued"] == [1, 3, 1]
        assert await kit.serve_all() == ["c", "a", "d", "e", "b"]
        await kit.stop()
    run_vt(body)


def test_a_more_urgent_claim_displaces_the_newest_of_the_least_urgent():
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 2, "maxQueued": 4}).up()
        await kit.busy()
        await kit.queue_all([("a", 1), ("b", 1), ("c", 1), ("d", 1)])
        assert kit.log == []
        kit.queue("u", 0)
        await settle(loop)
        assert kit.log == [("d", "ClaimQueueFullError")]
        assert kit.errors["d"].displaced is True
        assert kit.order() == ["u", "a", "b", "c"]
        assert counters(kit)["queue-shed"] == 1
        assert "queue-rejected" not in counters(kit)
        assert kit.boxes["d"]["waiter"].ch_waiter_node is None
        assert kit.boxes["d"]["waiter"].is_in_state("failed")
        # a further claim of the least urgent class rejects itself
        kit.queue("e", 1)
        await settle(loop)
        assert kit.log[-1] == ("e", "ClaimQueueFullError")
        assert kit.errors["e"].displaced is False
        assert kit.order() == ["u", "a", "b", "c"]
        st = kit.queue_stats()
        assert st["queued"] == [1, 3]
        assert (st["rejected"], st["shed"]) == (1, 1)
        assert counters(kit)["max-claim-queue"] == 4
        # a queue full of the most urgent class rejects that class too
        await kit.queue_all([("v", 0), ("w", 0), ("x", 0)])
        assert kit.order() == ["u", "v", "w", "x"]
        kit.queue("y", 0)
        await settle(loop)
        assert kit.errors["y"].displaced is False
        assert [kit.errors[k].displaced for k in "cba"] == [True] * 3
        assert await kit.serve_all() == ["u", "v", "w", "x"]
        assert all(b["fired"] == 1 for b in kit.boxes.values())
        await kit.stop()
    run_vt(body)


def test_lifo_serves_newest_first_and_sheds_the_oldest():
    async def body(loop):
        kit = await QueueKit(loop, {"order": "lifo", "maxQueued": 3}).up()
        await kit.busy()
        assert kit.queue_stats()["lifo"] is True
        await kit.queue_all(["a", "b", "c"])
        assert kit.order() == ["c", "b", "a"]
        await kit.queue_all(["d"])
        assert kit.log == [("a", "ClaimQueueFullError")]
        assert kit.errors["a"].displaced is True
        assert kit.order() == ["d", "c", "b"]
        st = kit.queue_stats()
        assert (st["rejected"], st["shed"], st["lifoPlaced"]) == (0, 1, 4)
        assert counters(kit)["queue-lifo"] == 4
        assert await kit.serve_all() == ["d", "c", "b"]
        await kit.stop()
    run_vt(body)


def test_lifo_within_classes():
    async def body(loop):
        kit = await QueueKit(loop, {"order": "lifo", "priorities": 3,
                                    "maxQueued": 5}).up()
        await kit.busy()
        await kit.queue_all([("a", 1), ("b", 2), ("c", 1), ("d", 0),
                             ("e", 2)])
        assert kit.order() == ["d", "c", "a", "e", "b"]
        # full: the oldest of the least urgent class goes, even for a
        # claim of its own class
        await kit.queue_all([("f", 2)])
        assert kit.errors["b"].displaced is True
        assert kit.order() == ["d", "c", "a", "f", "e"]
        await kit.queue_all([("g", 0)])
        assert kit.errors["e"].displaced is True
        assert kit.order() == ["g", "d", "c", "a", "f"]
        assert await kit.serve_all() == ["g", "d", "c", "a", "f"]
        await kit.stop()
    run_vt(body)


def test_adaptive_turns_newest_first_once_the_queue_stands():
    async def body(loop):
        kit = await QueueKit(loop, {"order": "adaptive",
                                    "lifoAfter": 100}).up()
        await kit.busy()
        assert kit.queue_stats()["lifo"] is False
        await kit.queue_all(["a"])
        await advance(loop, 0.04)
        await kit.queue_all(["b"])
        await advance(loop, 0.04)
        await kit.queue_all(["c"])            # at 80 ms
        assert kit.order() == ["a", "b", "c"]
        assert kit.queue_stats()["lifo"] is False
        await advance(loop, 0.07)             # 150 ms
        assert kit.queue_stats()["lifo"] is True
        await kit.queue_all(["d"])
        assert kit.order() == ["d", "a", "b", "c"]
        assert counters(kit)["queue-lifo"] == 1
        # dequeues do not reset it: the queue has not emptied
        kit.holders.pop()["hdl"].release()
        await settle(loop)
        assert kit.served() == ["d"]
        await kit.queue_all(["e"])
        assert kit.order() == ["e", "a", "b", "c"]
        assert await kit.serve_all() == ["e", "a", "b", "c"]
        kit.boxes["d"]["hdl"].release()
        await settle(loop)
        # drained: the next claims that queue are placed behind again
        assert kit.queue_stats()["queued"] == [0]
        assert kit.queue_stats()["lifo"] is False
        await kit.busy()
        await kit.queue_all(["f", "g"])
        assert kit.order() == ["f", "g"]
        await advance(loop, 0.1)              # exactly lifoAfter
        await kit.queue_all(["h"])
        assert kit.order() == ["h", "f", "g"]
        assert counters(kit)["queue-lifo"] == 3
        assert await kit.serve_all() == ["h", "f", "g"]
        await kit.stop()
    run_vt(body)


def test_stale_class_markers_after_timeout_and_cancel():
    """The pool remembers the last node of each class.  Waiters that
    leave behind its back (timeout, cancel) must not misplace the
    claims that follow."""
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 3}).up()
        await kit.busy()
        await kit.queue_all([("a", 0), ("b", 1), ("c", 1), ("d", 2)])
        kit.queue("t", 1, timeout=50)         # the last of class 1
        await settle(loop)
        assert kit.order() == ["a", "b", "c", "t", "d"]
        await advance(loop, 0.06)
        assert kit.log == [("t", "ClaimTimeoutError")]
        assert kit.order() == ["a", "b", "c", "d"]
        await kit.queue_all([("e", 1)])
        assert kit.order() == ["a", "b", "c", "e", "d"]
        # the last of class 0, and so the anchor of class 1 when class
        # 1 is empty: cancel class 1 entirely, then the marker of 0
        for label in "bce":
            kit.boxes[label]["waiter"].cancel()
        kit.boxes["a"]["waiter"].cancel()
        await settle(loop)
        assert kit.order() == ["d"]
        await kit.queue_all([("f", 1)])
        assert kit.order() == ["f", "d"]
        await kit.queue_all([("g", 0), ("h", 1), ("i", 2)])
        assert kit.order() == ["g", "f", "h", "d", "i"]
        # the tail of all goes, then its class gets a new claim
        kit.boxes["i"]["waiter"].cancel()
        kit.boxes["d"]["waiter"].cancel()
        await kit.queue_all([("j", 2), ("k", 0)])
        assert kit.order() == ["g", "k", "f", "h", "j"]
        assert kit.queue_stats()["queued"] == [2, 2, 1]
        # the feed takes heads away behind the pool's back too
        kit.holders.pop()["hdl"].release()
        await settle(loop)
        assert kit.served() == ["g"]
        kit.boxes["k"]["waiter"].cancel()
        await kit.queue_all([("l", 0), ("m", 1)])
        assert kit.order() == ["l", "f", "h", "m", "j"]
        assert await kit.serve_all() == ["l", "f", "h", "m", "j"]
        kit.boxes["g"]["hdl"].release()
        # cancelled claims never call back
        assert all(kit.boxes[k]["fired"] == 0 for k in "bceaidk")
        assert kit.queue_stats()["queued"] == [0, 0, 0]
        await kit.stop()
    run_vt(body)


def test_stale_markers_under_lifo_with_a_bound():
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 2, "order": "lifo",
                                    "maxQueued": 3}).up()
        await kit.busy()
        await kit.queue_all([("a", 1), ("b", 1), ("c", 0)])
        assert kit.order() == ["c", "b", "a"]
        # sheds a, the remembered last node of class 1
        await kit.queue_all([("d", 1)])
        assert kit.errors["a"].displaced is True
        assert kit.order() == ["c", "d", "b"]
        # sheds b, and class 1 is then d alone
        await kit.queue_all([("e", 0)])
        assert kit.order() == ["e", "c", "d"]
        kit.boxes["d"]["waiter"].cancel()
        await kit.queue_all([("f", 1), ("g", 1)])
        assert kit.order() == ["e", "c", "g"]
        assert kit.errors["f"].displaced is True
        assert await kit.serve_all() == ["e", "c", "g"]
        await kit.stop()
    run_vt(body)


def test_remembered_nodes_that_left_are_let_go():
    """A placement refreshes the markers of every class, not only of
    the classes it needs: the pool does not hold on to the node, and so
    the handle, of a waiter that has left."""
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 3, "maxQueued": 3}).up()
        await kit.busy()
        await kit.queue_all([("a", 2), ("b", 2), ("c", 1)])
        # sheds b, the remembered last node of class 2; the claim
        # itself needs to know about class 0 alone
        await kit.queue_all([("d", 0)])
        assert kit.errors["b"].displaced is True
        assert kit.order() == ["d", "c", "a"]
        last = kit.pool.p_cq_last
        assert [n is not None and n.linked for n in last] == [True] * 3
        assert [n.value.test_label for n in last] == ["d", "c", "a"]
        # likewise after a cancel in a class behind the new claim's
        kit.boxes["a"]["waiter"].cancel()
        await kit.queue_all([("e", 0)])
        last = kit.pool.p_cq_last
        assert last[2] is None
        assert [n.value.test_label for n in last[:2]] == ["e", "c"]
        assert await kit.serve_all() == ["d", "e", "c"]
        await kit.stop()
    run_vt(body)


def test_with_target_claim_delay():
    async def body(loop):
        kit = await QueueKit(loop, {"order": "adaptive", "priorities": 2},
                             targetClaimDelay=100).up()
        assert kit.pool.p_cq["lifoAfter"] == 100
        with pytest.raises(ValueError):
            kit.pool.claim({"timeout": 50}, lambda *a: None)
        with pytest.raises(ValueError):
            kit.pool.claim({"timeout": 50, "priority": 1}, lambda *a: None)
        await kit.busy()
        await kit.queue_all([("a", 1), ("b", 1)])
        await advance(loop, 0.15)
        await kit.queue_all([("c", 1), ("u", 0)])
        assert kit.order() == ["u", "c", "a", "b"]
        assert kit.queue_stats()["lifo"] is True
        # CoDel still judges whatever the feed dequeues, by the time
        # the claim was made: a and b have waited 6 and 7 target delays
        # by the time they reach the head, well inside the 10 that is
        # their claim timeout
        t0 = loop.time()
        await advance(loop, 0.3)
        for label in ("u", "c"):
            kit.holders.pop()["hdl"].release()
            await settle(loop)
        assert kit.served() == ["u", "c"]
        await advance(loop, 0.15)
        kit.boxes["u"]["hdl"].release()
        await settle(loop)
        await advance(loop, 0.1)
        kit.boxes["c"]["hdl"].release()
        await settle(loop)
        assert loop.time() - t0 < 0.6
        assert kit.log[2:] == [("a", "served"),
                               ("b", "ClaimTimeoutError")]
        assert isinstance(kit.errors["b"], ClaimTimeoutError)
        assert counters(kit)["claim-timeout"] == 1
        kit.boxes["a"]["hdl"].release()
        await settle(loop)
        assert all(b["fired"] == 1 for b in kit.boxes.values())
        assert kit.queue_stats()["queued"] == [0, 0]
        await kit.stop()
    run_vt(body)


@pytest.mark.parametrize("extra", [{}, {"lb": {"choices": "all"}}],
                         ids=["plain", "claimBalancing"])
def test_an_idle_connection_never_touches_the_queue(extra):
    async def body(loop):
        kit = await QueueKit(loop, {"maxQueued": 1, "priorities": 2,
                                    "order": "lifo"},
                             backends=("b1", "b2"), per=1, **extra).up()
        for _ in range(3):
            a = kit.claim({"avoidBackends": ["b1"], "priority": 1})
            await settle(loop)
            assert a["key"] == "b2"
            b = kit.claim({"avoidBackends": ["b1"]})
            await settle(loop)
            assert b["key"] == "b1"
            a["hdl"].release()
            b["hdl"].release()
            await settle(loop)
        got = counters(kit)
        assert not [c for c in got if c.startswith("queue-")]
        assert "queued-claim" not in got
        assert kit.queue_stats()["queued"] == [0, 0]
        if extra:
            assert got["balanced-claim"] == 6
        # and once nothing is idle the same claims queue by class
        await kit.busy()
        await kit.queue_all([("x", 1)])
        kit.queue("y", 0, avoidBackends=["b2"])
        await settle(loop)
        assert kit.errors["x"].displaced is True
        assert kit.order() == ["y"]
        assert await kit.serve_all() == ["y"]
        await kit.stop()
    run_vt(body)


def test_stop_drains_a_prioritised_queue():
    async def body(loop):
        kit = await QueueKit(loop, {"priorities": 2, "order": "lifo"}).up()
        await kit.busy()
        await kit.queue_all([("a", 1), ("b", 0), ("c", 1)])
        assert kit.order() == ["b", "c", "a"]
        kit.pool.stop()
        await settle(loop)
        assert kit.log == [("b", "PoolStoppingError"),
                           ("c", "PoolStoppingError"),
                           ("a", "PoolStoppingError")]
        assert isinstance(kit.errors["a"], PoolStoppingError)
        assert kit.queue_stats()["queued"] == [0, 0]
        late = {}
        kit.pool.claim({"priority": 1}, lambda err, *a: late.update(err=err))
        await settle(loop)
        assert isinstance(late["err"], PoolStoppingError)
        for box in kit.holders:
            box["hdl"].release()
        await advance(loop, 30.0)
        assert kit.pool.is_in_state("stopped")
    run_vt(body)


def test_failed_state_drains_a_prioritised_queue():
    async def body(loop):
        # no connection ever connects: the claims wait, and the connect
        # timeouts run out
        kit = QueueKit(loop, {"priorities": 2, "maxQueued": 8})
        kit.resolver_fsm.start()
        kit.resolver.add("b1", {"address": "10.0.0.1", "port": 80})
        await settle(loop)
        await kit.queue_all([("a", 1), ("b", 0), ("c", 1)])
        assert kit.order() == ["b", "a", "c"]
        await advance(loop, 30.0)
        assert kit.pool.is_in_state("failed")
        assert kit.log == [("b", "PoolFailedError"),
                           ("a", "PoolFailedError"),
                           ("c", "PoolFailedError")]
        assert isinstance(kit.errors["b"], PoolFailedError)
        assert kit.queue_stats()["queued"] == [0, 0]
        late = {}
        kit.pool.claim({"priority": 0}, lambda err, *a: late.update(err=err))
        await settle(loop)
        assert isinstance(late["err"], PoolFailedError)
        kit.pool.stop()
        await advance(loop, 30.0)
        assert kit.pool.is_in_state("stopped")
    run_vt(body)


def test_error_on_empty_is_not_queued():
    async def body(loop):
        kit = QueueKit(loop, {"maxQueued": 2})
        kit.resolver_fsm.start()
        await settle(loop)
        kit.queue("a", errorOnEmpty=True)
        await settle(loop)
        assert kit.log == [("a", "NoBackendsError")]
        assert kit.queue_stats()["queued"] == [0]
        assert "queued-claim" not in counters(kit)
        # the documented difference: a pool without the option links
        # the failed handle, as the reference does, and counts it
        plain = QueueKit(loop)
        plain.resolver_fsm.start()
        await settle(loop)
        plain.queue("a", errorOnEmpty=True)
        await settle(loop)
        assert plain.log == [("a", "NoBackendsError")]
        assert counters(plain)["queued-claim"] == 1
        assert plain.pool.get_stats()["waiterCount"] == 1
        kit.pool.stop()
        plain.pool.stop()
        await advance(loop, 30.0)
        assert kit.pool.is_in_state("stopped")
        assert plain.pool.is_in_state("stopped")
    run_vt(body)
