"""``maxConnectionAge`` and ``recycle()`` on a set: a due connection is
replaced make-before-break on the same backend.  The successor ``k.N+1``
is 'added' first; only then is ``k.N`` 'removed'.  With
``connectionAgeSpread: 0`` the virtual clock makes every time exact."""

import random

from cueball_amd.testing import advance, settle
from conftest import run_vt
from cset_age_kit import AGE, Kit, instance_vars


async def one_backend_up(kit):
    """One backend, connected and advertised at t0; returns t0."""
    await settle(kit.loop)
    assert len(kit.conns) == 1
    t0 = kit.loop.time()
    kit.conns[0].connect()
    await settle(kit.loop)
    assert kit.log == ["added b1.1"]
    return t0


async def two_backends_up(kit, first, other, gap=40.0):
    """`first` is up at t0; `other` joins the resolver and connects
    `gap` seconds later, so its deadline is that much further away.
    Returns t0."""
    await settle(kit.loop)
    assert [c.key for c in kit.conns] == [first]
    t0 = kit.loop.time()
    await kit.connect_new()
    await advance(kit.loop, gap)
    kit.resolver.add(other, {})
    await settle(kit.loop)
    await kit.connect_new()
    assert kit.log == ["added %s.1" % first, "added %s.1" % other]
    return t0


def test_successor_is_added_before_predecessor_is_removed():
    async def body(loop):
        kit = Kit(loop, hold=True, maxConnectionAge=AGE)
        cset = kit.cset
        t0 = await one_backend_up(kit)
        c1 = kit.conns[0]

        await kit.to(t0 + 59.9)
        kit.sample()
        assert len(kit.conns) == 1
        await kit.to(t0 + 60)
        kit.sample()
        # a second connection object, and nothing emitted yet
        assert len(kit.conns) == 2
        c2 = kit.conns[1]
        assert c2.key == "b1" and not c2.connected
        assert kit.log == ["added b1.1"]
        assert kit.recycled == []
        assert cset.get_stats()["totalConnections"] == 2

        c2.connect()
        await settle(loop)
        kit.sample()
        assert kit.log == ["added b1.1", "added b1.2", "removed b1.1"]
        assert kit.recycled == [("b1", "age")]
        assert kit.counter("recycled-age") == 1
        assert cset.get_connections() == [c2]
        assert cset.cs_fsm["b1"].csf_smgr.sm_socket is c2

        # b1.1 is the consumer's until it lets go
        await advance(loop, 5.0)
        assert not c1.dead and c1.connected
        ckey, conn, hdl = kit.held.pop()
        assert (ckey, conn) == ("b1.1", c1)
        hdl.release()
        await settle(loop)
        assert c1.dead
        assert not c2.dead
        assert len(cset.cs_lconns) == 1
        assert cset.get_stats()["totalConnections"] == 1
        kit.sample()
        assert kit.low == 1       # never without a connection
        kit.hold = False
        await kit.stop()
        assert kit.log[3:] == ["removed b1.2"]
    run_vt(body)


def test_spread_draws_a_lifetime_per_socket():
    async def body(loop):
        random.seed(7)
        kit = Kit(loop, backends=("b1", "b2"), target=2, maximum=2,
                  maxConnectionAge=AGE, connectionAgeSpread=0.5)
        await settle(loop)
        await kit.connect_new()
        ages = kit.ages()
        assert len(ages) == 2
        expires = [a["expiresInMs"] for a in ages]
        assert all(30_000 <= e <= 60_000 for e in expires)
        assert expires[0] != expires[1]
        await kit.stop()
    run_vt(body)


def test_replacements_are_paced_one_at_a_time():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"), target=2, maximum=2,
                  maxConnectionAge=AGE)
        await settle(loop)
        t0 = loop.time()
        await kit.connect_new()
        assert len(kit.log) == 2

        await kit.to(t0 + 61)
        # both due, one extra connection object
        assert len(kit.conns) == 3
        assert kit.recycled == []
        first = kit.conns[2].key
        second = "b2" if first == "b1" else "b1"
        await kit.connect_new()
        # the first swap has run, and the second replacement followed
        assert kit.recycled == [(first, "age")]
        assert len(kit.conns) == 4 and kit.conns[3].key == second
        assert kit.log[2:] == ["added %s.2" % first, "removed %s.1" % first]
        await kit.connect_new()
        assert kit.log[4:] == ["added %s.2" % second,
                               "removed %s.1" % second]
        assert kit.counter("recycled-age") == 2
        assert kit.recycled == [(first, "age"), (second, "age")]
        assert len(kit.conns) == 4
        assert [c.dead for c in kit.conns] == [True, True, False, False]
        assert kit.low == 1       # at the very first 'added'
        assert len(kit.cset.cs_lconns) == 2
        await kit.stop()
    run_vt(body)


def test_a_consumer_that_holds_removed_does_not_block_the_next():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"), hold=True, target=2,
                  maximum=2, maxConnectionAge=AGE)
        await settle(loop)
        t0 = loop.time()
        await kit.connect_new()
        await kit.to(t0 + 60)
        assert len(kit.conns) == 3
        await kit.connect_new()
        assert len(kit.held) == 1         # removed, and kept
        assert len(kit.conns) == 4        # the next one started anyway
        await kit.connect_new()
        assert len(kit.held) == 2
        assert kit.counter("recycled-age") == 2
        await advance(loop, 20.0)
        for ckey, conn, hdl in kit.held:
            assert not conn.dead and conn.connected
        assert kit.cset.get_stats()["totalConnections"] == 2
        assert sum(1 for a in kit.ages() if a["recycling"]) == 2
        for ckey, conn, hdl in kit.held:
            hdl.release()
        await settle(loop)
        assert [c.dead for c in kit.conns] == [True, True, False, False]
        assert sum(1 for a in kit.ages() if a["recycling"]) == 0
        kit.hold = False
        await kit.stop()
    run_vt(body)


def test_a_replacement_that_cannot_connect_leaves_the_old_one_alone():
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        cset = kit.cset
        t0 = await one_backend_up(kit)
        await kit.to(t0 + 60)
        assert len(kit.conns) == 2
        for attempt in range(3):
            assert kit.failed == []
            c = kit.pending()
            assert len(c) == 1
            c[0].emit("error", RuntimeError("refused"))
            await advance(loop, 0)    # the retry delay is 0
        assert len(kit.conns) == 4
        assert [c.dead for c in kit.conns] == [False, True, True, True]
        assert kit.log == ["added b1.1"]
        assert cset.get_connections() == [kit.conns[0]]
        assert kit.counter("recycle-failed") == 1
        assert kit.failed == [("b1", "age")]
        assert kit.recycled == []
        assert "b1" not in cset.cs_dead
        assert cset.is_in_state("running")
        assert len(cset.cs_lconns) == 1
        assert cset.get_stats()["totalConnections"] == 1
        # no time has passed since t0 + 60: one fresh lifetime from now
        ages = kit.ages()
        assert len(ages) == 1 and not ages[0]["recycling"]
        assert ages[0]["expiresInMs"] == AGE

        # and the next attempt comes when that one runs out
        await kit.to(t0 + 119.9)
        assert len(kit.conns) == 4
        await kit.to(t0 + 120)
        assert len(kit.conns) == 5
        await kit.connect_new()
        # serial 2 went to the attempt that failed: keys are never reused
        assert kit.log == ["added b1.1", "added b1.3", "removed b1.1"]
        await kit.stop()
    run_vt(body)


def _old_goes_away(how):
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        cset = kit.cset
        t0 = await one_backend_up(kit)
        await kit.to(t0 + 60)
        assert len(kit.conns) == 2
        c1, c2 = kit.conns
        if how == "error":
            c1.once("error", lambda e: None)
            c1.emit("error", RuntimeError("reset"))
        else:
            kit.advertised.pop("b1.1")[1].close()
        await settle(loop)
        # the existing path: 'removed' for a dead socket, none for a
        # handle the consumer closed
        expect = ["added b1.1"] + (["removed b1.1"] if how == "error"
                                   else [])
        assert kit.log == expect
        assert c1.dead
        # the replacement has taken over as the backend's slot
        assert cset.cs_fsm["b1"].csf_smgr.sm_socket is c2
        assert kit.recycled == [("b1", "age")]

        c2.connect()
        await settle(loop)
        assert kit.log == expect + ["added b1.2"]
        await advance(loop, 30.0)
        assert kit.log == expect + ["added b1.2"]
        assert kit.of("b1") == [c2]
        assert len(cset.cs_lconns) == 1
        assert list(cset.cs_lconns) == ["b1.2"]
        assert cset.get_stats()["totalConnections"] == 1
        assert len(kit.ages()) == 1
        assert kit.counter("recycled-age") == 1
        assert kit.counter("recycle-failed") == 0
        assert kit.failed == []
        assert "b1" not in cset.cs_dead
        await kit.stop()
        assert all(c.dead for c in kit.conns)
    return body


def test_old_connection_errors_under_its_replacement():
    run_vt(_old_goes_away("error"))


def test_consumer_closes_old_handle_under_its_replacement():
    run_vt(_old_goes_away("close"))


def test_backend_leaves_the_resolver_mid_replacement():
    async def body(loop):
        kit = Kit(loop, backends=("b1",), target=2, maximum=2,
                  maxConnectionAge=AGE)
        cset = kit.cset
        t0 = await two_backends_up(kit, "b1", "b2")
        await kit.to(t0 + 60)
        assert len(kit.conns) == 3 and kit.conns[2].key == "b1"

        kit.resolver.remove("b1")
        await advance(loop, 30.0)
        assert len(kit.of("b1", live=False)) >= 2
        assert kit.of("b1") == []
        assert "removed b1.1" in kit.log
        assert not any(e.startswith("added b1.") and e != "added b1.1"
                       for e in kit.log)
        assert kit.recycled == [] and kit.failed == []
        assert cset.is_in_state("running")
        assert "b1" not in cset.cs_fsm
        assert all(a["backend"] == "b2" for a in kit.ages())
        assert not any(ck.startswith("b1.") for ck in cset.cs_lconns)
        await kit.stop()
    run_vt(body)


def test_stop_mid_replacement():
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        t0 = await one_backend_up(kit)
        await kit.to(t0 + 60)
        assert len(kit.conns) == 2
        await kit.stop()
        assert all(c.dead for c in kit.conns)
        assert kit.log == ["added b1.1", "removed b1.1"]
        assert kit.advertised == {}
        assert kit.cset.cs_lconns == {}
        assert kit.cset.recycle() == 0
    run_vt(body)


def test_stop_between_added_and_swap():
    """stop() from the 'added' handler of the successor: both
    connections are advertised at that moment and both get their
    'removed'."""
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        t0 = await one_backend_up(kit)
        await kit.to(t0 + 60)
        kit.cset.on("added", lambda ckey, conn, hdl: kit.cset.stop())
        await kit.connect_new()
        await advance(loop, 30.0)
        assert kit.cset.is_in_state("stopped")
        assert all(c.dead for c in kit.conns)
        assert sorted(kit.log) == ["added b1.1", "added b1.2",
                                   "removed b1.1", "removed b1.2"]
        assert kit.advertised == {}
    run_vt(body)


def test_recycle_replaces_everything_advertised_now():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"), target=2, maximum=2)
        cset = kit.cset
        await settle(loop)
        await kit.connect_new()
        assert not any(n.startswith("cs_age") for n in instance_vars(cset))
        assert cset.recycle() == 2
        assert cset.recycle() == 0
        await settle(loop)
        assert len(kit.conns) == 3
        first = kit.conns[2].key
        second = "b2" if first == "b1" else "b1"
        await kit.connect_new()
        assert len(kit.conns) == 4 and kit.conns[3].key == second
        assert cset.recycle() == 1        # the successor, nothing else
        await kit.connect_new()
        assert kit.recycled[:2] == [(first, "manual"), (second, "manual")]
        await kit.connect_new()
        assert kit.recycled == [(first, "manual"), (second, "manual"),
                                (first, "manual")]
        assert kit.counter("recycled-manual") == 3
        assert kit.log[2:] == [
            "added %s.2" % first, "removed %s.1" % first,
            "added %s.2" % second, "removed %s.1" % second,
            "added %s.3" % first, "removed %s.2" % first]
        # connections opened afterwards carry no deadline
        ages = kit.ages()
        assert len(ages) == 2
        assert [a["expiresInMs"] for a in ages] == [None, None]
        assert cset.get_connection_ages()["maxAgeMs"] is None
        await advance(loop, 300.0)
        assert len(kit.conns) == 5
        await kit.stop()
        assert cset.recycle() == 0
    run_vt(body)


def test_connection_ages_during_a_replacement():
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        t0 = await one_backend_up(kit)
        await kit.to(t0 + 30)
        report = kit.cset.get_connection_ages()
        assert report["maxAgeMs"] == AGE and report["oldestMs"] == 30_000
        assert report["connections"] == [
            {"backend": "b1", "ckey": "b1.1", "state": "busy",
             "ageMs": 30_000, "expiresInMs": 30_000, "recycling": False}]
        await kit.to(t0 + 60)
        old, new = kit.ages()
        assert old == {"backend": "b1", "ckey": "b1.1", "state": "busy",
                       "ageMs": 60_000, "expiresInMs": None,
                       "recycling": True}
        assert new == {"backend": "b1", "ckey": None,
                       "state": "connecting", "ageMs": None,
                       "expiresInMs": None, "recycling": False}
        await kit.connect_new()
        ages = kit.ages()
        assert [a["ckey"] for a in ages] == ["b1.2"]
        assert ages[0]["expiresInMs"] == AGE
        await kit.stop()
    run_vt(body)


def test_target_shrink_drops_a_backend_mid_replacement():
    async def body(loop):
        kit = Kit(loop, backends=("b2",), target=2, maximum=2,
                  maxConnectionAge=AGE)
        cset = kit.cset
        t0 = await two_backends_up(kit, "b2", "b1")
        cset.cs_keys.sort()       # b1 is the one a target of 1 keeps
        await kit.to(t0 + 60)
        assert len(kit.conns) == 3 and kit.conns[2].key == "b2"
        b1conn = kit.of("b1")[0]

        cset.set_target(1)
        await advance(loop, 30.0)
        assert kit.of("b2") == []
        assert len(kit.of("b2", live=False)) >= 2
        assert kit.log[2:] == ["removed b2.1"]
        assert kit.recycled == [] and kit.failed == []
        assert list(cset.cs_fsm) == ["b1"]
        assert list(cset.cs_lconns) == ["b1.1"]
        assert kit.of("b1") == [b1conn] and b1conn.connected
        assert cset.get_connections() == [b1conn]
        assert cset.get_stats()["totalConnections"] == 1
        await kit.stop()
    run_vt(body)
