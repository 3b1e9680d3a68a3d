"""``outlierDetection`` on a pool: leases that fail in a row eject their
backend for a while; the pool keeps no connection to it, hands no claim
to it, and tries it again when the ejection is over."""

import random

import pytest

from cueball_amd.errors import CueballError
from cueball_amd.pool_monitor import monitor
from cueball_amd.testing import advance, settle
from conftest import run_vt
from outlier_kit import BASE, OD, Kit, instance_vars


def test_failures_in_a_row_eject_the_backend():
    async def body(loop):
        kit = Kit(loop, od=dict(OD, consecutiveFailures=3,
                                baseEjectionTime=600_000,
                                maxEjectionTime=600_000))
        pool = kit.pool
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == [] and kit.streak("b1") == 2
        assert kit.events == []
        t0 = loop.time()
        await kit.fail_on("b1")
        assert kit.ejected() == ["b1"]
        assert kit.events == [("ejected", "b1", {
            "reason": "consecutive-failures", "durationMs": 600_000,
            "ejections": 1}, kit.events[0][3])]
        assert t0 <= kit.events[0][3] <= loop.time()
        # all its slots stopped, and the other two carry the pool
        assert kit.slots("b1") == [] and kit.live("b1") == []
        # (right now the count is what the pool's anti-shrink filter
        # remembers of the leases above; the exact figures follow)
        st = pool.get_stats()
        assert 2 <= st["totalConnections"] <= 4
        assert st["idleConnections"] == st["totalConnections"]
        assert len(kit.slots("b2")) + len(kit.slots("b3")) == \
            st["totalConnections"]
        # no later claim is served by it, however many are open at
        # once: the maximum of four sits on the other two, evenly
        del kit.served[:]
        boxes = [await kit.claim() for _ in range(4)]
        assert all("hdl" in b for b in boxes)
        assert sorted(kit.served) == ["b2", "b2", "b3", "b3"]
        assert pool.get_stats()["totalConnections"] == 4
        assert (len(kit.slots("b1")), len(kit.slots("b2")),
                len(kit.slots("b3"))) == (0, 2, 2)
        for b in boxes:
            await kit.end(b, "release")
        # once the filter has forgotten the load, the pool is back at
        # its spares: exactly one connection on each of the other two
        await advance(loop, 60.0)
        assert kit.ejected() == ["b1"]
        st = pool.get_stats()
        assert st["totalConnections"] == 2 and st["idleConnections"] == 2
        assert (len(kit.slots("b1")), len(kit.slots("b2")),
                len(kit.slots("b3"))) == (0, 1, 1)
        assert kit.live("b1") == []
        assert len(kit.live("b2")) == 1 and len(kit.live("b3")) == 1
        await kit.stop()
    run_vt(body)


def test_a_success_resets_the_streak():
    async def body(loop):
        kit = Kit(loop)
        await settle(loop)
        await kit.fail_on("b1")
        assert kit.streak("b1") == 1
        await kit.end(await kit.lease_on("b1"), "release")
        assert kit.streak("b1") == 0
        await kit.fail_on("b1")
        assert kit.streak("b1") == 1 and kit.ejected() == []
        assert kit.stats("b1")["failures"] == 2
        assert kit.stats("b1")["successes"] == 1
        await kit.fail_on("b1")
        assert kit.ejected() == ["b1"]
        await kit.stop()
    run_vt(body)


def test_streaks_are_per_backend():
    async def body(loop):
        kit = Kit(loop)
        await settle(loop)
        # four leases at once cover all three backends
        boxes = [await kit.claim() for _ in range(4)]
        assert sorted(set(b["key"] for b in boxes)) == ["b1", "b2", "b3"]
        first = {}
        for b in boxes:
            first.setdefault(b["key"], b)
        await kit.end(first["b1"], "close")
        await kit.end(first["b2"], "close")
        # two failures in a row, but not on one backend
        assert kit.streak("b1") == 1 and kit.streak("b2") == 1
        assert kit.ejected() == [] and kit.events == []
        rest = [b for b in boxes
                if b is not first["b1"] and b is not first["b2"]]
        for b in rest:
            if b["key"] != "b1":
                await kit.end(b, "release")
        # b1's second failure, on its other lease if it has one
        more = [b for b in rest if b["key"] == "b1"]
        if more:
            await kit.end(more[0], "close")
        else:
            await kit.fail_on("b1")
        assert kit.ejected() == ["b1"]
        assert kit.stats("b2")["failures"] == 1
        await kit.stop()
    run_vt(body)


# how a lease ends, the option that decides, and whether it is a
# failure with that option on / off (None: the option does not matter)
SIGNALS = [
    ("error", None, True, True),
    ("sockclose", "countSocketClose", True, False),
    ("close", "countClose", True, False),
    ("report", None, True, True),
]


@pytest.mark.parametrize("how,option,when_on,when_off", SIGNALS)
@pytest.mark.parametrize("setting", [True, False])
def test_each_failure_signal(how, option, when_on, when_off, setting):
    async def body(loop):
        od = dict(OD)
        if option is not None:
            od[option] = setting
        kit = Kit(loop, od=od)
        await settle(loop)
        await kit.fail_on("b1", how=how)
        failed = when_on if setting else when_off
        rec = kit.stats("b1")
        assert rec["failures"] == (1 if failed else 0)
        assert rec["consecutiveFailures"] == (1 if failed else 0)
        # neutral, not a success
        assert rec["successes"] == 0
        await kit.fail_on("b1", how=how)
        assert kit.ejected() == (["b1"] if failed else [])
        await kit.stop()
    run_vt(body)


def test_both_options_off_leave_close_after_socket_close_neutral():
    async def body(loop):
        kit = Kit(loop, od=dict(OD, countClose=False,
                                countSocketClose=False))
        await settle(loop)
        for _ in range(3):
            box = await kit.lease_on("b1")
            box["conn"].emit("close")
            await settle(loop)
            await kit.end(box, "close")
        assert kit.stats("b1")["failures"] == 0
        # but an error is an error, however the lease is ended
        for _ in range(2):
            box = await kit.lease_on("b1")
            box["conn"].emit("error", Exception("boom"))
            await settle(loop)
            await kit.end(box, "close")
        assert kit.ejected() == ["b1"]
        await kit.stop()
    run_vt(body)


def test_an_error_counts_when_the_release_is_heard_first():
    """A socket that emits 'close' from its destroy(), as a TCP
    connection does, and a claimer that releases on 'close': the
    release happens inside the socket manager's own transition to
    'error', so the slot hears of the release first and goes idle as if
    the socket were fine."""
    async def body(loop):
        kit = Kit(loop)
        await settle(loop)
        for n in (1, 2):
            box = await kit.lease_on("b1")
            conn, hdl = box["conn"], box["hdl"]
            destroy = conn.destroy

            def destroy_and_close(conn=conn, destroy=destroy):
                destroy()
                conn.emit("close")

            conn.destroy = destroy_and_close
            conn.remove_listener("error", box["on_error"])
            onerr = conn.on("error", lambda e: None)

            hdl.disable_release_leak_check()
            conn.once("close", hdl.release)
            conn.emit("error", Exception("reset"))
            conn.remove_listener("error", onerr)
            assert hdl.is_in_state("released")
            await settle(loop)
            await advance(loop, 0.01)
            rec = kit.stats("b1")
            assert (rec["failures"], rec["successes"]) == (n, 0)
        assert kit.ejected() == ["b1"]
        await kit.stop()
    run_vt(body)


def test_report_failure_is_valid_only_while_claimed():
    async def body(loop):
        kit = Kit(loop)
        await settle(loop)
        box = await kit.lease_on("b1")
        hdl = box["hdl"]
        hdl.report_failure(Exception("503"))
        hdl.report_failure()
        await kit.end(box, "release")
        assert kit.stats("b1")["failures"] == 1
        with pytest.raises(CueballError):
            hdl.report_failure()
        with pytest.raises(CueballError):
            hdl.release()
        assert kit.stats("b1")["failures"] == 1
        # a handle that is still waiting
        waiting = []
        boxes = [await kit.claim() for _ in range(4)]
        late = kit.pool.claim({"timeout": 10_000},
                              lambda *a: waiting.append(a))
        await settle(loop)
        assert late.is_in_state("waiting")
        with pytest.raises(CueballError):
            late.report_failure()
        late.cancel()
        for b in boxes:
            await kit.end(b, "release")
        assert waiting == []
        await kit.stop()
    run_vt(body)


def ping_kit(loop, **od):
    kit = Kit(loop, backends=("b1", "b2"), od=dict(OD, **od),
              checker=lambda hdl, conn: kit.pings.append((hdl, conn)),
              checkTimeout=500)
    return kit


async def next_ping(kit, key):
    """Let the idle slots' health checks fire; release all but the
    first one on `key`, which is returned."""
    del kit.pings[:]
    await advance(kit.loop, 0.5)
    mine = None
    for hdl, conn in kit.pings:
        if conn.key == key and mine is None:
            mine = hdl
        else:
            hdl.release()
    assert mine is not None
    return mine


def test_a_ping_that_closes_is_a_failure():
    async def body(loop):
        # not even countClose matters for a health check
        kit = ping_kit(loop, countClose=False)
        await settle(loop)
        for n in (1, 2):
            hdl = await next_ping(kit, "b1")
            assert hdl.ch_pinger
            hdl.close()
            await settle(loop)
            await advance(loop, 0.01)
            assert kit.stats("b1")["failures"] == n
        assert kit.ejected() == ["b1"]
        assert kit.stats("b2")["failures"] == 0
        await kit.stop()
    run_vt(body)


def test_a_ping_that_releases_is_neutral():
    async def body(loop):
        kit = ping_kit(loop)
        await settle(loop)
        await kit.fail_on("b1")
        assert kit.streak("b1") == 1
        before = kit.stats("b1")
        for _ in range(3):
            hdl = await next_ping(kit, "b1")
            hdl.release()
            await settle(loop)
        # /health answers: that neither counts nor resets anything
        after = kit.stats("b1")
        assert after["consecutiveFailures"] == 1
        assert after["successes"] == before["successes"]
        assert after["failures"] == 1
        await kit.fail_on("b1")
        assert kit.ejected() == ["b1"]
        await kit.stop()
    run_vt(body)


def test_a_busy_slot_serves_its_lease_to_the_end():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"))
        await settle(loop)
        held = await kit.lease_on("b1")
        await kit.fail_on("b1", 2)
        assert kit.ejected() == ["b1"]
        # the lease is untouched by the ejection
        assert held["hdl"].is_in_state("claimed")
        assert kit.live("b1") == [held["conn"]]
        assert [s.get_state() for s in kit.slots("b1")] == ["busy"]
        assert held["conn"].seen_unwanted
        await kit.end(held, "release")
        assert kit.live("b1") == [] and kit.slots("b1") == []
        await kit.stop()
    run_vt(body)


def test_durations_double_up_to_the_cap():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"))
        await settle(loop)
        seen = []
        for want in (1000, 2000, 4000, 5000):
            await kit.fail_on("b1", 2)
            ev = kit.events[-1]
            assert ev[0] == "ejected" and ev[2]["durationMs"] == want
            seen.append(ev[2]["ejections"])
            t = ev[3]
            st = kit.stats("b1")
            assert st["ejectedForMs"] == pytest.approx(
                (loop.time() - t) * 1000.0)
            assert st["ejectedForMs"] + st["reinstatesInMs"] == \
                pytest.approx(want)
            await kit.to(t + want / 1000.0 - 0.001)
            assert kit.ejected() == ["b1"]
            await kit.to(t + want / 1000.0)
            # no jitter: to the tick
            assert kit.events[-1] == ("reinstated", "b1", "expired",
                                      t + want / 1000.0)
            assert kit.ejected() == [] and kit.streak("b1") == 0
            assert kit.stats("b1")["ejectedForMs"] is None
            assert kit.stats("b1")["reinstatesInMs"] is None
        assert seen == [1, 2, 3, 4]

        # just short of a clean period as long as the last ejection:
        # the count stands
        back = kit.events[-1][3]
        await kit.to(back + 4.9)
        assert kit.stats("b1")["ejections"] == 4
        await kit.fail_on("b1", 2)
        ev = kit.events[-1]
        assert ev[2] == {"reason": "consecutive-failures",
                         "durationMs": 5000, "ejections": 5}
        assert ev[3] < back + 5.0
        await kit.to(ev[3] + 5.0)
        back = kit.events[-1][3]
        assert kit.events[-1][:3] == ("reinstated", "b1", "expired")
        # a full clean period: forgotten
        await kit.to(back + 5.0)
        assert kit.stats("b1")["ejections"] == 0
        await kit.fail_on("b1", 2)
        assert kit.events[-1][2] == {"reason": "consecutive-failures",
                                     "durationMs": 1000, "ejections": 1}
        await kit.stop()
    run_vt(body)


def test_a_single_backend_is_never_ejected():
    async def body(loop):
        kit = Kit(loop, backends=("b1",))
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == [] and kit.counter("ejection-refused") == 1
        await kit.fail_on("b1", 2)
        # each refusal counts, and so does the streak
        assert kit.counter("ejection-refused") == 3
        assert kit.streak("b1") == 4
        assert kit.events == [] and kit.counter("backend-ejected") == 0
        assert kit.pool.is_in_state("running")
        await kit.stop()
    run_vt(body)


def test_the_last_usable_backend_is_refused():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"),
                  od=dict(OD, baseEjectionTime=60_000,
                          maxEjectionTime=60_000, maxEjectionPercent=100))
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == ["b1"]
        await kit.fail_on("b2", 3)
        assert kit.ejected() == ["b1"]
        assert kit.counter("ejection-refused") == 2
        assert kit.streak("b2") == 3
        await kit.stop()
    run_vt(body)


def test_max_ejection_percent_limits_the_share():
    async def body(loop):
        kit = Kit(loop, od=dict(OD, baseEjectionTime=60_000,
                                maxEjectionTime=60_000,
                                maxEjectionPercent=34))
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == ["b1"]
        # b3 is fine, but two of three is more than 34 %
        await kit.fail_on("b2", 2)
        assert kit.ejected() == ["b1"]
        assert kit.counter("ejection-refused") == 1
        await kit.fail_on("b2")
        assert kit.counter("ejection-refused") == 2
        assert kit.streak("b2") == 3
        assert kit.counter("backend-ejected") == 1
        await kit.stop()
    run_vt(body)


def test_panic_lifts_ejections_when_the_rest_is_dead():
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"),
                  od=dict(OD, baseEjectionTime=600_000,
                          maxEjectionTime=600_000),
                  recovery={"default": {"timeout": 2000, "retries": 3,
                                        "delay": 100}})
        pool = kit.pool
        await settle(loop)
        states = []
        pool.on("stateChanged", states.append)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == ["b1"]
        # b2 stops accepting connections
        kit.down.add("b2")
        for c in kit.live("b2"):
            c.emit("error", Exception("reset"))
        await advance(loop, 1.0)
        assert pool.is_declared_dead("b2")
        assert kit.events[-1][:3] == ("reinstated", "b1", "panic")
        assert kit.ejected() == [] and kit.od_timers() == []
        # a suspect backend is better than none
        assert pool.is_in_state("running") and "failed" not in states
        assert len(kit.live("b1")) >= 1
        box = await kit.claim()
        assert box["key"] == "b1"
        await kit.end(box, "release")
        await kit.stop()
    run_vt(body)


def test_a_removed_backend_comes_back_clean():
    async def body(loop):
        kit = Kit(loop)
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == ["b1"] and len(kit.od_timers()) == 1
        kit.resolver.remove("b1")
        await settle(loop)
        # dropped without an event, timer and all
        assert len(kit.events) == 1 and kit.od_timers() == []
        assert "b1" not in kit.stats()["backends"]
        assert kit.stats()["ejected"] == 0
        kit.resolver.add("b1", {"address": "10.0.0.1", "port": 80})
        await settle(loop)
        assert kit.stats("b1") == {
            "consecutiveFailures": 0, "failures": 0, "successes": 0,
            "ejected": False, "ejections": 0, "ejectedForMs": None,
            "reinstatesInMs": None}
        # it is a full member again at once, and nothing fires later
        box = await kit.lease_on("b1")
        await kit.end(box, "release")
        await advance(loop, 2.0)
        assert len(kit.events) == 1
        assert kit.counter("backend-reinstated") == 0
        await kit.stop()
    run_vt(body)


def test_stop_during_an_ejection():
    async def body(loop):
        kit = Kit(loop, od=dict(OD, baseEjectionTime=600_000,
                                maxEjectionTime=600_000))
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert len(kit.od_timers()) == 1
        await kit.stop()
        assert kit.od_timers() == []
        assert [e[0] for e in kit.events] == ["ejected"]
        assert kit.pool.eject_backend("b2", 1000) is False
    run_vt(body)


def test_leases_that_fail_after_stop_eject_nothing():
    """Leases are held through 'stopping.backends'; a backend whose
    leases fail while the pool drains is not ejected, and no timer
    outlives the pool."""
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"))
        pool = kit.pool
        await settle(loop)
        boxes = [await kit.claim() for _ in range(4)]
        assert sorted(b["key"] for b in boxes) == ["b1", "b1", "b2", "b2"]
        pool.stop()
        await settle(loop)
        assert not pool.is_in_state("stopped")
        for b in boxes:
            if b["key"] == "b1":
                await kit.end(b, "close")
        # judged, but to no effect
        assert kit.stats()["ejected"] == 0
        assert kit.events == [] and kit.od_timers() == []
        assert kit.counter("backend-ejected") == 0
        assert kit.counter("ejection-refused") == 0
        for b in boxes:
            if b["key"] == "b2":
                await kit.end(b, "release")
        await advance(loop, 30.0)
        assert pool.is_in_state("stopped")
        assert kit.od_timers() == []
        await advance(loop, 600.0)
        assert kit.events == []
        assert kit.counter("backend-reinstated") == 0
    run_vt(body)


def test_removing_the_last_backend_in_service_lifts_ejections():
    """b1 is ejected and the resolver then drops b2: b1 is all there is,
    and a suspect backend is better than none."""
    async def body(loop):
        kit = Kit(loop, backends=("b1", "b2"),
                  od=dict(OD, baseEjectionTime=60_000,
                          maxEjectionTime=60_000))
        pool = kit.pool
        await settle(loop)
        await kit.fail_on("b1", 2)
        assert kit.ejected() == ["b1"] and kit.live("b1") == []
        t = loop.time()
        kit.resolver.remove("b2")
        await settle(loop)
        assert kit.events[-1] == ("reinstated", "b1", "panic", t)
        assert kit.ejected() == [] and kit.od_timers() == []
        await advance(loop, 0.01)
        assert pool.is_in_state("running")
        assert kit.live("b2") == [] and len(kit.live("b1")) == 2
        box = await kit.claim()
        assert box["key"] == "b1"
        await kit.end(box, "release")
        # with another backend still in service nothing is lifted
        kit.resolver.add("b2", {"address": "10.0.0.1", "port": 80})
        kit.resolver.add("b3", {"address": "10.0.0.1", "port": 80})
        await settle(loop)
        assert pool.eject_backend("b1", 60_000) is True
        n = len(kit.events)
        kit.resolver.remove("b2")
        await settle(loop)
        assert kit.ejected() == ["b1"] and len(kit.events) == n
        await kit.stop()
    run_vt(body)


def test_manual_ejection_without_the_option():
    async def body(loop):
        kit = Kit(loop, od=None)
        pool = kit.pool
        await settle(loop)
        before = set(instance_vars(pool))
        assert pool.reinstate_backend("b1") is False
        assert set(instance_vars(pool)) == before
        with pytest.raises(ValueError):
            pool.eject_backend("b1")
        assert pool.eject_backend("nope", 5000) is False
        t0 = loop.time()
        assert pool.eject_backend("b1", 5000) is True
        assert pool.eject_backend("b1", 5000) is False
        await settle(loop)
        assert kit.events == [("ejected", "b1", {
            "reason": "manual", "durationMs": 5000, "ejections": 1}, t0)]
        st = kit.stats()
        assert st["enabled"] is False and st["ejected"] == 1
        assert kit.slots("b1") == []
        boxes = [await kit.claim() for _ in range(4)]
        assert sorted(set(b["key"] for b in boxes)) == ["b2", "b3"]
        for b in boxes:
            await kit.end(b, "close")
        # no detection without the option: nothing was counted
        assert kit.stats("b2")["failures"] == 0
        assert pool.eject_backend("b2", 5000) is True
        # b3 is the last one
        assert pool.eject_backend("b3", 5000) is False
        # an operator's refused request is no alarm
        assert kit.counter("ejection-refused") == 0
        assert pool.reinstate_backend("b2") is True
        assert pool.reinstate_backend("b2") is False
        assert kit.events[-1][:3] == ("reinstated", "b2", "manual")
        await kit.to(t0 + 5.0)
        assert kit.events[-1] == ("reinstated", "b1", "expired", t0 + 5.0)
        # a full member again
        boxes = [await kit.claim() for _ in range(4)]
        assert sorted(set(b["key"] for b in boxes)) == ["b1", "b2", "b3"]
        for b in boxes:
            await kit.end(b, "release")
        await kit.stop()
    run_vt(body)


def test_manual_ejection_with_the_option():
    async def body(loop):
        kit = Kit(loop, od=dict(OD, maxEjectionPercent=34))
        pool = kit.pool
        await settle(loop)
        assert pool.eject_backend("b1") is True
        assert kit.events[-1][2] == {"reason": "manual",
                                     "durationMs": BASE, "ejections": 1}
        # maxEjectionPercent is for the automatic kind
        assert pool.eject_backend("b2", 250) is True
        assert pool.eject_backend("b3", 250) is False
        assert kit.counter("ejection-refused") == 0
        assert pool.eject_backend("nope") is False
        assert kit.ejected() == ["b1", "b2"]
        assert pool.reinstate_backend("b1") is True
        assert pool.reinstate_backend("nope") is False
        for bad in ("1000", True):
            with pytest.raises(TypeError):
                pool.eject_backend("b1", bad)
        for bad in (0, -5, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                pool.eject_backend("b1", bad)
        await advance(loop, 0.25)
        assert kit.ejected() == []
        await kit.stop()
    run_vt(body)


def test_ejection_fails_over_to_the_next_srv_tier():
    async def body(loop):
        kit = Kit(loop, srvRanking=True, backends=(
            ("b1", {"priority": 0, "weight": 10}),
            ("b2", {"priority": 1, "weight": 10})))
        pool = kit.pool
        changes = []
        pool.on("priorityChanged", lambda old, new:
                changes.append((old, new)))
        await settle(loop)
        assert pool.get_ranking()["activePriority"] == 0
        assert kit.live("b2") == []
        await kit.fail_on("b1", 2)
        await settle(loop)
        assert kit.ejected() == ["b1"]
        assert changes == [(0, 1)]
        assert kit.live("b1") == [] and len(kit.live("b2")) >= 2
        t = kit.events[-1][3]
        await kit.to(t + 1.0)
        await advance(loop, 0.01)
        assert kit.ejected() == [] and changes == [(0, 1), (1, 0)]
        assert len(kit.live("b1")) >= 2 and kit.live("b2") == []
        await kit.stop()
    run_vt(body)


def test_stats_counters_gauge_and_snapshots():
    async def body(loop):
        plain = Kit(loop, od=None)
        kit = Kit(loop)
        pool = kit.pool
        await settle(loop)
        assert kit.stats() == {"enabled": True, "ejected": 0, "backends": {
            k: {"consecutiveFailures": 0, "failures": 0, "successes": 0,
                "ejected": False, "ejections": 0, "ejectedForMs": None,
                "reinstatesInMs": None} for k in ("b1", "b2", "b3")}}
        await kit.fail_on("b1", 2)
        await advance(loop, 0.25)
        st = kit.stats()
        assert st["ejected"] == 1
        assert st["backends"]["b1"]["ejected"] is True
        assert st["backends"]["b1"]["failures"] == 2
        assert st["backends"]["b1"]["ejections"] == 1
        text = pool.p_collector.collect()
        labels = 'pool="%s"' % pool.p_uuid.split("-")[0]
        line = [ln for ln in text.splitlines()
                if ln.startswith("cueball_pool_ejected_backends{")]
        assert len(line) == 1 and labels in line[0]
        assert 'domain="foobar"' in line[0]
        assert float(line[0].rsplit(" ", 1)[1]) == 1.0
        assert "cueball_pool_ejected_backends" not in \
            plain.pool.p_collector.collect()

        await advance(loop, 1.0)
        assert kit.counter("backend-ejected") == 1
        assert kit.counter("backend-reinstated") == 1
        assert kit.counter("ejection-refused") == 0
        await advance(loop, 0.25)
        line = [ln for ln in pool.p_collector.collect().splitlines()
                if ln.startswith("cueball_pool_ejected_backends{")]
        assert float(line[0].rsplit(" ", 1)[1]) == 0.0

        # the older surfaces keep their shape
        assert sorted(pool.get_stats()) == sorted(plain.pool.get_stats())
        assert sorted(pool.get_stats()) == [
            "counters", "idleConnections", "pendingConnections",
            "totalConnections", "waiterCount"]
        snap = monitor.get("pool", pool.p_uuid)
        assert sorted(snap) == sorted(
            monitor.get("pool", plain.pool.p_uuid))
        assert not any("eject" in k.lower() or "outlier" in k.lower()
                       for k in snap)
        await kit.stop()
        await plain.stop()
    run_vt(body)


@pytest.mark.parametrize("seed", [1, 7, 42, 1234, 99991])
def test_random_walk(seed):
    async def body(loop):
        rng = random.Random(seed)
        kit = Kit(loop, od=dict(OD, maxEjectionPercent=100,
                                maxEjectionTime=3000))
        pool = kit.pool
        await settle(loop)
        held = []
        n_claims = 0
        for _ in range(70):
            step = rng.choice(("claim", "claim", "outcome", "outcome",
                               "advance"))
            if step == "claim" and len(held) < 3:
                box = await kit.claim()
                if "hdl" in box:
                    n_claims += 1
                    # never from a backend that was out at that moment
                    assert box["key"] not in box["ejected"], box
                    held.append(box)
                else:
                    box["waiter"].cancel()
            elif step == "outcome" and held:
                box = held.pop(rng.randrange(len(held)))
                await kit.end(box, rng.choice(
                    ("release", "release", "close", "report", "error",
                     "sockclose")))
            else:
                await advance(loop, rng.choice((0.05, 0.3, 0.7, 1.5)))
            assert len(kit.ejected()) < 3
            assert pool.is_in_state("running")
        for box in held:
            await kit.end(box, "release")
        await advance(loop, 0.05)
        for key in kit.ejected():
            assert [s.get_state() for s in kit.slots(key)
                    if s.get_state() not in ("stopping", "stopped")] == []
            assert kit.live(key) == []
        assert n_claims > 10
        await kit.stop()
        assert kit.od_timers() == []
    run_vt(body)
