"""``concurrencyLimit`` in a pool: the ticket gate, the feed gate and the
kick, sizing, the other options beside it, and the count of leases in
flight however they end.  Sixteen connections on a DummyResolver, on the
virtual clock; passes on both runtimes."""

import pytest

from cueball_amd.testing import advance, settle
from conftest import run_vt
from balance_kit import idle_keys
from limit_kit import BASE, CLAIMERS, LimitKit

#: a limit that stays where it is put: no window is ever over this
FIXED = {"algorithm": "aimd", "latencyThreshold": 1e9, "initialLimit": 2,
         "maxLimit": 2}


def counter(kit, name):
    return kit.pool.get_stats()["counters"].get(name, 0)


def test_the_ticket_gate_queues_the_third_claim_beside_idle_slots():
    async def body(loop):
        kit = await LimitKit(loop, FIXED).up()
        kit.queue("a")
        kit.queue("b")
        kit.queue("c")
        await settle(loop)
        assert kit.served() == ["a", "b"]
        assert kit.order() == ["c"] and kit.idle() == 14
        assert kit.in_flight() == 2 and kit.limit()["allowed"] == 2
        assert counter(kit, "limit-held") == 1
        assert counter(kit, "queued-claim") == 1
        assert counter(kit, "max-claim-queue") == 1
        await advance(loop, 0.03)
        assert kit.order() == ["c"] and kit.in_flight() == 2
        kit.boxes["a"]["hdl"].release()
        await settle(loop)
        assert kit.served() == ["a", "b", "c"] and kit.order() == []
        assert kit.in_flight() == 2
        assert counter(kit, "limit-held") == 1
        # a claim that finds nothing idle at all is not one the limit held
        kit2 = await LimitKit(loop, FIXED, backends=("b1",), per=2).up()
        for label in "xyz":
            kit2.queue(label)
        await settle(loop)
        assert kit2.order() == ["z"] and counter(kit2, "limit-held") == 0
        assert counter(kit2, "queued-claim") == 1
        for label in "bc":
            kit.boxes[label]["hdl"].release()
        for label in "xy":
            kit2.boxes[label]["hdl"].release()
        await settle(loop)
        kit2.boxes["z"]["hdl"].release()
        await settle(loop)
        assert kit.in_flight() == 0 and kit2.in_flight() == 0
        await kit.stop()
        await kit2.stop()
    run_vt(body)


def test_the_feed_gate_parks_slots_in_a_probe_and_the_kick_serves_after():
    async def body(loop):
        cl = {"window": 100, "minSamples": 2, "probeSamples": 2,
              "probeLimit": 1, "probeSpread": 0, "probeInterval": 1000,
              "initialLimit": 4, "maxLimit": 4}
        kit = await LimitKit(loop, cl).up()
        assert kit.limit()["probing"] and kit.limit()["allowed"] == 1
        # the first probe: two leases of 10 ms, one after the other
        for _ in range(2):
            await kit.lease(10)
        assert kit.events == [(4, 1)]
        st = kit.limit()
        assert not st["probing"] and st["baselineMs"] == pytest.approx(10.0)
        assert st["allowed"] == 4 and st["limit"] == 4.0
        # 1000 ms after the first lease began the next probe is due
        await advance(loop, 1.0)
        for label in "ABCD":
            kit.queue(label)
        await settle(loop)
        for label in ("w1", "w2", "w3", "w4", "w5"):
            kit.queue(label)
            await settle(loop)
        assert kit.served() == list("ABCD")
        assert kit.order() == ["w1", "w2", "w3", "w4", "w5"]
        assert counter(kit, "limit-held") == 5 and kit.idle() == 12
        await advance(loop, 0.02)

        # A's end is the sample at which the probe begins: allowed 1
        kit.boxes["A"]["hdl"].release()
        await settle(loop)
        assert kit.events == [(4, 1), (1, 4)]
        assert kit.limit()["probing"] and counter(kit, "limit-probe") == 1
        assert kit.in_flight() == 3 and kit.idle() == 13
        assert kit.order() == ["w1", "w2", "w3", "w4", "w5"]
        for label, left in (("B", 2), ("C", 1)):
            kit.boxes[label]["hdl"].release()
            await settle(loop)
            assert kit.in_flight() == left
            assert kit.order() == ["w1", "w2", "w3", "w4", "w5"]
        assert kit.idle() == 15
        # with D gone there is room for one: D's slot feeds the head
        kit.boxes["D"]["hdl"].release()
        await settle(loop)
        assert kit.served()[4:] == ["w1"] and kit.in_flight() == 1
        assert kit.idle() == 15 and kit.limit()["limit"] == 4.0
        await advance(loop, 0.02)
        kit.boxes["w1"]["hdl"].release()
        await settle(loop)
        assert kit.served()[4:] == ["w1", "w2"] and kit.in_flight() == 1
        assert kit.limit()["probing"]
        await advance(loop, 0.03)
        head = idle_keys(kit.pool)[:2]
        # the probe's second sample ends it: room for four
        kit.boxes["w2"]["hdl"].release()
        await settle(loop)
        assert kit.events == [(4, 1), (1, 4), (4, 1)]
        st = kit.limit()
        assert not st["probing"] and st["limit"] == 4.0
        assert st["baselineMs"] == pytest.approx(25.0)
        assert kit.served()[4:] == ["w1", "w2", "w3", "w4", "w5"]
        assert kit.order() == [] and kit.in_flight() == 3
        # w3 took the slot that w2 gave back; the kick served the others
        # from the head of the idle queue, in its order
        assert kit.key("w3") == kit.key("w2")
        assert [kit.key("w4"), kit.key("w5")] == head == ["b3", "b4"]
        for label in ("w3", "w4", "w5"):
            kit.boxes[label]["hdl"].release()
        await settle(loop)
        assert kit.in_flight() == 0 and kit.idle() == 16
        await kit.stop()
    run_vt(body)


def test_the_closed_loop_keeps_a_saturated_server_at_its_knee():
    async def body(loop):
        seconds = 12.0
        plain = await LimitKit(loop).up()
        off = await plain.closed_loop(seconds)
        await plain.stop()
        kit = await LimitKit(loop, {
            "algorithm": "aimd", "latencyThreshold": 75, "window": 200,
            "minSamples": 5}).up()
        on = await kit.closed_loop(seconds)
        st = kit.limit()
        assert st["inFlight"] == 0

        def mean(xs):
            return sum(xs) / len(xs)

        off_peak = max(a for t, a in off["peaks"] if t > seconds / 2)
        off_mean = mean([h for t, h in off["leases"]])
        late_peak = max(a for t, a in on["peaks"] if t > seconds / 2)
        late_mean = mean([h for t, h in on["leases"] if t > seconds / 2])
        print("off: peak", off_peak, "mean", off_mean, "served",
              off["served"], "on: late peak", late_peak, "late mean",
              late_mean, "served", on["served"], st)
        assert off_peak == CLAIMERS
        assert off_mean == pytest.approx(4 * BASE, rel=0.02)
        assert late_peak <= 8
        assert late_mean <= 2 * BASE
        assert on["served"] >= 0.75 * off["served"]
        assert st["windows"] > 20 and st["lowered"] > 5
        await kit.stop()
    run_vt(body)


def test_held_waiters_do_not_open_connections_the_limit_forbids():
    async def body(loop):
        cl = {"algorithm": "aimd", "latencyThreshold": 1e9, "window": 100,
              "minSamples": 2, "initialLimit": 3}
        kit = await LimitKit(loop, cl, spares=2, maximum=16).up_auto()
        total = lambda: kit.pool.get_stats()["totalConnections"]  # noqa: E731
        assert total() == 2
        for n in range(13):
            kit.queue("c%d" % n)
        await advance(loop, 0.5)
        assert kit.in_flight() == 3 and kit.waiting() == 10
        assert total() == 3 + 2
        # leases of 60 ms, each followed by the next waiter: every window
        # is under the threshold at its peak, so the limit climbs
        done = 0
        seen = []
        while kit.waiting() > 0:
            await advance(loop, 0.06)
            live = [l for l in kit.served() if l not in seen]
            label = live[0]
            seen.append(label)
            kit.boxes[label]["hdl"].release()
            await advance(loop, 0.05)
            done += 1
            limit = kit.limit()["limit"]
            assert total() <= int(limit) + 2, (done, limit)
        limit = kit.limit()["limit"]
        assert limit >= 5.0 and counter(kit, "limit-raised") >= 2
        assert total() > 3 + 2
        for label in kit.served():
            if label not in seen:
                kit.boxes[label]["hdl"].release()
        await advance(loop, 0.05)
        assert kit.in_flight() == 0
        await kit.stop()
    run_vt(body)


# -- beside the other options ------------------------------------------------

def test_with_claim_queue_the_bound_and_the_classes_apply_to_held_claims():
    async def body(loop):
        kit = await LimitKit(loop, FIXED,
                             {"maxQueued": 2, "priorities": 2}).up()
        kit.queue("a", 1)
        kit.queue("b", 1)
        await settle(loop)
        await kit.queue_all([("w1", 1), ("w2", 1), ("w3", 0)])
        # held beside 14 idle slots, and bound like any waiters
        assert kit.idle() == 14 and kit.order() == ["w3", "w1"]
        assert kit.log[-1] == ("w2", "ClaimQueueFullError")
        assert kit.errors["w2"].displaced is True
        assert counter(kit, "limit-held") == 3
        assert counter(kit, "queue-shed") == 1
        # a lease that is closed frees no slot, only room: the kick
        # serves the head, class 0 first, from the idle queue
        kit.boxes["a"]["hdl"].close()
        await settle(loop)
        assert kit.served() == ["a", "b", "w3"] and kit.order() == ["w1"]
        kit.boxes["b"]["hdl"].close()
        await settle(loop)
        assert kit.served() == ["a", "b", "w3", "w1"]
        assert kit.in_flight() == 2
        for label in ("w3", "w1"):
            kit.boxes[label]["hdl"].release()
        await advance(loop, 0.1)
        assert kit.in_flight() == 0
        await kit.stop()
    run_vt(body)


def test_with_target_claim_delay_a_held_claim_past_it_is_shed_at_the_kick():
    async def body(loop):
        kit = await LimitKit(loop, FIXED, targetClaimDelay=50).up()
        kit.queue("a")
        kit.queue("b")
        await settle(loop)
        for label in ("w1", "w2", "w3"):
            kit.queue(label)
        await settle(loop)
        assert kit.order() == ["w1", "w2", "w3"] and kit.idle() == 14
        # 60 ms: w1 is past the target, which starts CoDel's interval
        await advance(loop, 0.06)
        kit.boxes["a"]["hdl"].close()
        await settle(loop)
        assert kit.served() == ["a", "b", "w1"]
        # 270 ms: past the interval and still past the target
        await advance(loop, 0.21)
        assert kit.order() == ["w2", "w3"]
        kit.boxes["w1"]["hdl"].close()
        await settle(loop)
        assert ("w2", "ClaimTimeoutError") in kit.log
        assert kit.served() == ["a", "b", "w1", "w3"]
        assert counter(kit, "claim-timeout") == 1
        assert kit.order() == [] and kit.in_flight() == 2
        for label in ("b", "w3"):
            kit.boxes[label]["hdl"].release()
        await advance(loop, 0.1)
        assert kit.in_flight() == 0
        await kit.stop()
    run_vt(body)


def test_with_claim_balancing_the_gate_comes_before_the_choice():
    async def body(loop):
        kit = await LimitKit(loop, FIXED,
                             claimBalancing={"choices": "all"}).up()
        for label in "abc":
            kit.queue(label)
        await settle(loop)
        assert kit.served() == ["a", "b"] and kit.order() == ["c"]
        assert counter(kit, "balanced-claim") == 2
        assert counter(kit, "limit-held") == 1 and kit.idle() == 14
        assert sum(kit.outstanding().values()) == 2
        kit.boxes["a"]["hdl"].release()
        await settle(loop)
        assert kit.served() == ["a", "b", "c"] and kit.in_flight() == 2
        for label in "bc":
            kit.boxes[label]["hdl"].release()
        await settle(loop)
        assert kit.in_flight() == 0
        assert sum(kit.outstanding().values()) == 0
        await kit.stop()
    run_vt(body)


def test_with_claim_affinity_keyed_and_keyless_claims_pass_the_gate():
    async def body(loop):
        kit = await LimitKit(loop, FIXED, claimAffinity={}).up()
        first = kit.pool.get_affinity_order("user:1")[0]
        kit.queue("a", affinityKey="user:1")
        kit.queue("b")
        await settle(loop)
        assert kit.served() == ["a", "b"] and kit.key("a") == first
        kit.queue("c", affinityKey="user:1")
        kit.queue("d")
        await settle(loop)
        assert kit.order() == ["c", "d"] and kit.idle() == 14
        assert counter(kit, "limit-held") == 2
        assert kit.pool.get_affinity_stats()["queued"] == 1
        for label in "ab":
            kit.boxes[label]["hdl"].release()
        await settle(loop)
        assert kit.served() == ["a", "b", "c", "d"]
        for label in "cd":
            kit.boxes[label]["hdl"].release()
        await settle(loop)
        assert kit.in_flight() == 0
        await kit.stop()
    run_vt(body)


def test_with_avoid_backends_the_gate_comes_first_and_has_idle_says_no():
    async def body(loop):
        kit = await LimitKit(loop, FIXED).up()
        assert kit.pool.has_idle_connection() is True
        kit.queue("a", avoidBackends=["b1"])
        await settle(loop)
        assert kit.key("a") == "b2"         # below the limit it chooses
        assert kit.pool.has_idle_connection() is True
        kit.queue("b")
        await settle(loop)
        assert kit.in_flight() == 2 and kit.idle() == 14
        assert kit.pool.has_idle_connection() is False
        assert kit.pool.has_idle_connection(["b1"]) is False
        kit.queue("c", avoidBackends=["b1"])
        await settle(loop)
        assert kit.order() == ["c"] and counter(kit, "limit-held") == 1
        kit.boxes["b"]["hdl"].release()
        await settle(loop)
        assert kit.served() == ["a", "b", "c"]
        for label in "ac":
            kit.boxes[label]["hdl"].release()
        await settle(loop)
        assert kit.pool.has_idle_connection() is True
        assert kit.in_flight() == 0
        await kit.stop()
    run_vt(body)


def test_error_on_empty_is_unchanged():
    async def body(loop):
        kit = LimitKit(loop, FIXED)
        kit.resolver_fsm.start()
        await settle(loop)
        kit.queue("a", errorOnEmpty=True)
        await settle(loop)
        assert kit.log == [("a", "NoBackendsError")]
        kit.pool.stop()
        await advance(loop, 1.0)
    run_vt(body)


# -- accounting ----------------------------------------------------------------

async def end_release(kit, box):
    box["hdl"].release()


async def end_close(kit, box):
    box["hdl"].close()


async def end_report_failure(kit, box):
    box["hdl"].report_failure()
    box["hdl"].release()


async def end_socket_error(kit, box):
    box["conn"].on("error", lambda err: None)
    box["conn"].emit("error", Exception("boom"))
    await settle(kit.loop)
    box["hdl"].release()


async def end_backend_removal(kit, box):
    kit.resolver.remove(box["conn"].key)
    await settle(kit.loop)
    box["hdl"].release()


async def end_pool_stop(kit, box):
    kit.pool.stop()
    await settle(kit.loop)
    box["hdl"].release()


ENDS = {"release": (end_release, True), "close": (end_close, False),
        "report_failure": (end_report_failure, False),
        "socket-error": (end_socket_error, False),
        "backend-removal": (end_backend_removal, True),
        "pool-stop": (end_pool_stop, True)}


@pytest.mark.parametrize("how", sorted(ENDS))
def test_in_flight_returns_to_zero_however_a_lease_ends(how):
    async def body(loop):
        end, sampled = ENDS[how]
        kit = await LimitKit(loop, FIXED).up()
        kit.queue("a")
        kit.queue("b")
        kit.queue("w")
        await settle(loop)
        assert kit.in_flight() == 2 and kit.order() == ["w"]
        await advance(loop, 0.02)
        for label in "ab":
            await end(kit, kit.boxes[label])
        await advance(loop, 0.2)
        st = kit.limit()
        if how == "pool-stop":
            assert kit.log[-1] == ("w", "PoolStoppingError")
            assert st["inFlight"] == 0
        else:
            # the waiter was fed, by the slot or by the kick
            assert kit.served() == ["a", "b", "w"] and kit.order() == []
            assert st["inFlight"] == 1
            kit.boxes["w"]["hdl"].release()
            await advance(loop, 0.05)
            st = kit.limit()
            assert st["inFlight"] == 0
        assert kit.pool.p_cl_lim.in_flight == 0
        assert not kit.pool.p_cl_open and not kit.pool.p_cl_handed
        assert st["discarded"] == (0 if sampled else 2)
        assert st["samples"] == (2 if sampled else 0) + \
            (0 if how == "pool-stop" else 1)
        if how != "pool-stop":
            await kit.stop()
        else:
            await advance(loop, 30.0)
            assert kit.pool.is_in_state("stopped")
    run_vt(body)


def test_a_held_claim_that_times_out_or_is_cancelled_was_never_in_flight():
    async def body(loop):
        kit = await LimitKit(loop, FIXED).up()
        kit.queue("a")
        kit.queue("b")
        kit.queue("slow", timeout=50)
        kit.queue("gone")
        kit.queue("w")
        await settle(loop)
        assert kit.order() == ["slow", "gone", "w"]
        kit.boxes["gone"]["waiter"].cancel()
        await advance(loop, 0.06)
        assert kit.log[-1] == ("slow", "ClaimTimeoutError")
        assert kit.order() == ["w"] and kit.in_flight() == 2
        kit.boxes["a"]["hdl"].release()
        await settle(loop)
        assert kit.served() == ["a", "b", "w"]
        assert kit.boxes["gone"]["fired"] == 0
        for label in "bw":
            kit.boxes[label]["hdl"].release()
        await settle(loop)
        assert kit.in_flight() == 0 and kit.waiting() == 0
        assert kit.idle() == 16
        await kit.stop()
    run_vt(body)


def test_pinger_leases_are_never_seen():
    async def body(loop):
        pings = []

        def checker(hdl, conn):
            pings.append(hdl)
            loop.call_later(0.005, hdl.release)

        kit = await LimitKit(loop, FIXED, checker=checker,
                             checkTimeout=100).up()
        await advance(loop, 0.102)
        assert len(pings) == 16
        assert any(h.is_in_state("claimed") for h in pings)
        assert kit.in_flight() == 0 and kit.pool.p_cl_lim.in_flight == 0
        await advance(loop, 0.5)
        st = kit.limit()
        assert st["inFlight"] == 0 and st["samples"] == 0
        assert st["discarded"] == 0 and len(pings) > 16
        await kit.stop()
    run_vt(body)


def test_the_gauges_are_published_from_the_tick():
    async def body(loop):
        kit = await LimitKit(loop, FIXED).up()
        kit.queue("a")
        await advance(loop, 0.5)
        text = kit.pool.p_collector.collect()
        assert "cueball_pool_concurrency_limit" in text
        assert "cueball_pool_in_flight" in text
        lines = [l for l in text.splitlines() if not l.startswith("#")]
        assert [l for l in lines
                if l.startswith("cueball_pool_concurrency_limit")
                ][0].split()[-1] in ("2", "2.0")
        assert [l for l in lines if l.startswith("cueball_pool_in_flight")
                ][0].split()[-1] in ("1", "1.0")
        kit.boxes["a"]["hdl"].release()
        await settle(loop)
        await kit.stop()
    run_vt(body)
