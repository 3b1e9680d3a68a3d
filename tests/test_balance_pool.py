"""A pool with ``claimBalancing`` on a VirtualLoop with fake
connections.  Smallest shape: two backends with two connections each
(spares 4, maximum 4); some cases need only one each."""

import math
import random

import pytest

from cueball_amd.errors import ClaimTimeoutError
from cueball_amd.testing import advance, settle
from conftest import run_vt
from balance_kit import Kit, idle_keys

ALL = {"choices": "all"}


# -- 1. equal costs are FIFO -------------------------------------------------

@pytest.mark.parametrize("policy", ["peakEwma", "leastLoaded"])
def test_equal_leases_are_claimed_in_fifo_order(policy):
    """Every lease is held 10 ms, one at a time and in overlapping
    pairs.  Under leastLoaded every cost is then equal whenever a claim
    chooses; under peakEwma every sample is the same 10 ms, and the
    backend whose estimate has aged longest is the one whose slot has
    sat longest in the idle queue, which is its head.  Either way the
    cheapest slot is the first in queue order, and the balanced pool
    claims exactly what the plain one does."""
    async def body(loop):
        plain = await Kit(loop).up()
        on = await Kit(loop, lb={"choices": "all", "policy": policy}).up()

        async def run(kit):
            seq = []
            for _ in range(12):
                seq.append(await kit.lease(10))
            for _ in range(6):
                a, b = kit.claim(), kit.claim()
                await settle(loop)
                seq += [a["key"], b["key"]]
                await advance(loop, 0.01)
                a["hdl"].release()
                b["hdl"].release()
                await settle(loop)
            return seq

        want = await run(plain)
        got = await run(on)
        assert want[:4] == ["b1", "b2", "b1", "b2"]
        assert got == want
        assert on.counter("balanced-claim") == 24
        assert on.counter("balanced-reordered") == 0
        assert plain.counter("balanced-claim") == 0
        await plain.stop()
        await on.stop()
    run_vt(body)


# -- 2. the workload of the issue ------------------------------------------------

HOLD = {"b1": 10, "b2": 100}


def test_a_slow_backend_is_shunned_while_there_is_headroom():
    """400 claims, one every 50 ms; b1 holds a lease 10 ms, b2 100 ms;
    no claim ever queues.  The pool without the option is the
    yardstick, run here too."""
    async def body(loop):
        off = await Kit(loop).up()
        keys, off_mean = await off.workload(400, 50, HOLD)
        off_b2 = keys.count("b2")
        assert len(keys) == 400
        assert off_b2 >= 0.30 * 400, off_b2
        assert off.counter("queued-claim") == 0

        on = await Kit(loop, lb=ALL).up()
        keys, on_mean = await on.workload(400, 50, HOLD)
        on_b2 = keys.count("b2")
        print("off: b2 %d, mean %.1f ms; all: b2 %d, mean %.1f ms"
              % (off_b2, off_mean, on_b2, on_mean))
        assert len(keys) == 400
        assert on_b2 <= 8, on_b2
        assert on_mean < off_mean / 2.0
        assert on.counter("queued-claim") == 0
        st = on.stats()
        assert st["backends"]["b1"]["picked"] == 400 - on_b2
        assert st["backends"]["b2"]["picked"] == on_b2
        assert st["backends"]["b1"]["leases"] == 400 - on_b2

        two = await Kit(loop, lb={"choices": 2,
                                  "rng": random.Random(1)}).up()
        keys, two_mean = await two.workload(400, 50, HOLD)
        two_b2 = keys.count("b2")
        print("two choices: b2 %d, mean %.1f ms" % (two_b2, two_mean))
        assert len(keys) == 400
        # both draws must land on b2's two slots of four: 1/6 of 400
        assert 0 < two_b2 < 100, two_b2
        for kit in (off, on, two):
            await kit.stop()
    run_vt(body)


# -- 3. aging re-admits -------------------------------------------------------

def test_an_aged_estimate_readmits_the_backend():
    async def body(loop):
        kit = await Kit(loop, lb={"choices": "all",
                                  "decayTime": 1000}).up()
        await kit.lease_on("b1", 10)
        await kit.lease_on("b2", 100)
        taught = loop.time()
        assert kit.stats("b1")["latencyMs"] < 10.0 + 1e-6
        assert kit.stats("b2")["latencyMs"] == pytest.approx(100.0)
        # both are fast from here on; b2 has to wait out its estimate
        fast = {"b1": 10, "b2": 10}
        keys, _ = await kit.workload(80, 50, fast,
                                     until=lambda key: key == "b2")
        assert keys[-1] == "b2" and keys.count("b2") == 1
        readmitted = (kit.served_at[-1] - taught) * 1000.0
        edge = 1000.0 * math.log(10.0)
        print("b2 claimed again %.0f ms after its last sample (edge %.0f)"
              % (readmitted, edge))
        assert edge <= readmitted <= edge + 200.0
        assert set(keys[:-1]) == {"b1"}
        await kit.stop()
    run_vt(body)


# -- 4. peak ---------------------------------------------------------------------

def test_one_slow_lease_lifts_the_estimate_at_once():
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        for _ in range(3):
            await kit.lease_on("b1", 10)
        assert kit.stats("b1")["latencyMs"] == pytest.approx(10.0)
        await kit.lease_on("b1", 100)
        assert kit.stats("b1")["latencyMs"] == pytest.approx(100.0)
        assert kit.stats("b1")["leases"] == 4
        # and one fast lease does not bring it back down
        await kit.lease_on("b1", 10)
        assert kit.stats("b1")["latencyMs"] > 99.0
        await kit.stop()
    run_vt(body)


# -- 5. outstanding -----------------------------------------------------------

def test_a_burst_sees_its_own_picks_and_releases_count_down():
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        boxes = [kit.claim() for _ in range(4)]
        await settle(loop)
        assert all(b["err"] is None for b in boxes)
        assert kit.outstanding() == {"b1": 2, "b2": 2}
        # the first two went to different backends: the second claim
        # saw the first one's pick
        assert {boxes[0]["key"], boxes[1]["key"]} == {"b1", "b2"}
        left = 4
        for box in boxes:
            box["hdl"].release()
            await settle(loop)
            left -= 1
            out = kit.outstanding()
            assert sum(out.values()) == left and max(out.values()) <= 2
        assert kit.outstanding() == {"b1": 0, "b2": 0}
        await kit.stop()
    run_vt(body)


def test_a_rejected_claim_leaves_no_count_behind():
    async def body(loop):
        kit = await Kit(loop, lb=ALL, per=1).up()
        head = kit.pool.p_idleq.peek()
        assert head.csf_backend["key"] == "b1"
        picks = []
        pick = kit.pool._lb_pick
        kit.pool._lb_pick = lambda avoid: picks.append(
            idle_keys(kit.pool)) or pick(avoid)
        box = kit.claim()
        # b1's socket dies now; its slot is still idle when the ticket
        # looks, takes the claim and rejects it
        conn = [c for c in kit.conns if c.key == "b1"][0]
        conn.emit("error", Exception("boom"))
        assert head.is_in_state("idle")
        await settle(loop)
        assert box["err"] is None and box["key"] == "b2"
        # two looks at the queue: b1 was handed over and took it back
        assert picks == [["b1", "b2"], ["b2"]]
        assert kit.outstanding() == {"b1": 0, "b2": 1}
        assert kit.stats("b1")["picked"] == 0
        assert kit.stats("b1")["leases"] == 0
        assert kit.counter("balanced-claim") == 1
        await advance(loop, 0.05)
        box["hdl"].release()
        await settle(loop)
        assert kit.outstanding() == {"b1": 0, "b2": 0}
        assert kit.stats("b1")["failedLeases"] == 0
        await kit.stop()
    run_vt(body)


def test_a_waiter_fed_on_release_is_counted_on_its_backend():
    async def body(loop):
        kit = await Kit(loop, lb=ALL, per=1).up()
        a, b = kit.claim(), kit.claim()
        await settle(loop)
        waiting = kit.claim()
        await settle(loop)
        assert "err" not in waiting
        assert kit.pool.get_stats()["waiterCount"] == 1
        assert kit.outstanding() == {"b1": 1, "b2": 1}
        b["hdl"].release()
        await settle(loop)
        assert waiting["err"] is None and waiting["key"] == b["key"]
        assert kit.outstanding() == {"b1": 1, "b2": 1}
        # the balancer chose two of the three
        assert kit.counter("balanced-claim") == 2
        a["hdl"].release()
        await settle(loop)
        assert kit.outstanding() == {a["key"]: 0, b["key"]: 1}
        await advance(loop, 0.02)
        waiting["hdl"].release()
        await settle(loop)
        assert kit.outstanding() == {"b1": 0, "b2": 0}
        assert kit.stats(b["key"])["leases"] == 2
        await kit.stop()
    run_vt(body)


# -- 6. failed leases -----------------------------------------------------------

@pytest.mark.parametrize("how", ["close", "report"])
def test_a_failed_lease_is_counted_and_leaves_no_sample(how):
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        await kit.lease_on("b1", 10)
        await kit.lease_on("b2", 10)
        before = kit.pool.p_lb_backends["b1"].ewma.value
        assert before == pytest.approx(10.0)
        got = await kit.lease(1, {"avoidBackends": ["b2"]}, how=how)
        assert got == "b1"
        await advance(loop, 0.05)
        st = kit.stats("b1")
        assert st["failedLeases"] == 1 and st["leases"] == 2
        assert st["outstanding"] == 0
        # a 1 ms lease would have pulled the estimate down
        rec = kit.pool.p_lb_backends["b1"]
        assert rec.ewma.value == before
        assert kit.stats("b2")["failedLeases"] == 0
        await kit.stop()
    run_vt(body)


def test_pinger_leases_change_nothing():
    async def body(loop):
        pings = []

        def checker(hdl, conn):
            pings.append(conn.key)
            loop.call_later(0.005, hdl.release)

        kit = await Kit(loop, lb=ALL, checker=checker,
                        checkTimeout=100).up()
        await kit.lease_on("b1", 10)
        before = kit.stats()
        counters = dict(kit.pool.get_stats()["counters"])
        await advance(loop, 0.5)
        assert len(pings) >= 4
        after = kit.stats()
        for k in ("b1", "b2"):
            for field in ("outstanding", "leases", "failedLeases",
                          "picked"):
                assert after["backends"][k][field] == \
                    before["backends"][k][field], (k, field)
        assert after["backends"]["b2"]["latencyMs"] is None
        assert kit.pool.p_lb_backends["b1"].ewma.value == \
            pytest.approx(10.0)
        assert kit.pool.get_stats()["counters"] == counters
        assert not kit.pool.p_lb_open and not kit.pool.p_lb_handed
        await kit.stop()
    run_vt(body)


# -- 7. with avoidBackends ----------------------------------------------------

def test_avoid_narrows_the_candidates_first():
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        await kit.lease_on("b1", 10)
        await kit.lease_on("b2", 100)
        pool = kit.pool
        # avoiding the cheap backend yields the dear one; the slots
        # passed over stay linked where they are
        order = list(pool.p_idleq)
        head = pool.p_idleq.peek()
        box = kit.claim({"avoidBackends": ["b1"]})
        await settle(loop)
        assert box["key"] == "b2"
        taken = box["hdl"].ch_slot
        assert taken.p_idleq_node is None
        assert list(pool.p_idleq) == [f for f in order if f is not taken]
        assert pool.p_idleq.peek() is head
        assert all(f.p_idleq_node is not None and f.is_in_state("idle")
                   for f in pool.p_idleq)
        box["hdl"].release()
        await settle(loop)

        # avoiding every idle backend yields the cheapest of all
        order = list(pool.p_idleq)
        box = kit.claim({"avoidBackends": ["b1", "b2"]})
        await settle(loop)
        assert box["key"] == "b1"
        first_b1 = [f for f in order if f.csf_backend["key"] == "b1"][0]
        assert box["hdl"].ch_slot is first_b1
        assert list(pool.p_idleq) == [f for f in order if f is not first_b1]
        assert kit.counter("queued-claim") == 0
        box["hdl"].release()
        await settle(loop)
        await kit.stop()
    run_vt(body)


def test_a_stale_entry_met_on_the_walk_is_unlinked():
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        pool = kit.pool
        head = pool.p_idleq.peek()
        seen = {}
        box = kit.claim()

        def probe(st):
            # runs right after the claim's ticket, in the same emit
            if st == "waiting" and not seen:
                seen["node"] = head.p_idleq_node
                seen["idle"] = idle_keys(pool)

        box["waiter"].on("stateChanged", probe)
        head.set_unwanted()
        assert not head.is_in_state("idle")
        assert head.p_idleq_node is not None
        await settle(loop)
        assert seen == {"node": None, "idle": ["b1", "b2"]}
        assert box["err"] is None and box["key"] == "b2"
        await advance(loop, 0.01)
        box["hdl"].release()
        await settle(loop)
        await kit.stop()
    run_vt(body)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_two_choices_never_take_a_stale_entry(seed):
    """Three claims in one loop turn, three live idle slots and one
    that has left 'idle' without the pool having heard: whatever is
    drawn, every claim is served from a live slot and none queues."""
    async def body(loop):
        kit = await Kit(loop, lb={"choices": 2,
                                  "rng": random.Random(seed)}).up()
        pool = kit.pool
        slots = list(pool.p_idleq)
        stale = slots[2]
        boxes = [kit.claim() for _ in range(3)]
        stale.set_unwanted()
        assert not stale.is_in_state("idle")
        assert stale.p_idleq_node is not None
        await settle(loop)
        assert [b["err"] for b in boxes] == [None] * 3
        got = [b["hdl"].ch_slot for b in boxes]
        assert stale not in got and len(set(got)) == 3
        assert set(got) == set(slots) - {stale}
        assert kit.counter("queued-claim") == 0
        assert stale.p_idleq_node is None
        assert sum(kit.outstanding().values()) == 3
        for b in boxes:
            b["hdl"].release()
        await settle(loop)
        assert sum(kit.outstanding().values()) == 0
        await kit.stop()
    run_vt(body)


# -- 8. backend removal---------------------------------------------------------

def test_a_removed_backend_loses_its_record():
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        await kit.lease_on("b1", 10)
        await kit.lease_on("b2", 100)
        assert set(kit.stats()["backends"]) == {"b1", "b2"}
        kit.resolver.remove("b2")
        await advance(loop, 0.1)
        assert set(kit.stats()["backends"]) == {"b1"}
        assert set(kit.pool.p_lb_backends) == {"b1"}
        kit.resolver.add("b2", {"address": "10.0.0.1", "port": 80})
        await advance(loop, 0.1)
        st = kit.stats("b2")
        assert st["latencyMs"] is None
        assert st["leases"] == 0 and st["picked"] == 0
        assert st["outstanding"] == 0
        # it borrows b1's estimate
        assert st["cost"] == pytest.approx(kit.stats("b1")["cost"])
        await kit.stop()
    run_vt(body)


def test_the_record_survives_ejection():
    async def body(loop):
        kit = await Kit(loop, lb=ALL).up()
        await kit.lease_on("b1", 10)
        await kit.lease_on("b2", 100)
        assert kit.pool.eject_backend("b2", 500) is True
        await advance(loop, 0.2)
        st = kit.stats("b2")
        assert st["connections"] == 0 and st["leases"] == 1
        assert 0 < st["latencyMs"] < 100.0
        await advance(loop, 1.0)
        assert kit.stats("b2")["connections"] > 0
        assert kit.stats("b2")["leases"] == 1
        await kit.stop()
    run_vt(body)


# -- 9. leastLoaded -----------------------------------------------------------------

def test_least_loaded_goes_where_fewer_leases_are():
    async def body(loop):
        kit = await Kit(loop, lb={"choices": "all",
                                  "policy": "leastLoaded"}).up()
        # b1 proves to be much the faster one: it does not matter
        await kit.lease_on("b2", 200)
        held = kit.claim({"avoidBackends": ["b2"]})
        await settle(loop)
        assert held["key"] == "b1"
        # b1's other slot is at the head of the queue
        assert idle_keys(kit.pool)[0] == "b1"
        box = kit.claim()
        await settle(loop)
        assert box["key"] == "b2"
        assert kit.counter("balanced-reordered") >= 1
        assert kit.stats("b1")["cost"] == 2.0
        assert kit.stats("b2")["cost"] == 2.0
        for b in (held, box):
            b["hdl"].release()
        await settle(loop)
        await kit.stop()
    run_vt(body)


# -- 10. queueing ---------------------------------------------------------------------

def test_claims_beyond_the_idle_slots_queue_in_order():
    async def body(loop):
        async def run(kit):
            held = [kit.claim() for _ in range(2)]
            await settle(loop)
            queued = [kit.claim({"timeout": 500}) for _ in range(3)]
            await settle(loop)
            assert all("err" not in q for q in queued)
            st = kit.pool.get_stats()
            assert st["waiterCount"] == 3
            assert st["counters"]["queued-claim"] == 3
            served = []
            for q in queued:
                q["waiter"].on("stateChanged", lambda st, q=q:
                               st == "claimed" and served.append(q))
            held[0]["hdl"].release()
            await settle(loop)
            assert served == [queued[0]]
            held[1]["hdl"].release()
            await settle(loop)
            assert served == queued[:2]
            # the third times out like any other waiter
            await advance(loop, 0.6)
            assert isinstance(queued[2]["err"], ClaimTimeoutError)
            assert kit.pool.get_stats()["waiterCount"] == 0
            for q in queued[:2]:
                q["hdl"].release()
            await settle(loop)
            return dict(kit.pool.get_stats()["counters"])

        plain = await Kit(loop, per=1).up()
        on = await Kit(loop, lb=ALL, per=1).up()
        want = await run(plain)
        got = await run(on)
        assert got.pop("balanced-claim") == 2
        got.pop("balanced-reordered", None)
        assert got == want
        await plain.stop()
        await on.stop()
    run_vt(body)


def test_on_a_target_claim_delay_pool():
    async def body(loop):
        kit = await Kit(loop, lb=ALL, per=1, targetClaimDelay=200).up()
        assert kit.pool.p_codel is not None
        with pytest.raises(ValueError):
            kit.pool.claim({"timeout": 100}, lambda *a: None)
        held = [kit.claim() for _ in range(2)]
        await settle(loop)
        assert {h["key"] for h in held} == {"b1", "b2"}
        waiting = kit.claim()
        await settle(loop)
        assert "err" not in waiting
        # never fed: shed at CoDel's maximum idle time
        await advance(loop, kit.pool.p_codel.get_max_idle() / 1000.0 + 0.1)
        assert isinstance(waiting["err"], ClaimTimeoutError)
        late = kit.claim()
        await settle(loop)
        held[0]["hdl"].release()
        await settle(loop)
        assert late["err"] is None and late["key"] == held[0]["key"]
        for b in (held[1], late):
            b["hdl"].release()
        await settle(loop)
        assert kit.outstanding() == {"b1": 0, "b2": 0}
        await kit.stop()
    run_vt(body)


def test_a_stopping_pool_fails_the_claim_as_before():
    async def body(loop):
        kit = await Kit(loop, lb=ALL, per=1).up()
        box = kit.claim()
        kit.pool.stop()
        await settle(loop)
        assert box["err"] is not None
        assert type(box["err"]).__name__ == "PoolStoppingError"
        late = kit.claim()
        await settle(loop)
        assert type(late["err"]).__name__ == "PoolStoppingError"
        await advance(loop, 30.0)
        assert kit.pool.is_in_state("stopped")
    run_vt(body)
