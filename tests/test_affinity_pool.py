"""A pool with ``claimAffinity`` on a VirtualLoop with fake connections,
at the smallest shapes that show each rule.  The orders used here are
the vectors of test_affinity_hash.py: over b1, b2 the first choice of
``k0`` is b1 and that of ``k1`` is b2; over b1, b2, b3 the order of
``k0`` is b1 b3 b2, that of ``k1`` is b2 b1 b3, that of ``k2`` is
b3 b2 b1."""

import pytest

from cueball_amd.affinity import order as affinity_order
from cueball_amd.errors import ClaimTimeoutError
from cueball_amd.testing import advance, settle
from conftest import run_vt
from balance_kit import Kit, idle_keys

B3 = ("b1", "b2", "b3")


def keyed(key, **more):
    opts = {"affinityKey": key}
    opts.update(more)
    return opts


def af_counters(kit):
    return {name[len("affinity-"):]: n
            for name, n in kit.pool.get_stats()["counters"].items()
            if name.startswith("affinity-")}


async def release(kit, *boxes):
    for box in boxes:
        box["hdl"].release()
    await settle(kit.loop)


# -- 1. the key chooses, whatever the queue order ------------------------------------

@pytest.mark.parametrize("backends", [("b1", "b2"), ("b2", "b1")])
def test_the_key_chooses_whatever_the_queue_order(backends):
    async def body(loop):
        kit = await Kit(loop, per=1, claimAffinity={}).up()
        pool = kit.pool
        if backends[0] == "b2":
            # b1 goes to the back of the queue
            assert await kit.lease(1) == "b1"
        assert idle_keys(pool) == list(backends)
        assert pool.get_affinity_order(b"k0") == ["b1", "b2"]
        assert pool.get_affinity_order("k1") == ["b2", "b1"]
        head, other = backends
        want = "k0" if other == "b1" else "k1"

        # the key of the second slot in the queue: the head is passed
        # over and stays linked at the head
        head_node = next(iter(pool.p_idleq)).p_idleq_node
        box = kit.claim(keyed(want))
        await settle(loop)
        assert box["key"] == other
        assert box["hdl"].get_backend()["key"] == other
        assert idle_keys(pool) == [head]
        assert next(iter(pool.p_idleq)).p_idleq_node is head_node
        assert head_node.linked
        await release(kit, box)
        assert idle_keys(pool) == [head, other]

        # bytes and str are one key
        for key in (b"k0", "k0"):
            assert await kit.lease(1, keyed(key)) == "b1"
        for key in (b"k1", "k1"):
            assert await kit.lease(1, keyed(key)) == "b2"
        assert af_counters(kit) == {"claim": 5, "hit": 5}

        # a claim without a key takes the head, as before, and is none
        # of affinity's business
        order = idle_keys(pool)
        assert await kit.lease(1) == order[0]
        assert await kit.lease(1, {}) == order[1]
        assert af_counters(kit) == {"claim": 5, "hit": 5}
        assert kit.counter("queued-claim") == 0
        await kit.stop()
    run_vt(body)


# -- 2. the load bound -----------------------------------------------------------------

WITH_BOUND = (["b1", "b1", "b2", "b1", "b2"],
              {"claim": 5, "hit": 3, "spill-load": 1, "spill-busy": 1})
NO_BOUND = (["b1", "b1", "b1", "b2", "b2"],
            {"claim": 5, "hit": 3, "spill-busy": 2})


@pytest.mark.parametrize("option, burst, want", [
    ({"loadFactor": 1.25}, False, WITH_BOUND),
    ({}, False, WITH_BOUND),
    ({"loadFactor": 1.25}, True, WITH_BOUND),
    ({"loadFactor": None}, False, NO_BOUND),
    ({"loadFactor": None}, True, NO_BOUND),
])
def test_five_concurrent_claims_of_one_key(option, burst, want):
    """Two backends with three connections each.  With the bound, by
    the load_cap table: the third claim finds b1 with 2 in use against a
    cap of ceil(1.25 * 3 / 2) = 2 and spills; the fourth finds a cap of
    ceil(1.25 * 4 / 2) = 3 and is a hit; the fifth finds b1 all in
    use."""
    async def body(loop):
        kit = await Kit(loop, per=3, claimAffinity=option).up()
        boxes = []
        for _ in range(5):
            boxes.append(kit.claim(keyed(b"k0")))
            if not burst:
                await settle(loop)
        await settle(loop)
        keys, counters = want
        assert [b["key"] for b in boxes] == keys
        assert af_counters(kit) == counters
        st = kit.pool.get_affinity_stats()
        assert st["enabled"] is True
        assert st["loadFactor"] == option.get("loadFactor", 1.25)
        assert st["claims"] == 5 and st["hits"] == 3
        assert st["spilledLoad"] == counters.get("spill-load", 0)
        assert st["spilledBusy"] == counters["spill-busy"]
        assert st["queued"] == 0
        assert st["backends"] == {
            "b1": {"connections": 3, "idle": 0, "inUse": 3,
                   "firstChoice": 5, "placed": 3},
            "b2": {"connections": 3, "idle": 1, "inUse": 2,
                   "firstChoice": 0, "placed": 2}}
        assert idle_keys(kit.pool) == ["b2"]
        await release(kit, *boxes)
        st = kit.pool.get_affinity_stats()["backends"]
        assert [st[k]["inUse"] for k in ("b1", "b2")] == [0, 0]
        assert [st[k]["idle"] for k in ("b1", "b2")] == [3, 3]
        assert kit.counter("queued-claim") == 0
        await kit.stop()
    run_vt(body)


def test_unkeyed_leases_count_towards_the_bound():
    """in use is every lease, not the keyed ones only: two plain claims
    take the head of the queue, b1 and b2; a keyed one then finds b1
    with 1 in use under a cap of ceil(1.25 * 3 / 2) = 2 and hits; the
    next finds 2 in use against ceil(1.25 * 4 / 2) = 3 and hits again;
    the last finds b1 all in use."""
    async def body(loop):
        kit = await Kit(loop, per=3, claimAffinity={}).up()
        plain = [kit.claim(), kit.claim()]
        await settle(loop)
        assert [b["key"] for b in plain] == ["b1", "b2"]
        boxes = [kit.claim(keyed(b"k0")) for _ in range(3)]
        await settle(loop)
        assert [b["key"] for b in boxes] == ["b1", "b1", "b2"]
        assert af_counters(kit) == {"claim": 3, "hit": 2, "spill-busy": 1}
        await release(kit, *(plain + boxes))
        await kit.stop()
    run_vt(body)


def test_every_idle_backend_over_the_bound_still_serves():
    """Rule 5.  loadFactor 1, three connections each, but two of b1's
    have gone and their replacements are still connecting.  b1's one
    connection and two of b2's are leased: T = 3, m = 2, the cap is
    ceil(4 / 2) = 2, and b2, the only backend with an idle slot, has 2
    in use.  A claim whose first choice is b1 gets b2's last all the
    same, and does not wait."""
    async def body(loop):
        kit = await Kit(loop, per=3, claimAffinity={"loadFactor": 1}).up()
        pool = kit.pool
        kit.auto = False
        for fsm in [f for f in pool.p_idleq
                    if f.csf_backend["key"] == "b1"][1:]:
            fsm.set_unwanted()
        await settle(loop)
        await advance(loop, 0.01)
        assert idle_keys(pool) == ["b1", "b2", "b2", "b2"]
        first = kit.claim(keyed(b"k0"))
        await settle(loop)
        assert first["key"] == "b1"
        plain = [kit.claim(), kit.claim()]
        await settle(loop)
        assert [b["key"] for b in plain] == ["b2", "b2"]
        st = pool.get_affinity_stats()["backends"]
        assert (st["b1"]["inUse"], st["b1"]["idle"]) == (1, 0)
        assert (st["b2"]["inUse"], st["b2"]["idle"]) == (2, 1)
        box = kit.claim(keyed(b"k0"))
        await settle(loop)
        assert box["key"] == "b2"
        assert af_counters(kit) == {"claim": 2, "hit": 1, "spill-busy": 1}
        assert kit.counter("queued-claim") == 0
        await release(kit, first, box, *plain)
        kit.auto = True
        for c in kit.pending:
            c.connect()
        await settle(loop)
        await kit.stop()
    run_vt(body)


# -- 3. avoidBackends ------------------------------------------------------------------

def test_avoided_backends_move_to_the_end_of_the_order():
    async def body(loop):
        kit = await Kit(loop, backends=B3, per=1, claimAffinity={}).up()
        assert kit.pool.get_affinity_order(b"k0") == ["b1", "b3", "b2"]
        assert await kit.lease(1, keyed(b"k0")) == "b1"
        assert await kit.lease(
            1, keyed(b"k0", avoidBackends=["b1"])) == "b3"
        # the first backend that is not avoided: a hit
        assert af_counters(kit) == {"claim": 2, "hit": 2}
        assert await kit.lease(
            1, keyed(b"k0", avoidBackends=["b1", "b3"])) == "b2"
        assert await kit.lease(
            1, keyed(b"k0", avoidBackends=["b3", "b2", "b1"])) == "b1"
        assert af_counters(kit) == {"claim": 4, "hit": 4}
        # avoided and busy: b3, the key's first choice now, is leased,
        # so the claim spills to b2 before it takes the avoided b1
        held = kit.claim({"avoidBackends": ["b1", "b2"]})
        await settle(loop)
        assert held["key"] == "b3"
        assert await kit.lease(
            1, keyed(b"k0", avoidBackends=["b1"])) == "b2"
        assert af_counters(kit) == {"claim": 5, "hit": 4, "spill-busy": 1}
        other = kit.claim({"avoidBackends": ["b1", "b3"]})
        await settle(loop)
        assert other["key"] == "b2"
        # only the avoided backend is idle: a preference, so it is taken
        assert await kit.lease(
            1, keyed(b"k0", avoidBackends=["b1"])) == "b1"
        assert af_counters(kit) == {"claim": 6, "hit": 4, "spill-busy": 2}
        assert kit.counter("queued-claim") == 0
        await release(kit, held, other)
        await kit.stop()
    run_vt(body)


# -- 4. nothing idle ---------------------------------------------------------------------

def test_a_keyed_claim_queues_when_nothing_is_idle():
    async def body(loop):
        kit = await Kit(loop, per=1, claimAffinity={}).up()
        a, b = kit.claim(), kit.claim()
        await settle(loop)
        assert (a["key"], b["key"]) == ("b1", "b2")
        # k0's first choice is b1; b2 frees up first and serves it
        box = kit.claim(keyed(b"k0"))
        await settle(loop)
        assert "err" not in box
        assert kit.counter("queued-claim") == 1
        assert af_counters(kit) == {"claim": 1, "queued": 1}
        assert kit.pool.get_stats()["waiterCount"] == 1
        await release(kit, b)
        assert box["err"] is None and box["key"] == "b2"
        # counted once
        assert af_counters(kit) == {"claim": 1, "queued": 1}
        st = kit.pool.get_affinity_stats()
        assert (st["claims"], st["queued"], st["hits"]) == (1, 1, 0)
        assert st["backends"]["b1"]["firstChoice"] == 1
        assert st["backends"]["b2"]["placed"] == 0

        # and it obeys its timeout
        late = kit.claim(keyed(b"k1", timeout=50))
        await settle(loop)
        assert kit.counter("queued-claim") == 2
        await advance(loop, 0.06)
        assert isinstance(late["err"], ClaimTimeoutError)
        assert kit.counter("claim-timeout") == 1
        assert kit.pool.get_stats()["waiterCount"] == 0
        assert af_counters(kit) == {"claim": 2, "queued": 2}
        await release(kit, a, box)
        await kit.stop()
    run_vt(body)


def test_error_on_empty_is_not_counted_as_queued():
    async def body(loop):
        kit = Kit(loop, per=1, claimAffinity={})
        kit.resolver_fsm.start()
        await settle(loop)
        box = kit.claim(keyed(b"k0", errorOnEmpty=True))
        await settle(loop)
        assert type(box["err"]).__name__ == "NoBackendsError"
        assert af_counters(kit) == {}
        kit.pool.stop()
        await advance(loop, 30.0)
        assert kit.pool.is_in_state("stopped")
    run_vt(body)


# -- 5. the resolver removes a backend ------------------------------------------------

def test_a_removed_backend_moves_only_its_own_keys():
    async def body(loop):
        kit = await Kit(loop, backends=B3, per=1, claimAffinity={}).up()
        pool = kit.pool
        keys = [b"k%d" % i for i in range(8)]
        before = {k: pool.get_affinity_order(k) for k in keys}
        assert before == {k: affinity_order(k, B3) for k in keys}
        assert before[b"k0"] == ["b1", "b3", "b2"]
        assert before[b"k1"] == ["b2", "b1", "b3"]
        assert before[b"k2"] == ["b3", "b2", "b1"]
        for k in keys:
            assert await kit.lease(1, keyed(k)) == before[k][0]

        kit.resolver.remove("b3")
        await settle(loop)
        await advance(loop, 0.05)
        assert sorted(set(idle_keys(pool))) == ["b1", "b2"]
        assert "b3" not in pool.p_af_hashes
        moved = 0
        for k in keys:
            now = pool.get_affinity_order(k)
            assert now == [b for b in before[k] if b != "b3"]
            got = await kit.lease(1, keyed(k))
            if before[k][0] == "b3":
                moved += 1
                assert got == before[k][1]
            else:
                assert got == before[k][0]
        assert moved == 3                       # k2, k5, k6
        assert af_counters(kit) == {"claim": 16, "hit": 16}
        assert set(pool.get_affinity_stats()["backends"]) == {"b1", "b2"}

        kit.resolver.add("b3", {"address": "10.0.0.1", "port": 80})
        await settle(loop)
        await advance(loop, 0.05)
        assert "b3" in idle_keys(pool)
        for k in keys:
            assert pool.get_affinity_order(k) == before[k]
            assert await kit.lease(1, keyed(k)) == before[k][0]
        assert af_counters(kit) == {"claim": 24, "hit": 24}
        await kit.stop()
    run_vt(body)


# -- 6. a stale entry --------------------------------------------------------------------

def test_a_stale_entry_met_on_the_walk_is_unlinked_and_skipped():
    async def body(loop):
        kit = await Kit(loop, per=2, claimAffinity={}).up()
        pool = kit.pool
        slots = list(pool.p_idleq)
        assert idle_keys(pool) == ["b1", "b2", "b1", "b2"]
        stale = slots[0]
        box = kit.claim(keyed(b"k0"))
        # the slot leaves 'idle' now; the pool hears of it a turn later
        stale.set_unwanted()
        assert not stale.is_in_state("idle")
        assert stale.p_idleq_node is not None
        await settle(loop)
        assert box["err"] is None and box["key"] == "b1"
        assert box["hdl"].ch_slot is slots[2]
        assert stale.p_idleq_node is None
        assert af_counters(kit) == {"claim": 1, "hit": 1}
        assert kit.counter("queued-claim") == 0
        await release(kit, box)
        await advance(loop, 0.05)
        await kit.stop()
    run_vt(body)


# -- 7. with claimBalancing -----------------------------------------------------------

def test_with_balancing_a_keyed_claim_lands_by_affinity():
    async def body(loop):
        kit = await Kit(loop, lb={"choices": "all"}, per=2,
                        claimAffinity={}).up()
        # teach the balancer that b2 is the slow one: it would send
        # everything to b1
        await kit.lease_on("b1", 10)
        await kit.lease_on("b2", 100)
        assert await kit.lease(10) == "b1"
        leases = {k: kit.stats(k)["leases"] for k in ("b1", "b2")}
        assert leases == {"b1": 2, "b2": 1}

        box = kit.claim(keyed(b"k1"))
        await settle(loop)
        assert box["key"] == "b2"
        # in the balancer's books from the try on
        assert kit.outstanding() == {"b1": 0, "b2": 1}
        assert box["hdl"].ch_slot not in kit.pool.p_lb_handed
        await advance(loop, 0.01)
        await release(kit, box)
        assert kit.outstanding() == {"b1": 0, "b2": 0}
        assert kit.stats("b2")["leases"] == 2
        assert kit.stats("b1")["leases"] == 2
        assert kit.pool.p_lb_handed == {}
        assert af_counters(kit) == {"claim": 1, "hit": 1}
        # not one of the balancer's choices
        balanced = kit.counter("balanced-claim")
        # a claim without a key is balanced as before
        assert await kit.lease(10) == "b1"
        assert kit.counter("balanced-claim") == balanced + 1
        assert af_counters(kit) == {"claim": 1, "hit": 1}

        # a burst: the books see each pick at once
        boxes = [kit.claim(keyed(b"k1")) for _ in range(2)]
        await settle(loop)
        assert [b["key"] for b in boxes] == ["b2", "b2"]
        assert kit.outstanding() == {"b1": 0, "b2": 2}
        await release(kit, *boxes)
        assert kit.outstanding() == {"b1": 0, "b2": 0}
        await kit.stop()
    run_vt(body)


# -- 8. with claimQueue -----------------------------------------------------------------

def test_with_a_claim_queue_priority_orders_the_keyed_waiters():
    async def body(loop):
        kit = await Kit(loop, per=1, claimAffinity={},
                        claimQueue={"priorities": 2}).up()
        assert await kit.lease(1, keyed(b"k1")) == "b2"
        a, b = kit.claim(), kit.claim()
        await settle(loop)
        low = kit.claim(keyed(b"k0", priority=1))
        await settle(loop)
        high = kit.claim(keyed(b"k0", priority=0))
        await settle(loop)
        assert kit.pool.get_queue_stats()["queued"] == [1, 1]
        assert af_counters(kit) == {"claim": 3, "hit": 1, "queued": 2}
        await release(kit, b)
        assert high.get("key") == "b2" and "err" not in low
        await release(kit, a)
        assert low["key"] == "b1"
        with pytest.raises(ValueError):
            kit.claim(keyed(b"k0", priority=2))
        await release(kit, low, high)
        await kit.stop()
    run_vt(body)


# -- 9. the gauge ------------------------------------------------------------------------

def test_the_hit_ratio_gauge():
    async def body(loop):
        kit = await Kit(loop, per=1, claimAffinity={}).up()
        pool = kit.pool
        await advance(loop, 0.5)
        # absent before the first keyed claim
        assert "cueball_pool_affinity_hit_ratio{" not in \
            pool.p_collector.collect()
        held = kit.claim(keyed(b"k0"))
        await settle(loop)
        assert await kit.lease(1, keyed(b"k0")) == "b2"
        await advance(loop, 0.5)
        lines = [ln for ln in pool.p_collector.collect().splitlines()
                 if ln.startswith("cueball_pool_affinity_hit_ratio{")]
        assert len(lines) == 1
        for name, value in pool._gauge_labels.items():
            assert '%s="%s"' % (name, value) in lines[0]
        assert 'pool="' in lines[0] and 'domain="foobar"' in lines[0]
        assert float(lines[0].rsplit(" ", 1)[1]) == 0.5
        # the key set of get_stats() is what it was
        assert set(pool.get_stats()) == {
            "counters", "totalConnections", "idleConnections",
            "pendingConnections", "waiterCount"}
        await release(kit, held)
        await kit.stop()
    run_vt(body)


