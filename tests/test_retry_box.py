"""Request retries over real sockets on the deployment box (run with
-m gpu).

Two loopback servers behind one agent: one answers, the other resets
every request it is sent.  200 sequential GETs, about 2 s, with
``retry`` and ``outlierDetection`` both on: every request succeeds, the
resetting backend is ejected, no retry happens while it is out, and the
retries counted are exactly the resets the server dealt.
"""

import asyncio

import pytest

from retry_kit import (HOST, ScriptServer, finish, key_of, make_agent,
                       request, run)

pytestmark = pytest.mark.gpu

REQUESTS = 200
PACE = 0.01


def test_native_runtime_in_use():
    """Retries must ride on the native claim path, not replace it."""
    from cueball_amd import _speed
    from cueball_amd import connection_fsm, fsm, pool
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert connection_fsm._SlotKit is _speed.SlotKit


def test_retries_and_ejection_over_real_sockets():
    async def body():
        loop = asyncio.get_running_loop()
        good = await ScriptServer().start()
        bad = await ScriptServer(default="reset").start()
        agent, pool = await make_agent(
            [good, bad], {"delay": 1},
            outlierDetection={"consecutiveFailures": 3,
                              "baseEjectionTime": 400})
        bad_key = key_of(pool, bad)
        events = []
        pool.on("backendEjected",
                lambda key, info: events.append(("ejected", key)))
        pool.on("backendReinstated",
                lambda key, why: events.append(("reinstated", key)))

        def out():
            return agent.get_outlier_stats()[HOST]["ejected"] > 0

        def retries():
            # no entry before the host's first request
            c = agent.get_retry_stats().get(HOST, {}).get("counters", {})
            return sum(c.get("retry-" + r, 0) for r in
                       ("reset", "timeout", "status", "claim-failure"))

        while_out = 0
        start = loop.time()
        for n in range(REQUESTS):
            was_out, n_events, n_retries = out(), len(events), retries()
            resp = await request(agent, "/%d" % n)
            # every request succeeds
            assert not isinstance(resp, Exception), (n, resp)
            assert resp.status_code == 200 and resp.body == b"ok"
            if was_out and len(events) == n_events:
                # the backend was out from claim to response
                while_out += 1
                assert retries() == n_retries, "a retry during an ejection"
            await asyncio.sleep(PACE)
        took = loop.time() - start

        counters = agent.get_retry_stats()[HOST]["counters"]
        ocount = pool.get_stats()["counters"]
        print("requests", REQUESTS, "seconds %.2f" % took, "resets",
              bad.resets, "during ejections", while_out, "events", events,
              "retry counters", counters)
        # the resetting backend got ejected, and nobody else
        assert events and events[0] == ("ejected", bad_key)
        assert all(key == bad_key for _, key in events)
        assert ocount["backend-ejected"] >= 1
        assert ocount.get("ejection-refused", 0) == 0
        assert while_out > 20
        # the good server answered every request, once
        assert len(good.paths) == REQUESTS
        assert sorted(good.paths) == sorted("/%d" % n
                                            for n in range(REQUESTS))
        # the retries counted are the resets dealt
        assert bad.resets >= 3
        assert counters["retry-reset"] == bad.resets
        assert retries() == bad.resets
        assert counters["retry-budget-exhausted"] == 0
        assert counters["retries-exhausted"] == 0
        st = agent.get_retry_stats()[HOST]
        assert st["active"] == 0 and st["retrying"] == 0
        await finish(agent, good, bad)
    run(body())
