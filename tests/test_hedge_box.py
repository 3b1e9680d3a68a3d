"""Request hedging over real sockets on the deployment box (run with
-m gpu).

Two loopback servers behind one agent with the *adaptive* hedge policy.
200 paced GETs, about 3 s: the first half runs against two healthy
servers and fills the latency window; then one server starts to hold
every request it is sent.  Every request still succeeds, the hedges won
are exactly the requests the held server was sent, and the budget never
had to refuse one.

``minDelay`` is a floor well above the jitter of a loopback request, so
that a healthy request is never hedged (its hedge would go to the held
server and lose, which is correct, and is not what is counted here);
``maxDelay`` bounds how long the test can take.
"""

import asyncio

import pytest

from hedge_kit import hedge_counters
from retry_kit import HOST, ScriptServer, finish, make_agent, request, run

pytestmark = pytest.mark.gpu

REQUESTS = 200
HEALTHY = 100
PACE = 0.01
HEDGE = {"minSamples": 20, "window": 2000, "minDelay": 20, "maxDelay": 40}


def test_native_runtime_in_use():
    """Hedging must ride on the native claim path, not replace it."""
    from cueball_amd import _speed
    from cueball_amd import connection_fsm, fsm, latency, pool
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert connection_fsm._SlotKit is _speed.SlotKit
    # and the latency window is the native histogram
    assert latency.LatencyHistogram is _speed.LatencyHistogram


def test_adaptive_hedging_beats_a_held_server_over_real_sockets():
    async def body():
        loop = asyncio.get_running_loop()
        fast = await ScriptServer().start()
        slow = await ScriptServer().start()
        release = asyncio.Event()
        agent, pool = await make_agent([fast, slow], None, hedge=HEDGE)
        mark = None
        delays = []
        start = loop.time()
        for n in range(REQUESTS):
            if n == HEALTHY:
                # the window has filled: there is an estimate
                st = agent.get_hedge_stats()[HOST]
                assert st["samples"] >= HEALTHY
                assert st["delayMs"] is not None
                assert st["counters"]["hedge-sent"] == 0
                assert st["counters"]["hedge-skipped-samples"] == \
                    HEDGE["minSamples"]
                mark = len(slow.paths)
                assert mark > 0, "the second server was never used"
                slow.default = ("hold", release)
            resp = await request(agent, "/%d" % n)
            # every request succeeds
            assert not isinstance(resp, Exception), (n, resp)
            assert resp.status_code == 200 and resp.body == b"ok"
            delays.append(agent.get_hedge_stats()[HOST]["delayMs"])
            await asyncio.sleep(PACE)
        took = loop.time() - start

        st = agent.get_hedge_stats()[HOST]
        counters = hedge_counters(agent)
        sent_held = len(slow.paths) - mark
        print("requests", REQUESTS, "seconds %.2f" % took, "held", sent_held,
              "delayMs first/last", delays[HEALTHY], delays[-1],
              "samples", st["samples"], "hedge counters", counters)
        # the held server is sent a request whenever its connection
        # heads the idle queue; each one costs it that connection, and
        # the pool takes a few requests' time to replace it
        assert sent_held >= 5
        assert counters["hedge-won"] == sent_held
        assert counters["hedge-sent"] == sent_held
        assert counters["hedge-skipped-budget"] == 0
        assert counters["hedge-lost"] == 0 and counters["hedge-failed"] == 0
        assert set(slow.paths[mark:]) <= set(fast.paths)
        assert sorted(set(fast.paths + slow.paths[:mark])) == \
            sorted("/%d" % n for n in range(REQUESTS))
        for d in delays[HEALTHY:]:
            assert HEDGE["minDelay"] <= d <= HEDGE["maxDelay"]
        assert st["active"] == 0 and st["hedging"] == 0
        release.set()
        await finish(agent, fast, slow)
    run(body())
