"""``claimBalancing`` on an agent, against two real localhost HTTP
servers, one of which delays every response by 30 ms: the same paced
GETs through an agent without the option and through one with it."""

import asyncio

from balance_kit import DelayServer
from retry_kit import HOST, finish, key_of, make_agent, request, run

REQUESTS = 60
PACE = 0.005
DELAY = 0.03


async def drive(agent):
    for n in range(REQUESTS):
        resp = await request(agent, "/%d" % n)
        # every request succeeds
        assert not isinstance(resp, Exception), (n, resp)
        assert resp.status_code == 200 and resp.body == b"ok"
        await asyncio.sleep(PACE)


def test_an_agent_steers_around_a_delayed_server():
    async def body():
        counts = {}
        for name, opts in (("off", {}),
                           ("on", {"claimBalancing": {"choices": "all"}})):
            fast = await DelayServer().start()
            slow = await DelayServer(delay=DELAY).start()
            agent, pool = await make_agent([fast, slow], None, **opts)
            await drive(agent)
            assert fast.served + slow.served == REQUESTS
            counts[name] = slow.served
            if name == "on":
                st = agent.get_balancing_stats(HOST)
                assert st["enabled"] is True
                lat = {k: v["latencyMs"] for k, v in st["backends"].items()}
                fast_key, slow_key = key_of(pool, fast), key_of(pool, slow)
                assert lat[slow_key] is not None and lat[fast_key] is not None
                assert lat[slow_key] > lat[fast_key]
                assert lat[slow_key] >= DELAY * 1000.0 * 0.5
                assert sum(v["leases"] for v in st["backends"].values()) \
                    == REQUESTS
                assert all(v["failedLeases"] == 0
                           for v in st["backends"].values())
                # the 5 Hz sample publishes the gauges
                await asyncio.sleep(0.25)
                text = agent.collector.collect()
                for metric in ("cueball_pool_backend_latency_seconds",
                               "cueball_pool_backend_outstanding"):
                    lines = [ln for ln in text.splitlines()
                             if ln.startswith(metric + "{")]
                    assert lines, metric
                    assert all('backend="' in ln and 'pool="' in ln and
                               'domain="%s"' % HOST in ln for ln in lines)
                    assert any('backend="%s"' % slow_key in ln
                               for ln in lines)
            else:
                assert agent.get_balancing_stats(HOST) == {"enabled": False}
                assert "cueball_pool_backend_" not in \
                    agent.collector.collect()
            await finish(agent, fast, slow)
        print("delayed server served: off %(off)d, on %(on)d" % counts)
        # round-robin over idle connections sends it about half
        assert counts["off"] >= REQUESTS // 4, counts
        assert counts["on"] < counts["off"] / 3.0, counts
    run(body())
