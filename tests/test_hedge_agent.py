"""The ``hedge`` option of an agent over real loopback sockets: scripted
backends behind one StaticIpResolver.  Every wait is an ``until`` with
a deadline; nothing here asserts on how long anything took."""

import asyncio

from cueball_amd.errors import RequestTimeoutError
from cueball_amd.hedge import COUNTERS, HedgedTry
from cueball_amd.http_client import HttpRequest
from cueball_amd.retry import RetriedRequest
from hedge_kit import hedge_counters, held_server
from retry_kit import (DEADLINE, HOST, ScriptServer, finish, idle_keys,
                       key_of, make_agent, quiet, request, run, served_by,
                       stop_servers, until)
from test_retry_agent import go


async def slow_and_fast(hedge, retry=None, **opts):
    """(held, fast, release, agent, pool): one server that holds every
    request until `release` is set, one that answers."""
    held, release = await held_server()
    fast = await ScriptServer().start()
    agent, pool = await make_agent([held, fast], retry, hedge=hedge, **opts)
    return held, fast, release, agent, pool


async def all_idle(pool, *servers):
    await until(lambda: quiet(pool) and
                {key_of(pool, s) for s in servers} <= set(idle_keys(pool)),
                "an idle connection to each server")


def test_a_slow_server_is_beaten():
    async def body():
        held, fast, release, agent, pool = await slow_and_fast({"delay": 20})
        conns_before = held.conn_count
        hedges = []
        paths = ["/%d" % n for n in range(40)]
        for path in paths:
            req, resp = await go(agent, path)
            assert isinstance(req, HedgedTry)
            assert not isinstance(resp, Exception), (path, resp)
            assert resp.status_code == 200 and resp.body == b"ok"
            if req.hedged:
                hedges.append(path)
                assert req.winner == "hedge"
                assert len(req.try_backends) == 2
            # the next request finds a connection to each again
            await all_idle(pool, held, fast)
        # whatever the held server was sent, the fast one was sent too
        assert held.paths, "the held server was never the first choice"
        assert set(held.paths) <= set(fast.paths)
        assert sorted(set(fast.paths)) == sorted(paths)
        counters = hedge_counters(agent)
        assert counters["hedge-sent"] == len(held.paths)
        assert counters["hedge-won"] == len(held.paths)
        assert sorted(hedges) == sorted(held.paths)
        assert counters["hedge-lost"] == counters["hedge-failed"] == 0
        # a loser's connection is closed, and the pool replaces it
        assert held.conn_count >= conns_before + len(held.paths)
        st = agent.get_hedge_stats()[HOST]
        assert st["active"] == 0 and st["hedging"] == 0
        assert st["delayMs"] == 20 and st["limit"] == 1
        # every winner's sample and every loser's
        assert st["samples"] == len(paths) + len(held.paths)
        assert not agent.cba_hedge_hosts[HOST].pending
        await until(lambda: quiet(pool), "the pool to settle")

        text = agent.collector.collect()
        assert "# TYPE cueball_agent_hedges_total counter" in text
        assert "# TYPE cueball_agent_hedge_delay_seconds gauge" in text
        lines = text.splitlines()
        for outcome in ("sent", "won"):
            want = 'host="%s",outcome="%s"} %d' % (HOST, outcome,
                                                  len(held.paths))
            assert [ln for ln in lines if ln.startswith(
                "cueball_agent_hedges_total{") and ln.endswith(want)], want
        assert [ln for ln in lines if ln.startswith(
            "cueball_agent_hedge_delay_seconds{") and ln.endswith(" 0.02")]
        release.set()
        await finish(agent, held, fast)
    run(body())


def test_no_gratuitous_hedges():
    async def body():
        a = await ScriptServer().start()
        b = await ScriptServer().start()
        agent, pool = await make_agent([a, b], None, hedge={"delay": 10000})
        paths = ["/%d" % n for n in range(40)]
        for path in paths:
            resp = await request(agent, path)
            assert resp.status_code == 200
            assert not agent.cba_hedge_hosts[HOST].pending
        # every path was served exactly once
        assert sorted(a.paths + b.paths) == sorted(paths)
        counters = hedge_counters(agent)
        assert counters == dict.fromkeys(COUNTERS, 0)
        st = agent.get_hedge_stats()[HOST]
        assert st["active"] == 0 and st["hedging"] == 0
        assert st["samples"] == len(paths)
        await finish(agent, a, b)
    run(body())


def test_with_retry_a_failed_hedged_try_avoids_both_backends():
    async def body():
        servers = [await ScriptServer().start() for _ in range(3)]
        agent, pool = await make_agent(
            servers, {"delay": 1}, hedge={"delay": 20}, spares=3, maximum=6)
        await all_idle(pool, *servers)
        # roles by the idle queue: its head serves the primary, the
        # next one the hedge
        by_key = {key_of(pool, s): s for s in servers}
        slow, bad, good = [by_key[k] for k in idle_keys(pool)[:3]]
        release = asyncio.Event()
        slow.default = ("hold", release)
        bad.default = "reset"

        fut = asyncio.get_running_loop().create_future()
        req = agent.request(HOST, "GET", "/c", None, None,
                            lambda err, resp: fut.set_result(err or resp))
        assert isinstance(req, RetriedRequest)
        await until(lambda: hedge_counters(agent)["hedge-failed"] == 1,
                    "the hedge to be reset")
        assert req.attempts == 1 and not fut.done()
        assert served_by("/c", slow, bad, good) == [slow.port, bad.port]
        # now the primary fails as well: the held server hangs up
        for w in list(slow._writers):
            w.close()
        resp = await asyncio.wait_for(fut, DEADLINE)
        assert not isinstance(resp, Exception), resp
        assert resp.status_code == 200
        assert req.attempts == 2 and req.retry_reasons == ["reset"]
        # the retry avoided both backends of the failed try
        assert served_by("/c", slow, bad, good) == \
            [slow.port, bad.port, good.port]
        rst = agent.get_retry_stats()[HOST]
        assert rst["counters"]["retry-reset"] == 1
        assert rst["active"] == 0 and rst["retrying"] == 0
        counters = hedge_counters(agent)
        assert counters["hedge-sent"] == 1 and counters["hedge-failed"] == 1
        st = agent.get_hedge_stats()[HOST]
        assert st["active"] == 0 and st["hedging"] == 0
        release.set()
        await finish(agent, *servers)
    run(body())


def test_a_per_try_timeout_with_both_attempts_hung():
    async def body():
        a = await ScriptServer(default="hang").start()
        b = await ScriptServer(default="hang").start()
        agent, pool = await make_agent(
            [a, b], {"perTryTimeout": 150, "maxRetries": 0},
            hedge={"delay": 20}, outlierDetection={})
        await all_idle(pool, a, b)
        errors = []
        req = agent.request(HOST, "GET", "/hung")
        req.on("error", errors.append)
        req.on("response", errors.append)
        await until(lambda: errors, "the timeout")
        # one error, and it is the timeout
        assert len(errors) == 1
        assert isinstance(errors[0], RequestTimeoutError)
        assert errors[0].kind == "per-try"
        # both servers saw the request
        assert served_by("/hung", a, b) == [a.port, b.port]
        assert hedge_counters(agent)["hedge-sent"] == 1
        # and both hung backends were reported to outlier detection
        stats = agent.get_outlier_stats()[HOST]["backends"]
        for s in (a, b):
            assert stats[key_of(pool, s)]["failures"] == 1, stats
            assert stats[key_of(pool, s)]["consecutiveFailures"] == 1
        # both leases were closed
        await until(lambda: a.hung_now == 0 and b.hung_now == 0,
                    "the hung sockets to close")
        await asyncio.sleep(0)
        assert len(errors) == 1
        st = agent.get_hedge_stats()[HOST]
        assert st["active"] == 0 and st["hedging"] == 0
        assert agent.get_retry_stats()[HOST]["active"] == 0
        await finish(agent, a, b)
    run(body())


def test_losing_attempts_are_neutral_for_outlier_detection():
    async def body():
        held, fast, release, agent, pool = await slow_and_fast(
            {"delay": 20}, outlierDetection={})
        loop = asyncio.get_running_loop()
        end = loop.time() + DEADLINE
        n = 0
        while hedge_counters(agent)["hedge-won"] < 10:
            assert loop.time() < end, "no ten hedges"
            resp = await request(agent, "/n%d" % n)
            assert resp.status_code == 200
            n += 1
            await all_idle(pool, held, fast)
        assert len(held.paths) == 10
        rec = agent.get_outlier_stats()[HOST]["backends"][key_of(pool, held)]
        assert rec["consecutiveFailures"] == 0 and rec["failures"] == 0
        assert not rec["ejected"]
        assert agent.get_outlier_stats()[HOST]["ejected"] == 0
        release.set()
        await finish(agent, held, fast)
    run(body())


def test_hedge_false_per_call_is_a_plain_request():
    async def body():
        a = await ScriptServer().start()
        b = await ScriptServer().start()
        agent, pool = await make_agent([a, b], None, hedge={"delay": 20})
        req, resp = await go(agent, "/plain", hedge=False)
        assert type(req) is HttpRequest and resp.status_code == 200
        resp = await request(agent, "/plain2", hedge=False)
        assert resp.status_code == 200
        # the driver never saw them
        assert agent.get_hedge_stats() == {}
        # a mapping overrides the agent's policy for one call
        req, resp = await go(agent, "/post", "POST", b"x",
                             hedge={"methods": ["POST"], "delay": 10000})
        assert isinstance(req, HedgedTry) and resp.status_code == 200
        assert req._hedgeable and not req.hedged
        req, resp = await go(agent, "/post2", "POST", b"x")
        assert isinstance(req, HedgedTry) and not req._hedgeable
        assert hedge_counters(agent) == dict.fromkeys(COUNTERS, 0)
        # with retry also on, hedge=False leaves the retry driver alone
        await finish(agent, a, b)

        a = await ScriptServer().start()
        agent, pool = await make_agent([a], {}, hedge={"delay": 20})
        req, resp = await go(agent, "/r", hedge=False)
        assert isinstance(req, RetriedRequest) and resp.status_code == 200
        assert agent.get_hedge_stats() == {}
        req, resp = await go(agent, "/h", retry=False)
        assert isinstance(req, HedgedTry) and resp.status_code == 200
        req, resp = await go(agent, "/n", retry=False, hedge=False)
        assert type(req) is HttpRequest and resp.status_code == 200
        await finish(agent, a)
    run(body())


def test_agent_stop_with_a_hedge_timer_pending():
    async def body():
        held, fast, release, agent, pool = await slow_and_fast(
            {"delay": 10000})
        await all_idle(pool, held, fast)
        hhosts = agent.cba_hedge_hosts
        done = []
        reqs = []
        n = 0
        # until one request sits on the held server, its timer armed
        while not held.paths:
            req = agent.request(HOST, "GET", "/s%d" % n, None, None,
                                lambda err, resp: done.append(err or resp))
            reqs.append(req)
            n += 1
            await until(lambda: len(held.paths) + len(done) == n,
                        "the request to arrive")
        waiting = reqs[-1]
        assert waiting._timer is not None
        assert hhosts[HOST].pending == {waiting}

        loop = asyncio.get_running_loop()
        stopped = loop.create_future()
        agent.stop(lambda err: stopped.set_result(err))
        # gone at once, not when it would have fired
        assert waiting._timer is None and not hhosts[HOST].pending
        assert not [h for h in loop._scheduled if not h._cancelled and
                    getattr(h._callback, "__self__", None) is waiting]
        # the request itself is the pool's to wait for, as ever
        release.set()
        await asyncio.wait_for(stopped, DEADLINE)
        assert len(done) == n and done[-1].status_code == 200
        assert not waiting.hedged
        st = agent.get_hedge_stats()[HOST]
        assert st["active"] == 0 and st["hedging"] == 0
        await stop_servers(held, fast)
    run(body())
