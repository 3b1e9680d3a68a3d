"""The ``retry`` option of an agent over real loopback sockets: two
scripted backends behind one StaticIpResolver, spares 2, maximum 4."""

import asyncio

from cueball_amd.connection_fsm import count_listeners
from cueball_amd.errors import CueballError, RequestTimeoutError
from cueball_amd.http_client import HttpParseError, HttpRequest
from cueball_amd.retry import COUNTERS, RetriedRequest
from retry_kit import (DEADLINE, HOST, ScriptServer, finish, idle_keys,
                       key_of, make_agent, quiet, request, run, served_by,
                       stop_agent, stop_servers, until)


async def pair(retry, **opts):
    a = await ScriptServer().start()
    b = await ScriptServer().start()
    agent, pool = await make_agent([a, b], retry, **opts)
    return a, b, agent, pool


async def head_and_other(pool, a, b):
    """(head, other): `head` is the server whose connection the next
    plain claim is handed; both have an idle connection."""
    await until(lambda: quiet(pool) and
                {key_of(pool, a), key_of(pool, b)} <= set(idle_keys(pool)),
                "an idle connection to each server")
    if idle_keys(pool)[0] == key_of(pool, a):
        return a, b
    return b, a


async def go(agent, path, method="GET", body=None, **kw):
    """(request object, response or error) of one agent.request()."""
    fut = asyncio.get_running_loop().create_future()

    def cb(err, resp):
        if not fut.done():
            fut.set_result(resp if err is None else err)

    req = agent.request(HOST, method, path, None, body, cb, **kw)
    return req, await asyncio.wait_for(fut, DEADLINE)


def test_a_reset_get_succeeds_on_the_other_backend():
    async def body():
        a, b, agent, pool = await pair({"delay": 1})
        bad, good = await head_and_other(pool, a, b)
        bad.default = "reset"
        events = []
        req, resp = await go(agent, "/one")
        assert isinstance(req, RetriedRequest)
        req.on("retry", lambda *args: events.append(args))
        assert resp.status_code == 200 and resp.body == b"ok"
        assert req.attempts == 2 and req.retry_reasons == ["reset"]
        # the first try met the bad one, the retry went elsewhere
        assert served_by("/one", bad, good) == [bad.port, good.port]
        assert bad.resets == 1
        st = agent.get_retry_stats()[HOST]
        assert st["active"] == 0 and st["retrying"] == 0
        assert st["counters"]["retry-reset"] == 1
        await until(lambda: quiet(pool), "the pool to settle")
        await finish(agent, a, b)
    run(body())


def test_without_avoidance_the_retry_may_meet_the_bad_backend_again():
    async def body():
        a, b, agent, pool = await pair(
            {"delay": 1, "maxRetries": 2, "avoidFailedBackends": False})
        bad, good = await head_and_other(pool, a, b)
        bad.default = "reset"
        # take the good backend's idle connection away
        held = {}
        pool.claim({"avoidBackends": [key_of(pool, bad)]},
                   lambda err, hdl=None, conn=None: held.update(
                       hdl=hdl, key=hdl.get_backend()["key"]))
        await until(lambda: held, "the good connection")
        assert held["key"] == key_of(pool, good)
        assert set(idle_keys(pool)) == {key_of(pool, bad)}
        req, res = await go(agent, "/two")
        assert 1 <= req.attempts <= 3
        assert len(served_by("/two", bad, good)) == req.attempts
        if isinstance(res, Exception):
            assert req.attempts == 3 and bad.paths.count("/two") == 3
        else:
            assert res.status_code == 200
        held["hdl"].release()
        await finish(agent, a, b)
    run(body())


def test_a_post_is_not_retried_unless_the_call_says_so():
    async def body():
        a, b, agent, pool = await pair({"delay": 1})
        bad, good = await head_and_other(pool, a, b)
        bad.default = "reset"
        req, res = await go(agent, "/post", "POST", b"payload")
        assert isinstance(req, RetriedRequest)
        assert isinstance(res, (OSError, HttpParseError)), res
        assert req.attempts == 1 and req.retry_reasons == []
        assert served_by("/post", bad, good) == [bad.port]
        assert agent.get_retry_stats()[HOST]["counters"] == \
            {c: 0 for c in COUNTERS}

        # a POST that carries an idempotency key
        bad.default, good.default = "ok", "ok"
        bad, good = await head_and_other(pool, a, b)
        bad.default = "reset"
        req, res = await go(agent, "/post2", "POST", b"payload",
                            retry={"methods": ["POST"]})
        assert res.status_code == 200
        assert req.attempts == 2 and req.retry_reasons == ["reset"]
        assert served_by("/post2", bad, good) == [bad.port, good.port]
        assert good.methods[-1] == "POST"

        # and a call that wants no driver gets none
        req, res = await go(agent, "/plain", retry=False)
        assert type(req) is HttpRequest
        await finish(agent, a, b)
    run(body())


def test_a_hung_backend_is_timed_out_and_retried_elsewhere():
    async def body():
        a, b, agent, pool = await pair({"delay": 1, "perTryTimeout": 150})
        bad, good = await head_and_other(pool, a, b)
        bad.default = "hang"
        loop = asyncio.get_running_loop()
        t0 = loop.time()
        req, resp = await go(agent, "/hung")
        took = loop.time() - t0
        assert resp.status_code == 200
        assert req.attempts == 2 and req.retry_reasons == ["timeout"]
        assert served_by("/hung", bad, good) == [bad.port, good.port]
        assert 0.14 <= took < 2.0
        counters = agent.get_retry_stats()[HOST]["counters"]
        assert counters["timeout-per-try"] == 1
        assert counters["retry-timeout"] == 1
        # the hung lease was closed, not left with the backend
        await until(lambda: bad.hung_now == 0, "the hung socket to close")
        assert bad.hangs == 1
        bad.default = "ok"
        await until(lambda: quiet(pool), "the pool to settle")
        st = pool.get_stats()
        assert st["waiterCount"] == 0
        assert st["idleConnections"] + st["pendingConnections"] == \
            st["totalConnections"]

        # with no retry left the request ends with the timeout
        bad, good = await head_and_other(pool, a, b)
        bad.default = "hang"
        req, err = await go(agent, "/hung2", retry={"maxRetries": 0})
        assert isinstance(err, RequestTimeoutError)
        assert err.kind == "per-try" and err.timeout_ms == 150
        assert req.attempts == 1
        await until(lambda: bad.hung_now == 0, "the hung socket to close")
        await finish(agent, a, b)
    run(body())


def test_per_try_timeouts_eject_a_hung_backend():
    async def body():
        a, b, agent, pool = await pair(
            {"delay": 1, "perTryTimeout": 150},
            outlierDetection={"consecutiveFailures": 2})
        bad, good = await head_and_other(pool, a, b)
        bad.default = "hang"
        ejected = []
        pool.on("backendEjected",
                lambda key, info: ejected.append((key, dict(info))))
        loop = asyncio.get_running_loop()
        end = loop.time() + DEADLINE
        n = 0
        while not ejected:
            assert loop.time() < end, "no ejection"
            resp = await request(agent, "/e%d" % n)
            assert resp.status_code == 200
            n += 1
            await asyncio.sleep(0.005)
        assert ejected[0][0] == key_of(pool, bad)
        assert ejected[0][1]["reason"] == "consecutive-failures"
        # two per-try timeouts did it
        assert bad.hangs == 2
        counters = agent.get_retry_stats()[HOST]["counters"]
        assert counters["timeout-per-try"] == 2
        assert counters["retry-timeout"] == 2
        stats = agent.get_outlier_stats()[HOST]
        assert stats["backends"][key_of(pool, bad)]["failures"] == 2
        await finish(agent, a, b)
    run(body())


def test_a_503_is_retried_and_leaves_the_connection_reusable():
    async def body():
        a, b, agent, pool = await pair(
            {"delay": 1, "maxRetries": 1, "retryOn": ["status"]})
        bad, good = await head_and_other(pool, a, b)
        conns = (bad.conn_count, good.conn_count)
        bad.script.append(("status", 503))
        req, resp = await go(agent, "/s")
        assert resp.status_code == 200
        assert req.attempts == 2 and req.retry_reasons == ["status"]
        assert served_by("/s", bad, good) == [bad.port, good.port]
        await until(lambda: quiet(pool), "the pool to settle")
        # released, not closed: nobody had to connect again
        for i in range(6):
            resp = await request(agent, "/after%d" % i)
            assert resp.status_code == 200
        await until(lambda: quiet(pool), "the pool to settle")
        assert (bad.conn_count, good.conn_count) == conns
        assert bad.paths.count("/s") == 1 and len(bad.paths) > 1

        # both answer 503 and one retry is all there is: the last
        # response is delivered, as a response
        bad.script.append(("status", 503))
        good.script.append(("status", 503))
        req, resp = await go(agent, "/s2")
        assert resp.status_code == 503 and resp.body == b"503"
        assert resp.complete and req.attempts == 2
        counters = agent.get_retry_stats()[HOST]["counters"]
        assert counters["retry-status"] == 2
        assert counters["retries-exhausted"] == 1
        # a status that is not in retryStatuses is nobody's business
        bad.script.append(("status", 500))
        good.script.append(("status", 500))
        req, resp = await go(agent, "/s3")
        assert resp.status_code == 500 and req.attempts == 1
        await until(lambda: quiet(pool), "the pool to settle")
        assert (bad.conn_count, good.conn_count) == conns
        await finish(agent, a, b)
    run(body())


def metric_line(name, value, **labels):
    """One exposition line of the agent's collector, whose every metric
    carries the static label ``component``."""
    labels.update(component="cueball", host=HOST)
    return "\n%s{%s} %d\n" % (name, ",".join(
        '%s="%s"' % kv for kv in sorted(labels.items())), value)


def test_prometheus_lines():
    async def body():
        a, b, agent, pool = await pair(
            {"delay": 1, "perTryTimeout": 150,
             "budget": {"percent": 0, "minConcurrency": 1}})
        bad, good = await head_and_other(pool, a, b)
        bad.script.append("reset")
        resp = await request(agent, "/r")
        assert resp.status_code == 200
        bad, good = await head_and_other(pool, a, b)
        bad.script.append("hang")
        resp = await request(agent, "/h")
        assert resp.status_code == 200
        text = agent.collector.collect()
        assert metric_line("cueball_agent_retries_total", 1,
                           reason="reset") in text
        assert metric_line("cueball_agent_retries_total", 1,
                           reason="timeout") in text
        assert metric_line("cueball_agent_request_timeouts_total", 1,
                           kind="per-try") in text
        assert "cueball_agent_retry_budget_exhausted_total{" not in text
        await finish(agent, a, b)

        # a budget that allows nothing, and a total timeout
        a, b, agent, pool = await pair(
            {"delay": 1, "totalTimeout": 150,
             "budget": {"percent": 0, "minConcurrency": 0}})
        bad, good = await head_and_other(pool, a, b)
        bad.script.append("reset")
        res = await request(agent, "/r")
        assert isinstance(res, Exception)
        bad, good = await head_and_other(pool, a, b)
        bad.script.append("hang")
        res = await request(agent, "/h")
        assert isinstance(res, RequestTimeoutError) and res.kind == "total"
        text = agent.collector.collect()
        assert metric_line("cueball_agent_retry_budget_exhausted_total",
                           1) in text
        assert metric_line("cueball_agent_request_timeouts_total", 1,
                           kind="total") in text
        assert "cueball_agent_retries_total{" not in text
        st = agent.get_retry_stats()[HOST]
        assert st["limit"] == 0
        assert st["counters"]["retry-budget-exhausted"] == 1
        assert st["counters"]["timeout-total"] == 1
        await finish(agent, a, b)
    run(body())


def test_agent_stop_during_a_backoff_ends_the_request():
    async def body():
        a, b, agent, pool = await pair(
            {"delay": 5000, "maxDelay": 5000, "jitter": False})
        bad, good = await head_and_other(pool, a, b)
        bad.default = "reset"
        loop = asyncio.get_running_loop()
        got = []
        retries = []
        req = agent.request(HOST, "GET", "/stop", None, None,
                            lambda err, resp: got.append((err, resp)))
        req.on("retry", lambda *args: retries.append(args))
        await until(lambda: retries, "the backoff to begin")
        assert retries == [(1, "reset", 5000)] and got == []
        assert agent.get_retry_stats()[HOST]["retrying"] == 1
        t0 = loop.time()
        await stop_agent(agent)
        assert len(got) == 1 and isinstance(got[0][0], CueballError)
        assert "stopped" in str(got[0][0]) and got[0][1] is None
        assert loop.time() - t0 < 2.0
        st = agent.get_retry_stats()[HOST]
        assert st["active"] == 0 and st["retrying"] == 0
        assert req.attempts == 1
        await stop_servers(a, b)
    run(body())


def test_abort_closes_the_lease_of_the_current_try():
    async def body():
        a, b, agent, pool = await pair({"delay": 1, "totalTimeout": 5000})
        head, other = await head_and_other(pool, a, b)
        gate = asyncio.Event()
        head.script.append(("hold", gate))
        got, aborts = [], []
        req = agent.request(HOST, "GET", "/held", None, None,
                            lambda err, resp: got.append((err, resp)))
        req.on("abort", lambda: aborts.append(1))
        await until(lambda: head.paths == ["/held"], "the request to land")
        conns = head.conn_count
        req.abort()
        assert aborts == [1] and req.aborted and req.attempts == 1
        st = agent.get_retry_stats()[HOST]
        assert st["active"] == 0 and st["retrying"] == 0
        # the connection the server still holds is closed under it
        gate.set()
        await until(lambda: quiet(pool) and head.conn_count > conns,
                    "the lease to be closed and replaced")
        await asyncio.sleep(0.02)
        assert got == [] and aborts == [1]
        resp = await request(agent, "/next")
        assert resp.status_code == 200
        await finish(agent, a, b)
    run(body())


def test_one_bad_connection_costs_one_retry():
    async def body():
        a = await ScriptServer().start()
        b = await ScriptServer().start()
        # the first connection a accepts resets whatever it is sent;
        # the ones after it are fine
        a.conn_script.append("reset")
        agent, pool = await make_agent([a, b], {"delay": 1})
        for n in range(12):
            resp = await request(agent, "/c%d" % n)
            assert resp.status_code == 200
            await until(lambda: quiet(pool), "the pool to settle")
        assert a.resets == 1 and a.conn_count >= 2
        assert a.count("ok") >= 1 and b.count("ok") >= 1
        counters = agent.get_retry_stats()[HOST]["counters"]
        assert counters["retry-reset"] == 1
        assert sum(counters.values()) == 1
        await finish(agent, a, b)
    run(body())


def test_a_thousand_requests_leave_no_listeners_behind():
    async def body():
        a, b, agent, pool = await pair({"perTryTimeout": 5000,
                                        "totalTimeout": 8000})

        def counts():
            return {id(f): [count_listeners(f.get_socket_mgr().sm_socket, e)
                            for e in ("data", "close", "error", "readable")]
                    for fsms in pool.p_connections.values() for f in fsms}

        # a first burst, so that the pool has grown to its full size
        await asyncio.gather(*[request(agent, "/warm") for i in range(50)])
        await until(lambda: quiet(pool), "the pool to settle")
        before = counts()
        assert len(before) == 4
        for batch in range(20):
            results = await asyncio.gather(*[
                request(agent, "/%d/%d" % (batch, i)) for i in range(50)])
            assert all(r.status_code == 200 for r in results)
        assert len(a.paths) + len(b.paths) == 1050
        await until(lambda: quiet(pool), "the pool to settle")
        socks = [f.get_socket_mgr().sm_socket
                 for fsms in pool.p_connections.values() for f in fsms]
        assert socks
        for sock in socks:
            # only the socket manager's own listeners remain
            assert sock.listener_count("data") == 0
            assert sock.listener_count("close") <= 1
            assert sock.listener_count("error") <= 1
            for ev in ("free", "agentRemove"):
                assert sock.listener_count(ev) == 0
        # the same sockets, and nothing on them that the claim handle's
        # leak check would count
        assert counts() == before
        st = agent.get_retry_stats()[HOST]
        assert st["active"] == 0 and st["retrying"] == 0
        assert st["counters"] == {c: 0 for c in COUNTERS}
        # nor a timer of the driver's on the loop
        loop = asyncio.get_running_loop()
        assert not [h for h in loop._scheduled
                    if not h._cancelled and "RetriedRequest" in repr(h)]
        await finish(agent, a, b)
    run(body())
