"""The retry driver (cueball_amd.retry) with scripted tries on a
VirtualLoop: backoff, limits, reasons, the commit point, timeouts,
aborts, the budget, and that nothing outlives a request."""

import pytest

from cueball_amd import utils as mod_utils
from cueball_amd.errors import (ClaimTimeoutError, CueballError,
                                NoBackendsError, PoolFailedError,
                                PoolStoppingError, RequestTimeoutError)
from cueball_amd.retry import RetriedRequest, RetryHost, RetryPolicy
from cueball_amd.testing import advance
from conftest import run_vt
from retry_kit import Tries, timers


class Rig:
    """One RetryHost, and requests on it whose tries are scripted."""

    def __init__(self, loop, **retry):
        retry.setdefault("jitter", False)
        self.loop = loop
        self.options = mod_utils.assert_retry_policy({"retry": retry})
        self.policy = RetryPolicy(self.options)
        self.host = RetryHost("svc", self.options["budget"])
        self.stopped = False

    def request(self, method="GET", rng=None, policy=None):
        tries = Tries()
        req = RetriedRequest(self.loop, policy or self.policy, self.host,
                             method, tries, lambda: self.stopped, rng)
        log = []
        req.on("response", lambda r: log.append(("response", r)))
        req.on("error", lambda e: log.append(("error", e)))
        req.on("abort", lambda: log.append(("abort",)))
        req.on("retry", lambda n, why, ms: log.append(("retry", n, why, ms)))
        req.start()
        return req, tries, log

    def counter(self, name):
        return self.host.counters.get(name, 0)

    def assert_clean(self, *all_tries):
        """After every ending: no scheduled handle, both counts 0, no
        listener of the driver's left on any try."""
        assert timers(self.loop) == []
        assert self.host.active == 0 and self.host.retrying == 0
        assert not self.host.backoffs
        for tries in all_tries:
            for t in tries.tries:
                assert t.listeners_left() == 0


def reset():
    return ConnectionResetError("connection closed before response")


def test_success_on_the_first_try():
    async def body(loop):
        rig = Rig(loop, perTryTimeout=100, totalTimeout=1000)
        req, tries, log = rig.request()
        assert rig.host.active == 1 and len(timers(loop)) == 2
        assert tries.last.avoid == ()
        resp = tries.last.claimed("b1").respond(200, complete=False)
        assert log == [("response", resp)]
        # in flight until the body is in
        assert rig.host.active == 1 and len(timers(loop)) == 2
        resp.finish()
        assert req.attempts == 1 and req.retry_reasons == []
        assert resp.listener_count("end") == 0
        rig.assert_clean(tries)
        await advance(loop, 5.0)
        assert log == [("response", resp)]
    run_vt(body)


def test_backoff_caps_are_exact_without_jitter():
    async def body(loop):
        rig = Rig(loop, maxRetries=5, delay=25, maxDelay=250, budget=None)
        req, tries, log = rig.request()
        waits = []
        for n in range(1, 6):
            t0 = loop.time()
            tries.last.claimed("b1").fail(reset())
            assert log[-1][:3] == ("retry", n, "reset")
            waits.append(log[-1][3])
            assert len(tries.tries) == n and rig.host.retrying == 1
            # not a tick early
            await advance(loop, waits[-1] / 1000.0 - 0.001)
            assert len(tries.tries) == n
            await advance(loop, 0.001)
            assert len(tries.tries) == n + 1
            assert loop.time() - t0 == pytest.approx(waits[-1] / 1000.0)
        assert waits == [25, 50, 100, 200, 250]
        tries.last.claimed("b2").respond(200)
        assert req.attempts == 6 and req.retry_reasons == ["reset"] * 5
        assert rig.counter("retry-reset") == 5
        rig.assert_clean(tries)
    run_vt(body)


def test_backoff_with_jitter_stays_within_the_caps():
    async def body(loop):
        rig = Rig(loop, maxRetries=4, delay=25, maxDelay=150, budget=None,
                  jitter=True)
        caps = [25, 50, 100, 150]
        seen = [[] for _ in caps]
        for _ in range(200):
            req, tries, log = rig.request()
            for n in range(4):
                tries.last.claimed("b1").fail(reset())
                seen[n].append(log[-1][3])
                await advance(loop, 0.2)
            tries.last.respond(200)
        for cap, waits in zip(caps, seen):
            assert len(waits) == 200
            assert all(0 <= w <= cap for w in waits)
            # uniform over the whole range, not a point
            assert min(waits) < 0.2 * cap and max(waits) > 0.8 * cap
        # the draw is the injected one
        req, tries, log = rig.request(rng=lambda: 0.5)
        tries.last.claimed("b1").fail(reset())
        assert log[-1] == ("retry", 1, "reset", 12.5)
        req.abort()
        rig.assert_clean(tries)
    run_vt(body)


def test_max_retries():
    async def body(loop):
        rig = Rig(loop, maxRetries=2, delay=10, budget=None)
        req, tries, log = rig.request()
        errs = [reset() for _ in range(3)]
        for i, e in enumerate(errs):
            tries.last.claimed("b%d" % i).fail(e)
            await advance(loop, 0.5)
        assert len(tries.tries) == 3 and req.attempts == 3
        # the last outcome, the very object
        assert log[-1] == ("error", errs[2]) and log[-1][1] is errs[2]
        assert [l[0] for l in log] == ["retry", "retry", "error"]
        assert rig.counter("retries-exhausted") == 1
        assert rig.counter("retry-reset") == 2
        # each try avoids what failed before it
        assert [t.avoid for t in tries.tries] == [(), ("b0",), ("b0", "b1")]
        rig.assert_clean(tries)

        # maxRetries 0: timeouts only
        rig0 = Rig(loop, maxRetries=0)
        req, tries, log = rig0.request()
        e = reset()
        tries.last.claimed("b1").fail(e)
        assert log == [("error", e)] and req.attempts == 1
        rig0.assert_clean(tries)
    run_vt(body)


def test_avoid_failed_backends_off():
    async def body(loop):
        rig = Rig(loop, delay=10, avoidFailedBackends=False)
        req, tries, log = rig.request()
        tries.last.claimed("b1").fail(reset())
        await advance(loop, 0.1)
        assert [t.avoid for t in tries.tries] == [(), ()]
        tries.last.claimed("b1").respond(200)
        rig.assert_clean(tries)
    run_vt(body)


def test_the_method_filter():
    async def body(loop):
        rig = Rig(loop, delay=10)
        for method in ("POST", "PATCH", "post"):
            req, tries, log = rig.request(method)
            e = reset()
            tries.last.claimed("b1").fail(e)
            assert log == [("error", e)] and req.attempts == 1
            rig.assert_clean(tries)
        assert rig.host.counters == {}
        for method in ("GET", "HEAD", "OPTIONS", "PUT", "DELETE", "get"):
            req, tries, log = rig.request(method)
            tries.last.claimed("b1").fail(reset())
            assert log[-1][:3] == ("retry", 1, "reset"), method
            req.abort()
        # a per-call policy that names POST
        over = RetryPolicy(mod_utils.override_retry_policy(
            rig.options, {"methods": ["POST"]}))
        req, tries, log = rig.request("POST", policy=over)
        tries.last.claimed("b1").fail(reset())
        assert log[-1][:3] == ("retry", 1, "reset")
        req.abort()
        # a status selected for retry is no reason for a POST either
        rig = Rig(loop, retryOn=["status"])
        req, tries, log = rig.request("POST")
        resp = tries.last.claimed("b1").respond(503, complete=False)
        assert log == [("response", resp)]      # forwarded at once
        resp.finish()
        rig.assert_clean(tries)
    run_vt(body)


def outcome(rig, kind, t):
    """Make try `t` end in `kind`; returns what a request that does not
    retry ends with."""
    if kind == "reset":
        e = reset()
        t.claimed("b1").fail(e)
        return ("error", e)
    if kind == "claim-failure":
        e = ClaimTimeoutError(None)
        t.fail(e)
        return ("error", e)
    if kind == "status":
        return ("response", t.claimed("b1").respond(503))
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["reset", "claim-failure", "status",
                                  "timeout"])
def test_each_reason_only_when_selected(kind):
    async def body(loop):
        others = [r for r in mod_utils.RETRY_REASONS if r != kind]
        # selected: retried
        rig = Rig(loop, retryOn=[kind], perTryTimeout=100, delay=10)
        req, tries, log = rig.request()
        if kind == "timeout":
            await advance(loop, 0.1)
        else:
            outcome(rig, kind, tries.last)
        assert log == [("retry", 1, kind, 10)]
        assert rig.counter("retry-" + kind) == 1
        await advance(loop, 0.01)
        assert req.attempts == 2 and req.retry_reasons == [kind]
        tries.last.claimed("b2").respond(200)
        rig.assert_clean(tries)

        # everything else selected: the outcome is the request's
        rig = Rig(loop, retryOn=others, perTryTimeout=100, delay=10)
        req, tries, log = rig.request()
        if kind == "timeout":
            await advance(loop, 0.1)
            assert log[0][0] == "error" and log[0][1].kind == "per-try"
            assert tries.last.aborted
        else:
            assert log == [outcome(rig, kind, tries.last)]
        assert len(log) == 1 and req.attempts == 1
        assert rig.counter("retry-" + kind) == 0
        assert rig.counter("retries-exhausted") == 0
        rig.assert_clean(tries)
    run_vt(body)


def test_claim_failures():
    async def body(loop):
        rig = Rig(loop, retryOn=["claim-failure"], delay=10, budget=None,
                  maxRetries=5)
        req, tries, log = rig.request()
        for n, e in enumerate((ClaimTimeoutError(None),
                               NoBackendsError(None),
                               PoolFailedError(None)), 1):
            tries.last.fail(e)
            assert log[-1] == ("retry", n, "claim-failure",
                               10 * 2 ** (n - 1))
            await advance(loop, 0.1)
        # never got a socket: nothing to avoid
        assert all(t.avoid == () for t in tries.tries)
        # a stopping pool is never retried
        e = PoolStoppingError(None)
        tries.last.fail(e)
        assert log[-1] == ("error", e)
        rig.assert_clean(tries)
        # nor is a reset when only claim failures are selected, nor a
        # claim error when the try did have a socket ("reset" then)
        req, tries, log = rig.request()
        e = ClaimTimeoutError(None)
        tries.last.claimed("b1").fail(e)
        assert log == [("error", e)]
        rig.assert_clean(tries)
    run_vt(body)


def test_a_stopped_agent_is_never_retried():
    async def body(loop):
        rig = Rig(loop, delay=10)
        req, tries, log = rig.request()
        rig.stopped = True
        e = reset()
        tries.last.claimed("b1").fail(e)
        assert log == [("error", e)]
        rig.assert_clean(tries)
        # stopped during the backoff: the next try cannot start
        rig.stopped = False
        req, tries, log = rig.request()
        tries.last.claimed("b1").fail(reset())
        boom = CueballError("CueBallAgent is stopped")
        tries.raises = boom
        await advance(loop, 0.1)
        assert log[-1] == ("error", boom)
        rig.assert_clean(tries)
        # what the first try raises is the caller's
        tries = Tries()
        tries.raises = boom
        req = RetriedRequest(loop, rig.policy, rig.host, "GET", tries)
        with pytest.raises(CueballError):
            req.start()
        rig.assert_clean(tries)
    run_vt(body)


def test_the_commit_point():
    async def body(loop):
        rig = Rig(loop, retryOn=["reset", "status", "timeout"], delay=10)
        # an error after committed headers is not retried
        req, tries, log = rig.request()
        resp = tries.last.claimed("b1").respond(200, complete=False)
        assert log == [("response", resp)]
        e = reset()
        tries.last.fail(e)
        assert log == [("response", resp), ("error", e)]
        assert req.attempts == 1 and rig.host.counters == {}
        assert resp.listener_count("end") == 0
        rig.assert_clean(tries)
        await advance(loop, 1.0)
        assert len(tries.tries) == 1

        # a status that is not selected commits too
        req, tries, log = rig.request()
        resp = tries.last.claimed("b1").respond(500, complete=False)
        assert log == [("response", resp)]
        resp.finish()
        rig.assert_clean(tries)

        # a selected status is held back until its body is in, and
        # only then retried
        req, tries, log = rig.request()
        resp = tries.last.claimed("b1").respond(503, complete=False)
        assert log == [] and rig.host.retrying == 0
        resp.finish()
        assert log == [("retry", 1, "status", 10)]
        await advance(loop, 0.01)
        assert tries.last.avoid == ("b1",)
        # an error while a held-back body streams is a reset
        resp = tries.last.claimed("b2").respond(503, complete=False)
        tries.last.fail(reset())
        assert log[-1] == ("retry", 2, "reset", 20)
        assert resp.listener_count("end") == 0
        await advance(loop, 0.02)
        ok = tries.last.claimed("b1").respond(200)
        assert log[-1] == ("response", ok)
        assert req.retry_reasons == ["status", "reset"]
        rig.assert_clean(tries)
    run_vt(body)


def test_per_try_timeout_after_the_commit_point():
    async def body(loop):
        rig = Rig(loop, perTryTimeout=100, delay=10)
        req, tries, log = rig.request()
        t = tries.last.claimed("b1")
        resp = t.respond(200, complete=False)
        await advance(loop, 0.1)
        assert [l[0] for l in log] == ["response", "error"]
        err = log[1][1]
        assert isinstance(err, RequestTimeoutError)
        assert err.kind == "per-try" and err.timeout_ms == 100
        assert t.aborted and t.try_handle.reported == [err]
        assert req.attempts == 1 and rig.counter("timeout-per-try") == 1
        assert rig.counter("retry-timeout") == 0
        rig.assert_clean(tries)
    run_vt(body)


def test_a_retriable_status_is_delivered_once_retries_are_exhausted():
    async def body(loop):
        rig = Rig(loop, retryOn=["status"], maxRetries=1, delay=10)
        req, tries, log = rig.request()
        first = tries.last.claimed("b1").respond(503)
        assert log == [("retry", 1, "status", 10)]
        await advance(loop, 0.01)
        last = tries.last.claimed("b2").respond(502, complete=False)
        assert len(log) == 1
        last.finish()
        # as a response, complete, and the last one
        assert log[1] == ("response", last) and last is not first
        assert last.complete and len(log) == 2
        assert rig.counter("retries-exhausted") == 1
        rig.assert_clean(tries)
    run_vt(body)


def test_per_try_timeout():
    async def body(loop):
        rig = Rig(loop, perTryTimeout=150, delay=10, maxRetries=1)
        req, tries, log = rig.request()
        t1 = tries.last.claimed("b1")
        await advance(loop, 0.149)
        assert log == [] and not t1.aborted
        await advance(loop, 0.001)
        assert log == [("retry", 1, "timeout", 10)]
        # reported before the abort closes the lease
        assert t1.aborted and len(t1.try_handle.reported) == 1
        assert isinstance(t1.try_handle.reported[0], RequestTimeoutError)
        await advance(loop, 0.01)
        t2 = tries.last
        assert t2.avoid == ("b1",)
        # this one times out waiting for its claim: no handle to report
        await advance(loop, 0.15)
        assert t2.aborted and t2.try_handle is None
        assert log[-1][0] == "error" and log[-1][1].kind == "per-try"
        assert rig.counter("timeout-per-try") == 2
        assert rig.counter("retry-timeout") == 1
        assert rig.counter("retries-exhausted") == 1
        rig.assert_clean(tries)

        # a handle that is no longer held is not reported on
        req, tries, log = rig.request("POST")
        t = tries.last.claimed("b1")
        t.try_handle.state = "released"
        await advance(loop, 0.15)
        assert t.try_handle.reported == [] and t.aborted
        # both timeouts apply to a method that is never retried
        assert log[-1][0] == "error" and log[-1][1].kind == "per-try"
        rig.assert_clean(tries)
    run_vt(body)


def test_total_timeout_during_a_try_and_during_a_backoff():
    async def body(loop):
        rig = Rig(loop, totalTimeout=300, delay=200, maxDelay=200)
        # during a try
        req, tries, log = rig.request()
        t = tries.last.claimed("b1")
        await advance(loop, 0.3)
        assert len(log) == 1 and log[0][0] == "error"
        err = log[0][1]
        assert isinstance(err, RequestTimeoutError)
        assert err.kind == "total" and err.timeout_ms == 300
        assert t.aborted and req.attempts == 1
        assert rig.counter("timeout-total") == 1
        rig.assert_clean(tries)

        # during a backoff
        req, tries, log = rig.request()
        await advance(loop, 0.2)
        tries.last.claimed("b1").fail(reset())
        assert log[-1][:3] == ("retry", 1, "reset")
        assert rig.host.retrying == 1
        await advance(loop, 0.1)
        assert log[-1][0] == "error" and log[-1][1].kind == "total"
        assert req.attempts == 1 and rig.counter("timeout-total") == 2
        rig.assert_clean(tries)
        await advance(loop, 1.0)
        assert len(tries.tries) == 1 and len(log) == 2

        # a POST is bound by it as well
        req, tries, log = rig.request("POST")
        await advance(loop, 0.3)
        assert log[-1][1].kind == "total" and tries.last.aborted
        rig.assert_clean(tries)
    run_vt(body)


def test_abort_during_a_try_and_during_a_backoff():
    async def body(loop):
        rig = Rig(loop, perTryTimeout=500, totalTimeout=5000, delay=100)
        req, tries, log = rig.request()
        t = tries.last.claimed("b1")
        req.abort()
        assert log == [("abort",)] and t.aborted and req.aborted
        rig.assert_clean(tries)
        # whatever the aborted try says afterwards goes nowhere
        t.fail(reset())
        req.abort()
        await advance(loop, 10.0)
        assert log == [("abort",)] and len(tries.tries) == 1

        req, tries, log = rig.request()
        tries.last.claimed("b1").fail(reset())
        assert rig.host.retrying == 1 and rig.host.backoffs == {req}
        req.abort()
        assert [l[0] for l in log] == ["retry", "abort"]
        rig.assert_clean(tries)
        await advance(loop, 10.0)
        assert len(tries.tries) == 1 and len(log) == 2

        # abort from inside a listener of the response
        req, tries, log = rig.request()
        req.on("response", lambda r: req.abort())
        resp = tries.last.claimed("b1").respond(200, complete=False)
        assert [l[0] for l in log] == ["response", "abort"]
        assert resp.listener_count("end") == 0
        rig.assert_clean(tries)
    run_vt(body)


def test_host_stop_ends_the_backoffs():
    async def body(loop):
        rig = Rig(loop, delay=100)
        in_try, tries_a, log_a = rig.request()
        in_backoff, tries_b, log_b = rig.request()
        tries_b.last.claimed("b1").fail(reset())
        err = CueballError("stopped")
        rig.host.stop(err)
        assert log_b[-1] == ("error", err) and log_a == []
        assert rig.host.active == 1 and rig.host.retrying == 0
        assert len(timers(loop)) == 0
        tries_a.last.claimed("b1").respond(200)
        rig.assert_clean(tries_a, tries_b)
    run_vt(body)


def test_the_budget():
    async def body(loop):
        rig = Rig(loop, delay=10, maxRetries=1,
                  budget={"percent": 20, "minConcurrency": 1})
        reqs = [rig.request() for _ in range(10)]
        assert rig.host.active == 10 and rig.host.limit() == 2
        errs = []
        for req, tries, log in reqs:
            errs.append(reset())
            tries.last.claimed("b1").fail(errs[-1])
        await advance(loop, 0.05)
        # exactly two are retrying, their retries held open
        retrying = [r for r in reqs if r[0].attempts == 2]
        assert len(retrying) == 2 and retrying == reqs[:2]
        assert rig.host.retrying == 2 and rig.host.active == 2
        assert rig.host.stats()["limit"] == 1
        # the other eight have ended, each with its own error
        for (req, tries, log), e in zip(reqs[2:], errs[2:]):
            assert log == [("error", e)] and req.attempts == 1
        assert rig.counter("retry-budget-exhausted") == 8
        assert rig.counter("retry-reset") == 2
        assert rig.counter("retries-exhausted") == 0
        # releasing the two completes them
        for req, tries, log in retrying:
            resp = tries.last.claimed("b2").respond(200)
            assert log[-1] == ("response", resp)
        rig.assert_clean(*[r[1] for r in reqs])
    run_vt(body)


def test_the_budget_counts_a_request_once():
    async def body(loop):
        # one slot: the request that holds it may retry again, nobody
        # else may retry meanwhile
        rig = Rig(loop, delay=10, maxRetries=3,
                  budget={"percent": 0, "minConcurrency": 1})
        req, tries, log = rig.request()
        other, otries, olog = rig.request()
        tries.last.claimed("b1").fail(reset())
        await advance(loop, 0.01)
        tries.last.claimed("b2").fail(reset())
        assert log[-1][:3] == ("retry", 2, "reset")
        assert rig.host.retrying == 1
        e = reset()
        otries.last.claimed("b1").fail(e)
        assert olog == [("error", e)]
        assert rig.counter("retry-budget-exhausted") == 1
        await advance(loop, 0.1)
        tries.last.claimed("b1").respond(200)
        rig.assert_clean(tries, otries)
        # minConcurrency 0 and percent 0: no retry at all
        none = Rig(loop, budget={"percent": 0, "minConcurrency": 0})
        r, t, l = none.request()
        t.last.claimed("b1").fail(e)
        assert l == [("error", e)]
        assert none.counter("retry-budget-exhausted") == 1
        none.assert_clean(t)
    run_vt(body)
