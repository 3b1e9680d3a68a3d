"""The hedge driver (cueball_amd.hedge.HedgedTry) with scripted tries
on a VirtualLoop: when the second attempt is sent and when it is not,
who wins, errors, the budget, aborts, the try protocol towards the
retry driver, and that nothing outlives a try."""

import pytest

from cueball_amd import utils as mod_utils
from cueball_amd.errors import RequestTimeoutError
from cueball_amd.retry import RetriedRequest, RetryHost, RetryPolicy
from cueball_amd.testing import advance
from conftest import run_vt
from hedge_kit import Rig, policy_of
from retry_kit import Tries, timers


def reset():
    return ConnectionResetError("connection closed before response")


def test_the_primary_answers_before_the_delay():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        assert rig.host.active == 1 and len(timers(loop)) == 1
        assert ht in rig.host.pending
        assert tries.last.avoid == ()
        await advance(loop, 0.019)
        resp = tries.last.claimed("b1").respond(200)
        assert log == [("response", resp)]
        assert len(tries.tries) == 1 and not tries.last.aborted
        assert (ht.hedged, ht.winner, ht.aborted) == (False, "primary", False)
        assert ht.try_backend == "b1" and ht.try_backends == ("b1",)
        # the timer is gone, not just harmless
        rig.assert_clean(tries)
        await advance(loop, 1.0)
        assert len(tries.tries) == 1 and rig.counted() == {}
        assert rig.host.samples() == 1
        assert rig.host.current.max_ms == pytest.approx(19.0)
    run_vt(body)


def test_in_flight_until_the_body_is_in():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        resp = tries.last.claimed("b1").respond(200, complete=False)
        assert log == [("response", resp)]
        assert timers(loop) == [] and rig.host.active == 1
        resp.finish()
        assert resp.listener_count("end") == 0
        rig.assert_clean(tries)

        # an error under the body surfaces as on a plain request
        ht, tries, log = rig.start()
        resp = tries.last.claimed("b1").respond(200, complete=False)
        err = reset()
        tries.last.fail(err)
        assert log == [("response", resp), ("error", err)]
        assert resp.listener_count("end") == 0
        rig.assert_clean(tries)
    run_vt(body)


def test_the_hedge_is_sent_at_exactly_the_delay():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start(avoid=("b9",))
        assert tries.last.avoid == ("b9",)
        tries.last.claimed("b1")
        await advance(loop, 0.019)
        assert len(tries.tries) == 1            # not a tick early
        await advance(loop, 0.001)
        assert len(tries.tries) == 2
        assert tries.last.avoid == ("b9", "b1")
        assert rig.idle_asked == [("b9", "b1")]
        assert log == [("hedge", 20)]
        assert ht.hedged and ht.winner is None
        assert rig.host.hedging == 1 and rig.host.active == 1
        assert rig.counted() == {"hedge-sent": 1}
        assert timers(loop) == [] and not rig.host.pending
        # at most one hedge
        await advance(loop, 1.0)
        assert len(tries.tries) == 2
        ht.abort()
        rig.assert_clean(tries)
    run_vt(body)


def test_the_hedge_wins():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        primary = tries.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = tries.last.claimed("b2")
        await advance(loop, 0.005)
        resp = hedge.respond(503)               # whatever the status
        assert log == [("hedge", 20), ("response", resp)]
        assert primary.aborted and not hedge.aborted
        assert ht.winner == "hedge" and ht.hedged and not ht.aborted
        assert ht.try_backend == "b2" and ht.try_backends == ("b1", "b2")
        assert rig.counted() == {"hedge-sent": 1, "hedge-won": 1}
        rig.assert_clean(tries)
        # the winner's own time, and the loser's as a lower bound
        assert rig.host.samples() == 2
        assert rig.host.current.min_ms == pytest.approx(5.0)
        assert rig.host.current.max_ms == pytest.approx(25.0)
        # a late answer of the loser's goes nowhere
        primary.respond(200)
        assert len(log) == 2
    run_vt(body)


def test_the_primary_wins_after_a_hedge():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        primary = tries.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = tries.last                      # not even claimed yet
        resp = primary.respond(200)
        assert log == [("hedge", 20), ("response", resp)]
        assert hedge.aborted and not primary.aborted
        assert ht.winner == "primary" and ht.hedged
        assert ht.try_backend == "b1" and ht.try_backends == ("b1",)
        assert rig.counted() == {"hedge-sent": 1, "hedge-lost": 1}
        rig.assert_clean(tries)
    run_vt(body)


def test_the_hedge_errors_and_the_primary_carries_on():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        primary = tries.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = tries.last.claimed("b2")
        hedge.fail(reset())
        assert log == [("hedge", 20)]
        assert rig.counted() == {"hedge-sent": 1, "hedge-failed": 1}
        # its place in the budget is free again; no second hedge
        assert rig.host.hedging == 0 and rig.host.active == 1
        assert hedge.listeners_left() == 0
        await advance(loop, 1.0)
        assert len(tries.tries) == 2
        resp = primary.respond(200)
        assert log[-1] == ("response", resp) and ht.winner == "primary"
        assert not primary.aborted and not hedge.aborted
        assert ht.try_backend == "b1"
        assert rig.counted() == {"hedge-sent": 1, "hedge-failed": 1}
        rig.assert_clean(tries)
    run_vt(body)


def test_the_primary_errors_and_the_hedge_carries_on():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        primary = tries.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = tries.last.claimed("b2")
        primary.fail(reset())
        assert log == [("hedge", 20)] and rig.host.hedging == 1
        resp = hedge.respond(200)
        assert log[-1] == ("response", resp) and ht.winner == "hedge"
        assert not primary.aborted
        assert rig.counted() == {"hedge-sent": 1, "hedge-won": 1}
        rig.assert_clean(tries)
    run_vt(body)


@pytest.mark.parametrize("first", ["primary", "hedge"])
def test_both_fail(first):
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        primary = tries.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = tries.last.claimed("b2")
        order = [primary, hedge] if first == "primary" else [hedge, primary]
        errs = [reset(), reset()]
        order[0].fail(errs[0])
        assert log == [("hedge", 20)]
        order[1].fail(errs[1])
        # one error, the later one
        assert log == [("hedge", 20), ("error", errs[1])]
        assert ht.winner is None
        assert ht.try_backends == ("b1", "b2")
        assert ht.try_backend == ("b2" if first == "primary" else "b1")
        want = {"hedge-sent": 1}
        if first == "hedge":
            want["hedge-failed"] = 1
        assert rig.counted() == want
        rig.assert_clean(tries)
    run_vt(body)


def test_the_primary_errors_before_the_delay():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        err = reset()
        await advance(loop, 0.010)
        tries.last.claimed("b1").fail(err)
        assert log == [("error", err)]          # at once
        assert ht.try_backend == "b1" and not ht.hedged
        rig.assert_clean(tries)
        await advance(loop, 1.0)
        assert len(tries.tries) == 1 and rig.counted() == {}
        assert rig.host.samples() == 0
    run_vt(body)


def test_start_try_raising_is_raised_to_the_caller():
    async def body(loop):
        rig = Rig(loop, delay=20)
        tries = Tries()
        tries.raises = ValueError("no")
        from cueball_amd.hedge import HedgedTry
        ht = HedgedTry(loop, rig.policy, rig.host, "GET", tries)
        with pytest.raises(ValueError):
            ht.start()
        rig.assert_clean(tries)
    run_vt(body)


def test_an_unclaimed_primary_is_not_hedged():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        await advance(loop, 0.020)
        assert len(tries.tries) == 1 and log == []
        assert rig.counted() == {"hedge-skipped-unclaimed": 1}
        assert timers(loop) == [] and rig.idle_asked == []
        # and carries on as a plain try
        resp = tries.last.claimed("b1").respond(200)
        assert log == [("response", resp)] and not ht.hedged
        rig.assert_clean(tries)
    run_vt(body)


def test_no_idle_connection_elsewhere_means_no_hedge():
    async def body(loop):
        rig = Rig(loop, delay=20)
        rig.idle = False
        ht, tries, log = rig.start()
        tries.last.claimed("b1")
        await advance(loop, 0.020)
        assert len(tries.tries) == 1 and log == []
        assert rig.idle_asked == [("b1",)]
        assert rig.counted() == {"hedge-skipped-no-idle": 1}
        assert rig.host.hedging == 0
        resp = tries.last.respond(200)
        assert log == [("response", resp)]
        rig.assert_clean(tries)
    run_vt(body)


def test_a_stopped_agent_sends_no_hedge_and_counts_nothing():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        tries.last.claimed("b1")
        rig.stopped = True
        await advance(loop, 0.020)
        assert len(tries.tries) == 1 and rig.counted() == {}
        tries.last.respond(200)
        rig.assert_clean(tries)

        # HedgeHost.stop() takes the armed timers away
        rig.stopped = False
        ht, tries, log = rig.start()
        tries.last.claimed("b1")
        assert len(timers(loop)) == 1
        rig.host.stop()
        assert timers(loop) == [] and not rig.host.pending
        await advance(loop, 1.0)
        assert len(tries.tries) == 1
        tries.last.respond(200)
        rig.assert_clean(tries)
    run_vt(body)


def test_adaptive_without_samples_arms_no_timer():
    async def body(loop):
        rig = Rig(loop, minSamples=3)
        ht, tries, log = rig.start()
        assert timers(loop) == [] and not rig.host.pending
        assert rig.counted() == {"hedge-skipped-samples": 1}
        tries.last.claimed("b1")
        await advance(loop, 0.004)
        tries.last.respond(200)
        rig.assert_clean(tries)
        assert rig.host.samples() == 1
    run_vt(body)


def test_adaptive_with_samples_uses_the_estimate():
    async def body(loop):
        rig = Rig(loop, minSamples=3, percentile=50, budget=None)
        for ms in (40, 40, 40):
            rig.host.record(ms)
        ht, tries, log = rig.start()
        tries.last.claimed("b1")
        assert len(timers(loop)) == 1
        await advance(loop, 0.039)
        assert len(tries.tries) == 1
        await advance(loop, 0.001)
        assert len(tries.tries) == 2 and log == [("hedge", 40)]
        # a per-call policy: its own percentile and clamp, same window
        ht2, tries2, log2 = rig.start(policy=policy_of(maxDelay=10))
        tries2.last.claimed("b1")
        await advance(loop, 0.010)
        assert log2 == [("hedge", 10)]
        for t in (ht, ht2):
            t.abort()
        rig.assert_clean(tries, tries2)
    run_vt(body)


def test_the_budget():
    async def body(loop):
        rig = Rig(loop, delay=20,
                  budget={"percent": 20, "minConcurrency": 0})
        started = [rig.start() for _ in range(10)]
        for ht, tries, log in started:
            tries.last.claimed("b1")
        assert rig.host.active == 10 and rig.host.limit() == 2
        await advance(loop, 0.020)
        sent = [len(tries.tries) - 1 for ht, tries, log in started]
        assert sorted(sent) == [0] * 8 + [1, 1]
        assert rig.host.hedging == 2
        assert rig.counted() == {"hedge-sent": 2, "hedge-skipped-budget": 8}
        for ht, tries, log in started:
            tries.tries[0].respond(200)
        assert rig.counter("hedge-lost") == 2
        # both counts return to 0
        rig.assert_clean(*[tries for ht, tries, log in started])
    run_vt(body)


def test_no_budget_means_no_limit():
    async def body(loop):
        rig = Rig(loop, delay=20, budget=None)
        started = [rig.start() for _ in range(5)]
        for ht, tries, log in started:
            tries.last.claimed("b1")
        await advance(loop, 0.020)
        assert rig.host.hedging == 5 and rig.host.limit() is None
        for ht, tries, log in started:
            ht.abort()
        rig.assert_clean(*[tries for ht, tries, log in started])
    run_vt(body)


def test_post_is_not_hedged():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start(method="post")
        assert timers(loop) == [] and rig.host.active == 1
        tries.last.claimed("b1")
        await advance(loop, 1.0)
        assert len(tries.tries) == 1 and rig.counted() == {}
        resp = tries.last.respond(200)
        assert log == [("response", resp)]
        rig.assert_clean(tries)
        # unless the call's policy says so
        ht, tries, log = rig.start(
            method="POST", policy=policy_of(delay=20, methods=["POST"]))
        tries.last.claimed("b1")
        await advance(loop, 0.020)
        assert len(tries.tries) == 2
        ht.abort()
        rig.assert_clean(tries)
    run_vt(body)


def test_abort_aborts_both_and_emits_abort_once():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        primary = tries.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = tries.last.claimed("b2")
        ht.abort()
        ht.abort()
        assert log == [("hedge", 20), ("abort",)]
        assert primary.aborted and hedge.aborted and ht.aborted
        assert ht.winner is None
        rig.assert_clean(tries)
        # nothing further
        primary.respond(200)
        hedge.fail(reset())
        assert len(log) == 2
        # loser's samples are for races that were decided
        assert rig.host.samples() == 0

        # before the delay: the timer goes too
        ht, tries, log = rig.start()
        ht.abort()
        assert log == [("abort",)] and tries.last.aborted
        rig.assert_clean(tries)
        # after the end: a no-op
        ht, tries, log = rig.start()
        tries.last.claimed("b1").respond(200)
        ht.abort()
        assert len(log) == 1 and not ht.aborted and not tries.last.aborted
    run_vt(body)


def test_the_try_handle_proxy_reports_to_the_claimed_handles_only():
    async def body(loop):
        rig = Rig(loop, delay=20)
        ht, tries, log = rig.start()
        assert ht.try_handle is None and ht.try_backend is None
        assert ht.try_backends == ()
        primary = tries.last.claimed("b1")
        assert ht.try_handle.is_in_state("claimed")
        await advance(loop, 0.020)
        hedge = tries.last
        err = RequestTimeoutError("per-try", 100)
        # the hedge still waits for its claim
        ht.try_handle.report_failure(err)
        assert primary.try_handle.reported == [err]
        hedge.claimed("b2")
        ht.try_handle.report_failure(err)
        assert primary.try_handle.reported == [err, err]
        assert hedge.try_handle.reported == [err]
        # a handle that was released or closed is left alone
        primary.try_handle.state = "released"
        assert ht.try_handle.is_in_state("claimed")
        assert ht.try_handle.is_in_state("released")
        ht.try_handle.report_failure(err)
        assert len(primary.try_handle.reported) == 2
        assert len(hedge.try_handle.reported) == 2
        hedge.try_handle.state = "closed"
        assert not ht.try_handle.is_in_state("claimed")
        ht.try_handle.report_failure(err)       # nobody left: no error
        assert len(hedge.try_handle.reported) == 2
        ht.abort()
        rig.assert_clean(tries)
    run_vt(body)


# -- under the retry driver ---------------------------------------------------

class Nested:
    """A RetriedRequest whose every try is a HedgedTry over scripted
    attempts."""

    def __init__(self, loop, rig, **retry):
        retry.setdefault("jitter", False)
        options = mod_utils.assert_retry_policy({"retry": retry})
        self.rhost = RetryHost("svc", options["budget"])
        self.attempts = Tries()
        self.hedged = []

        def start_try(avoid):
            from cueball_amd.hedge import HedgedTry
            ht = HedgedTry(loop, rig.policy, rig.host, "GET", self.attempts,
                           avoid, rig.has_idle)
            self.hedged.append(ht)
            return ht.start()

        self.req = RetriedRequest(loop, RetryPolicy(options), self.rhost,
                                  "GET", start_try)
        self.log = []
        self.req.on("response", lambda r: self.log.append(("response", r)))
        self.req.on("error", lambda e: self.log.append(("error", e)))
        self.req.start()


def test_a_failed_hedged_try_is_retried_avoiding_both_backends():
    async def body(loop):
        rig = Rig(loop, delay=20)
        n = Nested(loop, rig, delay=10)
        primary = n.attempts.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = n.attempts.last.claimed("b2")
        hedge.fail(reset())
        assert n.req.attempts == 1              # the primary is still out
        primary.fail(reset())
        assert n.req.retry_reasons == ["reset"]
        await advance(loop, 0.010)
        assert n.req.attempts == 2 and len(n.hedged) == 2
        assert n.attempts.last.avoid == ("b1", "b2")
        resp = n.attempts.last.claimed("b3").respond(200)
        assert n.log == [("response", resp)]
        assert rig.counted() == {"hedge-sent": 1, "hedge-failed": 1}
        rig.assert_clean(n.attempts)
        assert n.rhost.active == 0 and n.rhost.retrying == 0
        for ht in n.hedged:
            assert ht.listener_count("response") == 0
            assert ht.listener_count("error") == 0
    run_vt(body)


def test_a_per_try_timeout_reports_and_aborts_both_attempts():
    async def body(loop):
        rig = Rig(loop, delay=20)
        n = Nested(loop, rig, perTryTimeout=100, maxRetries=0)
        primary = n.attempts.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = n.attempts.last.claimed("b2")
        await advance(loop, 0.080)
        assert len(n.log) == 1 and n.log[0][0] == "error"
        err = n.log[0][1]
        assert isinstance(err, RequestTimeoutError)
        assert primary.try_handle.reported == [err]
        assert hedge.try_handle.reported == [err]
        assert primary.aborted and hedge.aborted and n.hedged[0].aborted
        rig.assert_clean(n.attempts)
        assert n.rhost.active == 0
    run_vt(body)


def test_a_selected_status_from_the_winner_goes_through_the_retry_driver():
    async def body(loop):
        rig = Rig(loop, delay=20)
        n = Nested(loop, rig, delay=10, retryOn=["status"])
        primary = n.attempts.last.claimed("b1")
        await advance(loop, 0.020)
        hedge = n.attempts.last.claimed("b2")
        hedge.respond(503)
        assert primary.aborted and n.log == []
        assert n.req.retry_reasons == ["status"]
        await advance(loop, 0.010)
        assert n.attempts.last.avoid == ("b1", "b2")
        resp = n.attempts.last.claimed("b3").respond(200)
        assert n.log == [("response", resp)]
        rig.assert_clean(n.attempts)
    run_vt(body)
