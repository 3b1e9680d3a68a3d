"""The ``retry`` option: defaults, rejections, the per-call override
rules, and inertness without it."""

import gc
import math

import pytest

import cueball_amd
from cueball_amd import utils as mod_utils
from cueball_amd.agent import HttpAgent, HttpsAgent
from cueball_amd.errors import CueballError, RequestTimeoutError
from cueball_amd.http_client import HttpRequest
from cueball_amd.retry import COUNTERS, RetriedRequest, RetryPolicy
from cueball_amd.testing import DummyResolver, VirtualLoop, settle
from conftest import run_vt

RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}

DEFAULTS = {
    "maxRetries": 2,
    "retryOn": ["reset", "timeout"],
    "retryStatuses": [502, 503, 504],
    "methods": ["GET", "HEAD", "OPTIONS", "PUT", "DELETE"],
    "perTryTimeout": None,
    "totalTimeout": None,
    "delay": 25,
    "maxDelay": 250,
    "jitter": True,
    "avoidFailedBackends": True,
    "budget": {"percent": 20, "minConcurrency": 3},
}


def policy(retry):
    return mod_utils.assert_retry_policy({"retry": retry})


def test_every_default():
    assert policy({}) == DEFAULTS
    assert mod_utils.assert_retry_policy({}) is None
    assert mod_utils.assert_retry_policy({"retry": None}) is None
    # a None value is the default of its key
    assert policy({k: None for k in DEFAULTS if k != "budget"}) == DEFAULTS
    assert policy({"budget": {}})["budget"] == DEFAULTS["budget"]
    assert policy({"budget": {"percent": 50}})["budget"] == \
        {"percent": 50, "minConcurrency": 3}


def test_values_are_kept():
    got = policy({
        "maxRetries": 0, "retryOn": ("status", "claim-failure", "status"),
        "retryStatuses": {429}, "methods": ["post", "Get"],
        "perTryTimeout": 150, "totalTimeout": 1000.5, "delay": 0,
        "maxDelay": 0, "jitter": False, "avoidFailedBackends": False,
        "budget": None})
    assert got == {
        "maxRetries": 0, "retryOn": ["status", "claim-failure"],
        "retryStatuses": [429], "methods": ["POST", "GET"],
        "perTryTimeout": 150, "totalTimeout": 1000.5, "delay": 0,
        "maxDelay": 0, "jitter": False, "avoidFailedBackends": False,
        "budget": None}
    # maxDelay follows a long delay
    assert policy({"delay": 400})["maxDelay"] == 400
    assert policy({"budget": {"percent": 0, "minConcurrency": 0}}
                  )["budget"] == {"percent": 0, "minConcurrency": 0}


@pytest.mark.parametrize("retry,exc", [
    (True, TypeError), ([], TypeError), ("on", TypeError), (3, TypeError),
    ({"maxRetries": 1.0}, TypeError), ({"maxRetries": True}, TypeError),
    ({"maxRetries": "2"}, TypeError), ({"maxRetries": -1}, ValueError),
    ({"retryOn": "reset"}, TypeError), ({"retryOn": 5}, TypeError),
    ({"retryOn": {"reset": True}}, TypeError),
    ({"retryOn": [5]}, TypeError), ({"retryOn": ["resets"]}, ValueError),
    ({"retryOn": ["reset", "5xx"]}, ValueError),
    ({"retryStatuses": 503}, TypeError),
    ({"retryStatuses": "503"}, TypeError),
    ({"retryStatuses": ["503"]}, TypeError),
    ({"retryStatuses": [503.0]}, TypeError),
    ({"retryStatuses": [True]}, TypeError),
    ({"retryStatuses": [99]}, ValueError),
    ({"retryStatuses": [600]}, ValueError),
    ({"methods": "GET"}, TypeError), ({"methods": [1]}, TypeError),
    ({"methods": [""]}, ValueError),
    ({"perTryTimeout": "1"}, TypeError), ({"perTryTimeout": True}, TypeError),
    ({"perTryTimeout": 0}, ValueError), ({"perTryTimeout": -5}, ValueError),
    ({"perTryTimeout": math.inf}, ValueError),
    ({"perTryTimeout": math.nan}, ValueError),
    ({"totalTimeout": "1"}, TypeError), ({"totalTimeout": 0}, ValueError),
    ({"totalTimeout": math.inf}, ValueError),
    ({"delay": "25"}, TypeError), ({"delay": -1}, ValueError),
    ({"delay": math.inf}, ValueError),
    ({"maxDelay": "250"}, TypeError), ({"maxDelay": 10}, ValueError),
    ({"maxDelay": math.inf}, ValueError),
    ({"delay": 100, "maxDelay": 50}, ValueError),
    ({"jitter": 1}, TypeError), ({"jitter": "no"}, TypeError),
    ({"avoidFailedBackends": 0}, TypeError),
    ({"budget": 20}, TypeError), ({"budget": False}, TypeError),
    ({"budget": [20, 3]}, TypeError),
    ({"budget": {"percent": "20"}}, TypeError),
    ({"budget": {"percent": True}}, TypeError),
    ({"budget": {"percent": -1}}, ValueError),
    ({"budget": {"percent": 101}}, ValueError),
    ({"budget": {"percent": math.nan}}, ValueError),
    ({"budget": {"minConcurrency": 1.5}}, TypeError),
    ({"budget": {"minConcurrency": True}}, TypeError),
    ({"budget": {"minConcurrency": -1}}, ValueError),
])
def test_every_rejection(retry, exc):
    with pytest.raises(exc):
        policy(retry)
    # and at construction, for either agent
    loop = VirtualLoop()
    try:
        for cls in (HttpAgent, HttpsAgent):
            with pytest.raises(exc):
                cls({"recovery": RECOVERY, "spares": 1, "maximum": 2,
                     "loop": loop, "retry": retry})
    finally:
        loop.close()


def test_unknown_keys():
    with pytest.raises(ValueError, match="unknown keys.*maxRetry"):
        policy({"maxRetry": 2})
    with pytest.raises(ValueError, match="unknown keys.*perTryTimeoutMs"):
        policy({"maxRetries": 2, "perTryTimeoutMs": 5})
    with pytest.raises(ValueError, match="budget has unknown keys"):
        policy({"budget": {"percent": 20, "ttl": 10}})
    loop = VirtualLoop()
    try:
        with pytest.raises(ValueError, match="unknown keys"):
            HttpAgent({"recovery": RECOVERY, "spares": 1, "maximum": 2,
                       "loop": loop, "retry": {"retries": 2}})
    finally:
        loop.close()


def test_per_call_override_rules():
    base = policy({"maxRetries": 4, "perTryTimeout": 100})
    got = mod_utils.override_retry_policy(base, {"methods": ["POST"],
                                                 "maxRetries": 1})
    assert got == dict(base, methods=["POST"], maxRetries=1)
    assert base["maxRetries"] == 4 and "POST" not in base["methods"]
    # the empty mapping is the agent's policy
    assert mod_utils.override_retry_policy(base, {}) == base
    # everything but the budget, which all requests to a host share
    for k, v in (("retryOn", ["status"]), ("retryStatuses", [500]),
                 ("perTryTimeout", 5), ("totalTimeout", 50), ("delay", 1),
                 ("maxDelay", 300), ("jitter", False),
                 ("avoidFailedBackends", False)):
        assert mod_utils.override_retry_policy(base, {k: v})[k] == v
    with pytest.raises(ValueError, match="budget"):
        mod_utils.override_retry_policy(base, {"budget": None})
    with pytest.raises(ValueError, match="budget"):
        mod_utils.override_retry_policy(base, {"budget": {"percent": 100}})
    # validated like the option itself
    with pytest.raises(ValueError, match="unknown keys"):
        mod_utils.override_retry_policy(base, {"method": ["POST"]})
    with pytest.raises(TypeError):
        mod_utils.override_retry_policy(base, {"maxRetries": "1"})
    with pytest.raises(ValueError):
        mod_utils.override_retry_policy(base, {"maxDelay": 1})
    for bad in (True, 1, "on", ["methods"]):
        with pytest.raises(TypeError):
            mod_utils.override_retry_policy(base, bad)
    with pytest.raises(ValueError):
        mod_utils.override_retry_policy(None, {})


def test_policy_object():
    p = RetryPolicy(policy({"retryOn": ["reset"]}))
    assert p.statuses == frozenset()        # "status" not selected
    p = RetryPolicy(policy({"retryOn": ["status"], "delay": 10,
                            "maxDelay": 35, "jitter": False}))
    assert p.statuses == {502, 503, 504}
    assert [p.backoff_cap(n) for n in (1, 2, 3, 4)] == [10, 20, 35, 35]
    assert p.backoff_cap(5000) == 35


def test_request_timeout_error():
    assert cueball_amd.RequestTimeoutError is RequestTimeoutError
    assert "RequestTimeoutError" in cueball_amd.__all__
    for kind, ms in (("per-try", 150), ("total", 2000.5)):
        e = RequestTimeoutError(kind, ms)
        assert isinstance(e, CueballError)
        assert e.kind == kind and e.timeout_ms == ms
        assert kind in str(e) and ("%g" % ms) in str(e)


def instance_vars(agent):
    """vars(agent); the native runtime's objects keep their instance
    dict without a ``__dict__`` attribute, so there it is found among
    the object's referents."""
    try:
        return vars(agent)
    except TypeError:
        for ref in gc.get_referents(agent):
            if isinstance(ref, dict) and "cba_stopped" in ref:
                return ref
        raise


def agent_on(loop, **opts):
    base = {"recovery": RECOVERY, "spares": 1, "maximum": 2, "loop": loop}
    base.update(opts)
    agent = HttpAgent(base)
    resolver = DummyResolver()
    agent.create_pool("svc", {"resolver": resolver})
    resolver.start()
    return agent


async def stop(loop, agent):
    done = []
    agent.stop(lambda err: done.append(err))
    for _ in range(50):
        await settle(loop)
        if done:
            return
    raise AssertionError("agent did not stop")


def test_inert_without_the_option():
    async def body(loop):
        agent = agent_on(loop)
        # not one new attribute
        attrs = instance_vars(agent)
        assert "cba_outlier" in attrs
        assert not [k for k in attrs if "retry" in k]
        assert agent.cba_retry is None and agent.cba_retry_hosts is None
        assert agent.get_retry_stats() == {}
        # no new metrics
        assert "cueball_agent_" not in agent.collector.collect()

        req = agent.request("svc", "GET", "/x")
        assert type(req) is HttpRequest
        req.abort()
        req = agent.request("svc", "GET", "/x", retry=False)
        assert type(req) is HttpRequest
        req.abort()
        await settle(loop)
        # no new counters
        counters = agent.get_pool("svc").get_stats()["counters"]
        assert not [c for c in counters if "retr" in c or "timeout-" in c]

        with pytest.raises(ValueError):
            agent.request("svc", "GET", "/x", retry={})
        with pytest.raises(ValueError):
            agent.request("svc", "GET", "/x", retry={"maxRetries": 1})
        with pytest.raises(TypeError):
            agent.request("svc", "GET", "/x", retry=True)
        assert agent.get_retry_stats() == {}
        await stop(loop, agent)
    run_vt(body)


def test_with_the_option():
    async def body(loop):
        agent = agent_on(loop, retry={"maxRetries": 1})
        assert agent.cba_retry == dict(DEFAULTS, maxRetries=1)
        text = agent.collector.collect()
        for name in ("cueball_agent_retries_total",
                     "cueball_agent_retry_budget_exhausted_total",
                     "cueball_agent_request_timeouts_total"):
            assert "# TYPE %s counter" % name in text
        assert agent.get_retry_stats() == {}

        req = agent.request("svc", "GET", "/x")
        assert isinstance(req, RetriedRequest)
        assert req.attempts == 1 and req.retry_reasons == []
        assert req.aborted is False
        assert agent.get_retry_stats() == {"svc": {
            "active": 1, "retrying": 0, "limit": 3,
            "counters": {c: 0 for c in COUNTERS}}}
        aborts = []
        req.on("abort", lambda: aborts.append(1))
        req.on("error", lambda e: aborts.append(e))
        req.abort()
        req.abort()
        assert aborts == [1] and req.aborted is True
        assert agent.get_retry_stats()["svc"]["active"] == 0

        off = agent.request("svc", "GET", "/x", retry=False)
        assert type(off) is HttpRequest
        off.abort()
        over = agent.request("svc", "POST", "/x",
                             retry={"methods": ["POST"]})
        assert isinstance(over, RetriedRequest)
        over.abort()
        for bad, exc in ((True, TypeError), (1, TypeError),
                         ({"budget": None}, ValueError),
                         ({"nope": 1}, ValueError)):
            with pytest.raises(exc):
                agent.request("svc", "GET", "/x", retry=bad)
        assert agent.get_retry_stats()["svc"]["active"] == 0
        # the key set of the pool's stats is what it was
        assert sorted(agent.get_pool("svc").get_stats()) == [
            "counters", "idleConnections", "pendingConnections",
            "totalConnections", "waiterCount"]
        await settle(loop)
        await stop(loop, agent)
        # a stopped agent refuses, as ever
        with pytest.raises(CueballError):
            agent.request("svc", "GET", "/x")
        assert agent.get_retry_stats()["svc"]["active"] == 0
    run_vt(body)


def test_budget_off_has_no_limit():
    async def body(loop):
        agent = agent_on(loop, retry={"budget": None})
        req = agent.request("svc", "GET", "/x")
        assert agent.get_retry_stats()["svc"]["limit"] is None
        req.abort()
        await settle(loop)
        await stop(loop, agent)
    run_vt(body)
