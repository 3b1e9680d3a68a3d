"""Shared infrastructure: the rebalance planner, recovery-spec
validation, jittered delays, stack-trace capture gating and error
metrics (reference lib/utils.js).

``plan_rebalance`` is the algorithmic core of pool/set sizing; its
behavior (dead-backend single-connection + replacement allocation under
the max cap) is pinned by the 21-case table in tests/test_utils.py, the
rebuild's port of the reference's spec suite (test/utils.test.js:13-267).
"""

from __future__ import annotations

import math
import os
import random
import socket
import time
import traceback
from typing import Any, Dict, List, Mapping, Optional, Sequence

from . import metrics as mod_metrics

__all__ = [
    "shuffle",
    "plan_rebalance",
    "active_priority",
    "ranking_report",
    "assert_recovery",
    "assert_recovery_set",
    "assert_claim_delay",
    "current_millis",
    "gen_delay",
    "stack_traces_enabled",
    "enable_stack_traces",
    "disable_stack_traces",
    "maybe_capture_stack_trace",
    "create_error_metrics",
    "update_error_metrics",
    "METRIC_CUEBALL_EVENT_COUNTER",
    "TRACKED_ERROR_EVENTS",
]

METRIC_CUEBALL_EVENT_COUNTER = "cueball_events"

#: error-related events tracked in metrics (lib/utils.js:37-46)
TRACKED_ERROR_EVENTS = frozenset([
    "timeout-during-connect",
    "error-during-connect",
    "close-during-connect",
    "error-while-connected",
    "retries-exhausted",
    "claim-timeout",
    "error-while-claimed",
    "failed-state",
])

_STACK_TRACES_ENABLED = False


def stack_traces_enabled() -> bool:
    """Claim/release stack capture is off by default for performance
    (lib/utils.js:52-58); toggled via cueball_amd.enable_stack_traces()."""
    return _STACK_TRACES_ENABLED


#: the native core's mirror of the flag (set by connection_fsm when the
#: core is loaded): fn(enabled, placeholder)
_native_stack_flag = None


def _bind_native_stack_flag(fn) -> None:
    global _native_stack_flag
    _native_stack_flag = fn
    fn(_STACK_TRACES_ENABLED, _DISABLED_STACK)


def enable_stack_traces() -> None:
    global _STACK_TRACES_ENABLED
    _STACK_TRACES_ENABLED = True
    if _native_stack_flag is not None:
        _native_stack_flag(True, _DISABLED_STACK)


def disable_stack_traces() -> None:
    global _STACK_TRACES_ENABLED
    _STACK_TRACES_ENABLED = False
    if _native_stack_flag is not None:
        _native_stack_flag(False, _DISABLED_STACK)


_DISABLED_STACK = [
    "unknown (stack traces disabled)",
    "unknown (stack traces disabled)",
]


def maybe_capture_stack_trace() -> List[str]:
    """Real stack frames if enabled, else a shared 2-frame placeholder
    (lib/utils.js:106-115; off by default "for performance" — the
    shared list keeps the disabled path allocation-free)."""
    if not _STACK_TRACES_ENABLED:
        return _DISABLED_STACK
    frames = traceback.extract_stack()[:-1]
    return ["%s (%s:%d)" % (f.name, f.filename, f.lineno) for f in frames]


def current_millis() -> float:
    """Monotonic wall time in ms (lib/utils.js:198-204).  NOTE: pool/CoDel
    code paths use the event loop's clock instead so virtual-time tests
    work; this is for callers outside a loop."""
    return time.monotonic() * 1000.0


def shuffle(array: List[Any], rng: Optional[random.Random] = None) -> List[Any]:
    """In-place Fisher-Yates shuffle (lib/utils.js:207-217)."""
    rnd = rng.random if rng is not None else random.random
    i = len(array)
    while i > 0:
        j = int(rnd() * i)
        i -= 1
        array[i], array[j] = array[j], array[i]
    return array


def gen_delay(recov_or_delay: Any, spread: Optional[float] = None,
              rng: Optional[random.Random] = None) -> int:
    """Randomize a retry delay by +/- spread/2 around its base value, to
    de-synchronize retries across clients (lib/utils.js:446-461,
    docs/internals.adoc:388-404)."""
    base = recov_or_delay
    if isinstance(recov_or_delay, Mapping) and spread is None:
        base = recov_or_delay["delay"]
        spread = recov_or_delay.get("delay_spread",
                                    recov_or_delay.get("delaySpread"))
    if not isinstance(base, (int, float)):
        raise TypeError("base delay must be a number")
    if spread is None:
        spread = 0.2
    rnd = rng.random if rng is not None else random.random
    return int(round(base * (1 - spread / 2.0 + rnd() * spread)))


def _num(v: Any) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def assert_recovery(obj: Any, name: str = "recovery") -> None:
    """Validate one recovery spec: {retries, timeout, maxTimeout?, delay,
    maxDelay?, delaySpread?} with the retries<32-needs-max rule
    (lib/utils.js:125-186, docs/api.adoc:680-749)."""
    if not isinstance(obj, Mapping):
        raise TypeError("%s must be a mapping" % name)
    allowed = {"retries", "timeout", "maxTimeout", "delay", "maxDelay",
               "delaySpread"}
    extra = set(obj.keys()) - allowed
    if extra:
        raise ValueError("%s has unknown keys: %r" % (name, sorted(extra)))

    retries = obj.get("retries")
    if not _num(retries) or not math.isfinite(retries) or retries < 0:
        raise ValueError("%s.retries must be a finite number >= 0" % name)
    timeout = obj.get("timeout")
    if not _num(timeout) or not math.isfinite(timeout) or timeout <= 0:
        raise ValueError("%s.timeout must be a finite number > 0" % name)
    max_timeout = obj.get("maxTimeout")
    if max_timeout is not None:
        if not _num(max_timeout) or timeout > max_timeout:
            raise ValueError("%s.maxTimeout must be >= timeout" % name)
    delay = obj.get("delay")
    if not _num(delay) or not math.isfinite(delay) or delay < 0:
        raise ValueError("%s.delay must be a finite number >= 0" % name)
    max_delay = obj.get("maxDelay")
    if max_delay is not None:
        if not _num(max_delay) or delay > max_delay:
            raise ValueError("%s.maxDelay must be >= delay" % name)
    spread = obj.get("delaySpread")
    if spread is not None:
        if not _num(spread) or not (0.0 <= spread <= 1.0):
            raise ValueError("%s.delaySpread must be between 0.0 and 1.0"
                             % name)

    day_ms = 1000 * 3600 * 24
    if max_delay is None:
        if retries >= 32:
            raise ValueError("%s.maxDelay is required when retries >= 32 "
                             "(exponential increase becomes unreasonably "
                             "large)" % name)
        if delay * (1 << int(retries)) >= day_ms:
            raise ValueError("%s.maxDelay is required with given values of "
                             "retries and delay (effective unspecified "
                             "maxDelay is > 1 day)" % name)
    if max_timeout is None:
        if retries >= 32:
            raise ValueError("%s.maxTimeout is required when retries >= 32 "
                             "(exponential increase becomes unreasonably "
                             "large)" % name)
        if timeout * (1 << int(retries)) >= day_ms:
            raise ValueError("%s.maxTimeout is required with given values "
                             "of retries and timeout (effective unspecified "
                             "maxTimeout is > 1 day)" % name)


def assert_recovery_set(obj: Any) -> None:
    """Validate a whole recovery-spec object: per-operation keys like
    default/dns/dns_srv/connect/initial (lib/utils.js:117-123)."""
    if not isinstance(obj, Mapping):
        raise TypeError("recovery must be a mapping")
    if "default" not in obj:
        raise ValueError("recovery.default is required")
    for k, v in obj.items():
        assert_recovery(v, "recovery.%s" % k)


def assert_claim_delay(delay: Any) -> None:
    if delay is None:
        return
    if not _num(delay) or not math.isfinite(delay):
        raise ValueError("targetClaimDelay must be a finite number")
    if delay <= 0 or delay != math.floor(delay):
        raise ValueError("targetClaimDelay must be a positive integer")


def assert_connection_age(options: Mapping[str, Any]) -> tuple:
    """Validate ``maxConnectionAge`` (ms, finite, > 0) and
    ``connectionAgeSpread`` (fraction in [0, 1), default 0.2); returns
    ``(age, spread)``, ``(None, None)`` when the option is off.  A
    spread without an age is an error."""
    age = options.get("maxConnectionAge")
    spread = options.get("connectionAgeSpread")
    if age is not None:
        if not _num(age):
            raise TypeError("options.maxConnectionAge must be a number")
        if not math.isfinite(age) or age <= 0:
            raise ValueError("options.maxConnectionAge must be finite "
                             "and > 0")
    if spread is not None:
        if not _num(spread):
            raise TypeError("options.connectionAgeSpread must be a number")
        if not math.isfinite(spread) or spread < 0 or spread >= 1:
            raise ValueError("options.connectionAgeSpread must be in "
                             "[0, 1)")
        if age is None:
            raise ValueError("options.connectionAgeSpread needs "
                             "options.maxConnectionAge")
    if age is None:
        return (None, None)
    return (age, 0.2 if spread is None else spread)


_OUTLIER_KEYS = ("consecutiveFailures", "baseEjectionTime",
                 "maxEjectionTime", "maxEjectionPercent", "countClose",
                 "countSocketClose")


def assert_outlier_detection(options: Mapping[str, Any],
                             count_default: bool = True
                             ) -> Optional[Dict[str, Any]]:
    """Validate ``outlierDetection`` and return it with every default
    filled in, or None when the option is off.  ``count_default`` is the
    default of ``countClose`` and ``countSocketClose``: True for a pool,
    False for the pools of an agent, which closes leases on purpose."""
    od = options.get("outlierDetection")
    if od is None:
        return None
    name = "options.outlierDetection"
    if not isinstance(od, Mapping):
        raise TypeError("%s must be a mapping" % name)
    extra = set(od.keys()) - set(_OUTLIER_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (name, sorted(extra, key=str)))

    fails = od.get("consecutiveFailures")
    if fails is None:
        fails = 5
    if not isinstance(fails, int) or isinstance(fails, bool):
        raise TypeError("%s.consecutiveFailures must be an int" % name)
    if fails < 1:
        raise ValueError("%s.consecutiveFailures must be >= 1" % name)

    base = od.get("baseEjectionTime")
    if base is None:
        base = 30000
    if not _num(base):
        raise TypeError("%s.baseEjectionTime must be a number" % name)
    if not math.isfinite(base) or base <= 0:
        raise ValueError("%s.baseEjectionTime must be finite and > 0" % name)

    longest = od.get("maxEjectionTime")
    if longest is None:
        longest = max(300000, base)
    if not _num(longest):
        raise TypeError("%s.maxEjectionTime must be a number" % name)
    if not math.isfinite(longest) or longest < base:
        raise ValueError("%s.maxEjectionTime must be finite and >= "
                         "baseEjectionTime" % name)

    percent = od.get("maxEjectionPercent")
    if percent is None:
        percent = 50
    if not _num(percent):
        raise TypeError("%s.maxEjectionPercent must be a number" % name)
    if not (0 < percent <= 100):
        raise ValueError("%s.maxEjectionPercent must be in (0, 100]" % name)

    out: Dict[str, Any] = {
        "consecutiveFailures": fails, "baseEjectionTime": base,
        "maxEjectionTime": longest, "maxEjectionPercent": percent}
    for k in ("countClose", "countSocketClose"):
        v = od.get(k)
        if v is None:
            v = count_default
        if not isinstance(v, bool):
            raise TypeError("%s.%s must be a bool" % (name, k))
        out[k] = v
    return out


_BALANCING_KEYS = ("policy", "choices", "decayTime", "rng")
_BALANCING_POLICIES = ("peakEwma", "leastLoaded")


def assert_claim_balancing(options: Mapping[str, Any]
                           ) -> Optional[Dict[str, Any]]:
    """Validate ``claimBalancing`` and return it with every default
    filled in (``rng`` None meaning the ``random`` module), or None
    when the option is off."""
    lb = options.get("claimBalancing")
    if lb is None:
        return None
    name = "options.claimBalancing"
    if not isinstance(lb, Mapping):
        raise TypeError("%s must be a mapping" % name)
    extra = set(lb.keys()) - set(_BALANCING_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (name, sorted(extra, key=str)))

    policy = lb.get("policy")
    if policy is None:
        policy = "peakEwma"
    if not isinstance(policy, str):
        raise TypeError("%s.policy must be a string" % name)
    if policy not in _BALANCING_POLICIES:
        raise ValueError("%s.policy must be one of %r"
                         % (name, list(_BALANCING_POLICIES)))

    choices = lb.get("choices")
    if choices is None:
        choices = 2
    if isinstance(choices, str):
        if choices != "all":
            raise ValueError('%s.choices must be an int >= 2 or "all"'
                             % name)
    elif not isinstance(choices, int) or isinstance(choices, bool):
        raise TypeError('%s.choices must be an int or "all"' % name)
    elif choices < 2:
        raise ValueError('%s.choices must be >= 2 or "all"' % name)

    decay = lb.get("decayTime")
    if decay is None:
        decay = 10000
    if not _num(decay):
        raise TypeError("%s.decayTime must be a number" % name)
    if not math.isfinite(decay) or decay <= 0:
        raise ValueError("%s.decayTime must be finite and > 0" % name)

    rng = lb.get("rng")
    if rng is not None and not isinstance(rng, random.Random):
        raise TypeError("%s.rng must be a random.Random" % name)

    return {"policy": policy, "choices": choices, "decayTime": decay,
            "rng": rng}


_QUEUE_KEYS = ("maxQueued", "priorities", "defaultPriority", "order",
               "lifoAfter")
_QUEUE_ORDERS = ("fifo", "lifo", "adaptive")
#: the most classes a claim queue may have
MAX_CLAIM_PRIORITIES = 8


def assert_claim_queue(options: Mapping[str, Any]
                       ) -> Optional[Dict[str, Any]]:
    """Validate ``claimQueue`` and return it with every default filled
    in, or None when the option is off.  ``lifoAfter`` is None under the
    orders that do not use it; under ``"adaptive"`` its default is the
    pool's ``targetClaimDelay``."""
    cq = options.get("claimQueue")
    if cq is None:
        return None
    name = "options.claimQueue"
    if not isinstance(cq, Mapping):
        raise TypeError("%s must be a mapping" % name)
    extra = set(cq.keys()) - set(_QUEUE_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (name, sorted(extra, key=str)))

    bound = cq.get("maxQueued")
    if bound is not None:
        if not isinstance(bound, int) or isinstance(bound, bool):
            raise TypeError("%s.maxQueued must be an int or None" % name)
        if bound < 1:
            raise ValueError("%s.maxQueued must be >= 1" % name)

    classes = cq.get("priorities")
    if classes is None:
        classes = 1
    if not isinstance(classes, int) or isinstance(classes, bool):
        raise TypeError("%s.priorities must be an int" % name)
    if not (1 <= classes <= MAX_CLAIM_PRIORITIES):
        raise ValueError("%s.priorities must be in 1..%d"
                         % (name, MAX_CLAIM_PRIORITIES))

    default = cq.get("defaultPriority")
    if default is None:
        default = 0
    if not isinstance(default, int) or isinstance(default, bool):
        raise TypeError("%s.defaultPriority must be an int" % name)
    if not (0 <= default < classes):
        raise ValueError("%s.defaultPriority must be in 0..%d"
                         % (name, classes - 1))

    order = cq.get("order")
    if order is None:
        order = "fifo"
    if not isinstance(order, str):
        raise TypeError("%s.order must be a string" % name)
    if order not in _QUEUE_ORDERS:
        raise ValueError("%s.order must be one of %r"
                         % (name, list(_QUEUE_ORDERS)))

    after = cq.get("lifoAfter")
    if after is not None:
        if not _num(after):
            raise TypeError("%s.lifoAfter must be a number" % name)
        if order != "adaptive":
            raise ValueError('%s.lifoAfter needs order "adaptive"' % name)
        if not math.isfinite(after) or after < 0:
            raise ValueError("%s.lifoAfter must be finite and >= 0" % name)
    elif order == "adaptive":
        after = options.get("targetClaimDelay")
        if after is None:
            raise ValueError('%s.lifoAfter is required under order '
                             '"adaptive" unless the pool has '
                             'targetClaimDelay' % name)
        assert_claim_delay(after)

    return {"maxQueued": bound, "priorities": classes,
            "defaultPriority": default, "order": order,
            "lifoAfter": after}


def assert_claim_priority(priority: Any, cq: Optional[Mapping[str, Any]],
                          name: str = "options.priority",
                          owner: str = "a pool") -> int:
    """Validate a claim's class against `cq`, the validated
    ``claimQueue`` of the pool or agent asked (None when it has none):
    an int that is not a bool, in ``0 .. priorities-1``.  Naming a class
    where there is no ``claimQueue`` is a ValueError."""
    if not isinstance(priority, int) or isinstance(priority, bool):
        raise TypeError("%s must be an int" % name)
    if cq is None:
        raise ValueError("%s needs %s that was created with "
                         "options.claimQueue" % (name, owner))
    if not (0 <= priority < cq["priorities"]):
        raise ValueError("%s must be in 0..%d"
                         % (name, cq["priorities"] - 1))
    return priority


_AFFINITY_KEYS = ("loadFactor",)


def assert_claim_affinity(options: Mapping[str, Any]
                          ) -> Optional[Dict[str, Any]]:
    """Validate ``claimAffinity`` and return it with every default
    filled in, or None when the option is off.  ``loadFraction`` is
    ``loadFactor`` as an exact ratio ``(num, den)``, None for no
    bound."""
    from . import affinity as mod_affinity
    af = options.get("claimAffinity")
    if af is None:
        return None
    name = "options.claimAffinity"
    if not isinstance(af, Mapping):
        raise TypeError("%s must be a mapping" % name)
    extra = set(af.keys()) - set(_AFFINITY_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (name, sorted(extra, key=str)))
    factor = af.get("loadFactor", mod_affinity.DEFAULT_LOAD_FACTOR)
    fraction = None
    if factor is not None:
        if not _num(factor):
            raise TypeError("%s.loadFactor must be a number or None" % name)
        if not math.isfinite(factor) or factor < 1.0:
            raise ValueError("%s.loadFactor must be finite and >= 1.0"
                             % name)
        fraction = mod_affinity.load_fraction(factor)
    return {"loadFactor": factor, "loadFraction": fraction}


def assert_affinity_key(key: Any, af: Optional[Mapping[str, Any]],
                        name: str = "options.affinityKey",
                        owner: str = "a pool") -> bytes:
    """Validate a claim's affinity key against `af`, the validated
    ``claimAffinity`` of the pool or agent asked (None when it has
    none), and return it as the bytes the hash reads.  Naming a key
    where there is no ``claimAffinity`` is a ValueError."""
    from . import affinity as mod_affinity
    if not isinstance(key, (bytes, str)):
        raise TypeError("%s must be bytes or str" % name)
    if af is None:
        raise ValueError("%s needs %s that was created with "
                         "options.claimAffinity" % (name, owner))
    return mod_affinity.key_bytes(key)


_LIMIT_COMMON_KEYS = ("algorithm", "window", "minSamples", "minLimit",
                      "maxLimit", "initialLimit")
_LIMIT_KEYS = {
    "aimd": _LIMIT_COMMON_KEYS + ("latencyThreshold", "backoffRatio"),
    "gradient": _LIMIT_COMMON_KEYS + (
        "tolerance", "smoothing", "probeInterval", "probeSpread",
        "probeLimit", "probeSamples", "random"),
}


def assert_concurrency_limit(options: Mapping[str, Any]
                             ) -> Optional[Dict[str, Any]]:
    """Validate ``concurrencyLimit`` against the pool's ``maximum`` and
    return it with every default filled in (``random`` None meaning the
    ``random`` module), or None when the option is off (None or False).
    True stands for ``{}``: every default, which is the gradient
    controller."""
    cl = options.get("concurrencyLimit")
    if cl is None or cl is False:
        return None
    name = "options.concurrencyLimit"
    if cl is True:
        cl = {}
    if not isinstance(cl, Mapping):
        raise TypeError("%s must be a mapping or a bool" % name)
    algorithm = cl.get("algorithm")
    if algorithm is None:
        algorithm = "gradient"
    if not isinstance(algorithm, str):
        raise TypeError("%s.algorithm must be a string" % name)
    if algorithm not in _LIMIT_KEYS:
        raise ValueError("%s.algorithm must be one of %r"
                         % (name, sorted(_LIMIT_KEYS)))
    extra = set(cl.keys()) - set(_LIMIT_KEYS[algorithm])
    if extra:
        raise ValueError("%s has unknown keys under %r: %r"
                         % (name, algorithm, sorted(extra, key=str)))

    def number(key: str, default: Any) -> Any:
        v = cl.get(key)
        if v is None:
            return default
        if not _num(v):
            raise TypeError("%s.%s must be a number" % (name, key))
        if not math.isfinite(v):
            raise ValueError("%s.%s must be finite" % (name, key))
        return v

    def integer(key: str, default: Any) -> Any:
        v = cl.get(key)
        if v is None:
            return default
        if not isinstance(v, int) or isinstance(v, bool):
            raise TypeError("%s.%s must be an int" % (name, key))
        return v

    maximum = options.get("maximum")
    window = number("window", 1000)
    if window <= 0:
        raise ValueError("%s.window must be > 0" % name)
    min_samples = integer("minSamples", 10)
    if min_samples < 1:
        raise ValueError("%s.minSamples must be >= 1" % name)
    min_limit = integer("minLimit", 1)
    max_limit = integer("maxLimit", maximum)
    if not isinstance(max_limit, int) or isinstance(max_limit, bool):
        raise TypeError("%s.maxLimit needs the pool's maximum" % name)
    if min_limit < 1:
        raise ValueError("%s.minLimit must be >= 1" % name)
    if not (min_limit <= max_limit) or \
            (isinstance(maximum, int) and max_limit > maximum):
        raise ValueError("%s needs minLimit <= maxLimit <= maximum" % name)
    initial = number("initialLimit", max_limit)
    if not (min_limit <= initial <= max_limit):
        raise ValueError("%s.initialLimit must be in minLimit..maxLimit"
                         % name)
    out: Dict[str, Any] = {
        "algorithm": algorithm, "window": window,
        "minSamples": min_samples, "minLimit": min_limit,
        "maxLimit": max_limit, "initialLimit": initial}

    if algorithm == "aimd":
        threshold = number("latencyThreshold", None)
        if threshold is None:
            raise ValueError('%s.latencyThreshold is required under '
                             'algorithm "aimd"' % name)
        if threshold <= 0:
            raise ValueError("%s.latencyThreshold must be > 0" % name)
        ratio = number("backoffRatio", 0.9)
        if not (0.5 <= ratio < 1):
            raise ValueError("%s.backoffRatio must be in [0.5, 1)" % name)
        out.update(latencyThreshold=threshold, backoffRatio=ratio)
        return out

    tolerance = number("tolerance", 1.5)
    if tolerance < 1.0:
        raise ValueError("%s.tolerance must be >= 1.0" % name)
    smoothing = number("smoothing", 0.2)
    if not (0 < smoothing <= 1):
        raise ValueError("%s.smoothing must be in (0, 1]" % name)
    interval = number("probeInterval", 30000)
    if interval <= 0:
        raise ValueError("%s.probeInterval must be > 0" % name)
    spread = number("probeSpread", 0.15)
    if not (0 <= spread < 1):
        raise ValueError("%s.probeSpread must be in [0, 1)" % name)
    probe_limit = integer("probeLimit", 3)
    if probe_limit < 1:
        raise ValueError("%s.probeLimit must be >= 1" % name)
    probe_samples = integer("probeSamples", min_samples)
    if probe_samples < 1:
        raise ValueError("%s.probeSamples must be >= 1" % name)
    rnd = cl.get("random")
    if rnd is not None and not callable(getattr(rnd, "random", None)):
        raise TypeError("%s.random must have a random() method" % name)
    out.update(tolerance=tolerance, smoothing=smoothing,
               probeInterval=interval, probeSpread=spread,
               probeLimit=probe_limit, probeSamples=probe_samples,
               random=rnd)
    return out


RETRY_REASONS =("reset", "timeout", "status", "claim-failure")

_RETRY_KEYS = ("maxRetries", "retryOn", "retryStatuses", "methods",
               "perTryTimeout", "totalTimeout", "delay", "maxDelay",
               "jitter", "avoidFailedBackends", "budget")
_RETRY_BUDGET_KEYS = ("percent", "minConcurrency")


def _retry_list(value: Any, name: str, default: Sequence[Any]) -> List[Any]:
    """A list option: any iterable but a string or a mapping, without
    duplicates, in the order given."""
    if value is None:
        return list(default)
    if isinstance(value, (str, bytes, Mapping)):
        raise TypeError("%s must be a list" % name)
    try:
        items = list(value)
    except TypeError:
        raise TypeError("%s must be a list" % name)
    out: List[Any] = []
    for item in items:
        if item not in out:
            out.append(item)
    return out


def _retry_ms(value: Any, name: str) -> Optional[float]:
    if value is None:
        return None
    if not _num(value):
        raise TypeError("%s must be a number" % name)
    if not math.isfinite(value) or value <= 0:
        raise ValueError("%s must be finite and > 0" % name)
    return value


def assert_retry_policy(options: Mapping[str, Any]
                        ) -> Optional[Dict[str, Any]]:
    """Validate an agent's ``retry`` option and return the policy with
    every default filled in, or None when the option is off.  ``budget``
    is a mapping ``{percent, minConcurrency}``; an explicit None turns
    the budget off."""
    retry = options.get("retry")
    if retry is None:
        return None
    name = "options.retry"
    if not isinstance(retry, Mapping):
        raise TypeError("%s must be a mapping" % name)
    extra = set(retry.keys()) - set(_RETRY_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (name, sorted(extra, key=str)))

    retries = retry.get("maxRetries")
    if retries is None:
        retries = 2
    if not isinstance(retries, int) or isinstance(retries, bool):
        raise TypeError("%s.maxRetries must be an int" % name)
    if retries < 0:
        raise ValueError("%s.maxRetries must be >= 0" % name)

    retry_on = _retry_list(retry.get("retryOn"), name + ".retryOn",
                           ("reset", "timeout"))
    for reason in retry_on:
        if not isinstance(reason, str):
            raise TypeError("%s.retryOn must hold strings" % name)
        if reason not in RETRY_REASONS:
            raise ValueError("%s.retryOn: unknown reason %r (one of %s)"
                             % (name, reason, ", ".join(RETRY_REASONS)))

    statuses = _retry_list(retry.get("retryStatuses"),
                           name + ".retryStatuses", (502, 503, 504))
    for code in statuses:
        if not isinstance(code, int) or isinstance(code, bool):
            raise TypeError("%s.retryStatuses must hold ints" % name)
        if not (100 <= code <= 599):
            raise ValueError("%s.retryStatuses: %d is not an HTTP status"
                             % (name, code))

    methods = _retry_list(retry.get("methods"), name + ".methods",
                          ("GET", "HEAD", "OPTIONS", "PUT", "DELETE"))
    for method in methods:
        if not isinstance(method, str):
            raise TypeError("%s.methods must hold strings" % name)
        if not method:
            raise ValueError("%s.methods must not hold an empty string"
                             % name)
    methods = _retry_list([m.upper() for m in methods], "", ())

    per_try = _retry_ms(retry.get("perTryTimeout"), name + ".perTryTimeout")
    total = _retry_ms(retry.get("totalTimeout"), name + ".totalTimeout")

    delay = retry.get("delay")
    if delay is None:
        delay = 25
    if not _num(delay):
        raise TypeError("%s.delay must be a number" % name)
    if not math.isfinite(delay) or delay < 0:
        raise ValueError("%s.delay must be finite and >= 0" % name)
    max_delay = retry.get("maxDelay")
    if max_delay is None:
        max_delay = max(250, delay)
    if not _num(max_delay):
        raise TypeError("%s.maxDelay must be a number" % name)
    if not math.isfinite(max_delay) or max_delay < delay:
        raise ValueError("%s.maxDelay must be finite and >= delay" % name)

    out: Dict[str, Any] = {
        "maxRetries": retries, "retryOn": retry_on,
        "retryStatuses": statuses, "methods": methods,
        "perTryTimeout": per_try, "totalTimeout": total,
        "delay": delay, "maxDelay": max_delay}
    for k in ("jitter", "avoidFailedBackends"):
        v = retry.get(k)
        if v is None:
            v = True
        if not isinstance(v, bool):
            raise TypeError("%s.%s must be a bool" % (name, k))
        out[k] = v

    if "budget" in retry and retry["budget"] is None:
        out["budget"] = None
        return out
    budget = retry.get("budget")
    if budget is None:
        budget = {}
    bname = name + ".budget"
    if not isinstance(budget, Mapping):
        raise TypeError("%s must be a mapping or None" % bname)
    extra = set(budget.keys()) - set(_RETRY_BUDGET_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (bname, sorted(extra, key=str)))
    percent = budget.get("percent")
    if percent is None:
        percent = 20
    if not _num(percent):
        raise TypeError("%s.percent must be a number" % bname)
    if not (0 <= percent <= 100):
        raise ValueError("%s.percent must be in [0, 100]" % bname)
    min_conc = budget.get("minConcurrency")
    if min_conc is None:
        min_conc = 3
    if not isinstance(min_conc, int) or isinstance(min_conc, bool):
        raise TypeError("%s.minConcurrency must be an int" % bname)
    if min_conc < 0:
        raise ValueError("%s.minConcurrency must be >= 0" % bname)
    out["budget"] = {"percent": percent, "minConcurrency": min_conc}
    return out


def override_retry_policy(policy: Optional[Mapping[str, Any]],
                          override: Any) -> Dict[str, Any]:
    """The policy of one call: `policy` (an agent's validated ``retry``)
    with the keys of `override` replaced and validated again.  Every
    key but ``budget`` may be overridden: the budget is shared by all
    requests to a host."""
    if policy is None:
        raise ValueError("retry= needs an agent that was created with "
                         "options.retry")
    if not isinstance(override, Mapping):
        raise TypeError("retry= must be False or a mapping")
    if "budget" in override:
        raise ValueError("retry= cannot override budget: it is shared by "
                         "every request to the host")
    merged = dict(policy)
    merged.update(override)
    out = assert_retry_policy({"retry": merged})
    assert out is not None
    return out


_HEDGE_KEYS = ("delay", "percentile", "window", "minSamples", "minDelay",
               "maxDelay", "methods", "budget")
#: shared by every request to a host, so not for one call to change
_HEDGE_SHARED_KEYS = ("budget", "window", "minSamples")


def assert_hedge_policy(options: Mapping[str, Any]
                        ) -> Optional[Dict[str, Any]]:
    """Validate an agent's ``hedge`` option and return the policy with
    every default filled in, or None when the option is off.  ``delay``
    None means adaptive: a percentile of recent response times.
    ``budget`` is a mapping ``{percent, minConcurrency}``; an explicit
    None turns the budget off."""
    hedge = options.get("hedge")
    if hedge is None:
        return None
    name = "options.hedge"
    if not isinstance(hedge, Mapping):
        raise TypeError("%s must be a mapping" % name)
    extra = set(hedge.keys()) - set(_HEDGE_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (name, sorted(extra, key=str)))

    delay = _retry_ms(hedge.get("delay"), name + ".delay")

    percentile = hedge.get("percentile")
    if percentile is None:
        percentile = 95
    if not _num(percentile):
        raise TypeError("%s.percentile must be a number" % name)
    if not (0 < percentile < 100):
        raise ValueError("%s.percentile must be in (0, 100)" % name)

    window = _retry_ms(hedge.get("window"), name + ".window")
    if window is None:
        window = 10000

    samples = hedge.get("minSamples")
    if samples is None:
        samples = 50
    if not isinstance(samples, int) or isinstance(samples, bool):
        raise TypeError("%s.minSamples must be an int" % name)
    if samples < 1:
        raise ValueError("%s.minSamples must be >= 1" % name)

    min_delay = _retry_ms(hedge.get("minDelay"), name + ".minDelay")
    if min_delay is None:
        min_delay = 1
    max_delay = hedge.get("maxDelay")
    if max_delay is None:
        max_delay = max(1000, min_delay)
    if not _num(max_delay):
        raise TypeError("%s.maxDelay must be a number" % name)
    if not math.isfinite(max_delay) or max_delay < min_delay:
        raise ValueError("%s.maxDelay must be finite and >= minDelay" % name)

    methods = _retry_list(hedge.get("methods"), name + ".methods",
                          ("GET", "HEAD", "OPTIONS"))
    for method in methods:
        if not isinstance(method, str):
            raise TypeError("%s.methods must hold strings" % name)
        if not method:
            raise ValueError("%s.methods must not hold an empty string"
                             % name)
    methods = _retry_list([m.upper() for m in methods], "", ())

    out: Dict[str, Any] = {
        "delay": delay, "percentile": percentile, "window": window,
        "minSamples": samples, "minDelay": min_delay, "maxDelay": max_delay,
        "methods": methods}

    if "budget" in hedge and hedge["budget"] is None:
        out["budget"] = None
        return out
    budget = hedge.get("budget")
    if budget is None:
        budget = {}
    bname = name + ".budget"
    if not isinstance(budget, Mapping):
        raise TypeError("%s must be a mapping or None" % bname)
    extra = set(budget.keys()) - set(_RETRY_BUDGET_KEYS)
    if extra:
        raise ValueError("%s has unknown keys: %r"
                         % (bname, sorted(extra, key=str)))
    percent = budget.get("percent")
    if percent is None:
        percent = 10
    if not _num(percent):
        raise TypeError("%s.percent must be a number" % bname)
    if not (0 <= percent <= 100):
        raise ValueError("%s.percent must be in [0, 100]" % bname)
    min_conc = budget.get("minConcurrency")
    if min_conc is None:
        min_conc = 1
    if not isinstance(min_conc, int) or isinstance(min_conc, bool):
        raise TypeError("%s.minConcurrency must be an int" % bname)
    if min_conc < 0:
        raise ValueError("%s.minConcurrency must be >= 0" % bname)
    out["budget"] = {"percent": percent, "minConcurrency": min_conc}
    return out


def override_hedge_policy(policy: Optional[Mapping[str, Any]],
                          override: Any) -> Dict[str, Any]:
    """The policy of one call: `policy` (an agent's validated ``hedge``)
    with the keys of `override` replaced and validated again.  Every
    key may be overridden but ``budget``, ``window`` and ``minSamples``:
    the budget and the latency window are shared by all requests to a
    host."""
    if policy is None:
        raise ValueError("hedge= needs an agent that was created with "
                         "options.hedge")
    if not isinstance(override, Mapping):
        raise TypeError("hedge= must be False or a mapping")
    for k in _HEDGE_SHARED_KEYS:
        if k in override:
            raise ValueError("hedge= cannot override %s: it is shared by "
                             "every request to the host" % k)
    merged = dict(policy)
    merged.update(override)
    out = assert_hedge_policy({"hedge": merged})
    assert out is not None
    return out


def plan_rebalance(connections: Mapping[str, Sequence[Any]],
                   dead: Mapping[str, bool],
                   target: int, maximum: int,
                   singleton: bool = False,
                   ranks: Optional[Mapping[str, Sequence[int]]] = None
                   ) -> Dict[str, List[Any]]:
    """Compute the add/remove plan that takes the pool to an even spread.

    Semantics (reference lib/utils.js:239-393): round-robin ``target``
    connections over the backend preference list (the iteration order of
    ``connections``); any dead backend gets exactly one slot (its
    monitor) plus a queued *replacement* allocation, replacements
    themselves round-robin with the documented cap/starvation rules so
    every backend is tried at least once even when the max cap prevents
    double-replacement.  With ``singleton`` (Sets), at most one
    connection per distinct backend.

    With ``ranks`` (key -> (priority, weight), SRV ranking) only the
    active priority tier is spread, by weight; see
    ``_plan_rebalance_ranked``.  ``ranks=None`` never looks at rank data.

    Returns {"add": [backend keys...], "remove": [connection objects...]}.
    """
    if ranks is not None:
        return _plan_rebalance_ranked(connections, dead, target, maximum,
                                      singleton, ranks)
    if target < 0:
        raise ValueError("target must be >= 0")
    if maximum < target:
        raise ValueError("max must be >= target")

    keys = list(connections.keys())
    wanted: Dict[str, int] = {}
    plan: Dict[str, List[Any]] = {"add": [], "remove": []}
    replacements = 0
    done = 0

    # Pass 1: spread `target` connections round-robin; dead backends get
    # exactly one (the monitor) and queue a replacement.
    for _ in range(target):
        if not keys:
            break
        k = keys.pop(0)
        keys.append(k)
        if k not in wanted:
            wanted[k] = 0
        if not dead.get(k, False):
            if singleton:
                if wanted[k] == 0:
                    wanted[k] = 1
                    done += 1
            else:
                wanted[k] += 1
                done += 1
            continue
        if wanted[k] == 0:
            wanted[k] = 1
            done += 1
        replacements += 1

    if done + replacements > maximum:
        replacements = maximum - done

    # Pass 2: allocate replacements round-robin, with starvation control
    # under the max cap (see reference comments at lib/utils.js:314-327).
    i = 0
    while i < replacements:
        k = keys.pop(0)
        keys.append(k)
        first_visit = k not in wanted
        if first_visit:
            wanted[k] = 0
        alive = not dead.get(k, False)
        if alive:
            if singleton:
                if wanted[k] == 0:
                    wanted[k] = 1
                    done += 1
                    i += 1
                    continue
            else:
                wanted[k] += 1
                done += 1
                i += 1
                continue

        count = done + replacements - i
        if singleton:
            empties = [kk for kk in keys
                       if not dead.get(kk, False) and kk not in wanted]
        else:
            empties = [kk for kk in keys
                       if not dead.get(kk, False) or kk not in wanted]

        if count + 1 <= maximum:
            # room for both this dead backend and a further replacement
            if wanted[k] == 0:
                wanted[k] = 1
                done += 1
            if empties:
                replacements += 1
        elif count <= maximum and empties:
            # only room for one, but live/untried candidates exist: skip
            replacements += 1
        elif count <= maximum:
            # only room for one and everything looks dead: use this one
            if wanted[k] == 0:
                wanted[k] = 1
                done += 1
        else:
            break
        i += 1

    # Diff what we have against what we want.  Removals prefer backends
    # at the tail of the preference list, and remove the oldest
    # connections first; adds go in preference order.
    fwd = list(connections.keys())
    for key in reversed(fwd):
        have = len(connections.get(key) or ())
        want = wanted.get(key, 0)
        lst = list(connections.get(key) or ())
        while have > want:
            plan["remove"].append(lst.pop(0))
            have -= 1
    for key in fwd:
        have = len(connections.get(key) or ())
        want = wanted.get(key, 0)
        while have < want:
            plan["add"].append(key)
            have += 1

    return plan

def _diff_plan(connections: Mapping[str, Sequence[Any]],
               wanted: Mapping[str, int]) -> Dict[str, List[Any]]:
    """Diff what we have against what we want.  Removals prefer backends
    at the tail of the preference list, and remove the oldest connections
    first; adds go in preference order."""
    plan: Dict[str, List[Any]] = {"add": [], "remove": []}
    fwd = list(connections.keys())
    for key in reversed(fwd):
        lst = list(connections.get(key) or ())
        have = len(lst)
        want = wanted.get(key, 0)
        while have > want:
            plan["remove"].append(lst.pop(0))
            have -= 1
    for key in fwd:
        have = len(connections.get(key) or ())
        want = wanted.get(key, 0)
        while have < want:
            plan["add"].append(key)
            have += 1
    return plan


def active_priority(keys: Sequence[str], dead: Mapping[str, bool],
                    ranks: Mapping[str, Sequence[int]]) -> Optional[int]:
    """The SRV priority tier a pool or set should be using: the lowest
    priority value with at least one backend not declared dead, or, when
    every backend is dead, the lowest priority present.  None without
    backends.  Keys missing from ``ranks`` rank as (0, 0)."""
    lowest: Optional[int] = None
    lowest_alive: Optional[int] = None
    for k in keys:
        prio = ranks[k][0] if k in ranks else 0
        if lowest is None or prio < lowest:
            lowest = prio
        if not dead.get(k, False) and \
                (lowest_alive is None or prio < lowest_alive):
            lowest_alive = prio
    return lowest_alive if lowest_alive is not None else lowest


def ranking_report(keys: Sequence[str], dead: Mapping[str, bool],
                   ranks: Optional[Mapping[str, Sequence[int]]],
                   connections: Mapping[str, int]) -> Dict[str, Any]:
    """The body of ``get_ranking()`` for pools and sets: backends
    grouped into priority tiers, ascending.  ``connections`` maps key ->
    live connection count."""
    if ranks is None:
        return {"enabled": False}
    tiers: Dict[int, Dict[str, Any]] = {}
    for k in keys:
        prio, weight = ranks[k] if k in ranks else (0, 0)
        t = tiers.get(prio)
        if t is None:
            t = tiers[prio] = {"priority": prio, "backends": 0, "dead": 0,
                               "connections": 0, "weights": {}}
        t["backends"] += 1
        if dead.get(k, False):
            t["dead"] += 1
        t["connections"] += connections.get(k, 0)
        t["weights"][k] = weight
    return {
        "enabled": True,
        "activePriority": active_priority(keys, dead, ranks),
        "tiers": [tiers[p] for p in sorted(tiers)],
    }


class _WeightedCycle:
    """Key source of the ranked planner: smooth weighted round-robin
    over one tier, in preference order.  Every ``next()`` adds each
    key's weight to its running score, takes the highest score (ties to
    the earliest key) and subtracts the total from the winner, so over
    any ``sum(weights)`` consecutive steps key i is returned exactly
    ``weights[i]`` times, interleaved, not in runs.  With equal weights
    this is plain round-robin."""

    __slots__ = ("keys", "weights", "scores", "total")

    def __init__(self, keys: Sequence[str], weights: Sequence[int]) -> None:
        self.keys = list(keys)
        self.weights = list(weights)
        self.scores = [0] * len(self.keys)
        self.total = sum(self.weights)

    def next(self) -> str:
        scores = self.scores
        best = 0
        for i, w in enumerate(self.weights):
            scores[i] += w
            if scores[i] > scores[best]:
                best = i
        scores[best] -= self.total
        return self.keys[best]


def _plan_rebalance_ranked(connections: Mapping[str, Sequence[Any]],
                           dead: Mapping[str, bool],
                           target: int, maximum: int, singleton: bool,
                           ranks: Mapping[str, Sequence[int]]
                           ) -> Dict[str, List[Any]]:
    """``plan_rebalance`` with SRV ranks (RFC 2782).

    Only the active tier (``active_priority``) carries load.  Tiers
    numbered below it are dead by construction and get one slot each,
    their monitor, so the pool can fail back; at most ``maximum - 1`` of
    those, so the active tier always keeps a slot.  Tiers numbered above
    it get nothing.  The two passes of ``plan_rebalance`` then run over
    the active tier alone, with what is left of ``maximum``, drawing
    keys from a ``_WeightedCycle`` instead of the plain rotation.

    A key's weight in the cycle is ``max(weight, 1)`` over the tier's
    gcd (weight 0 means "very small share", not "never"), except that a
    dead backend always counts 1 (it only needs its monitor, and its
    share flows to the replacements) and in ``singleton`` mode every key
    counts 1 and the tier is visited heaviest first.  Both exceptions
    also keep the number of steps independent of the weights.  With all
    ranks equal the plan is exactly that of ``ranks=None``.
    """
    if target < 0:
        raise ValueError("target must be >= 0")
    if maximum < target:
        raise ValueError("max must be >= target")

    all_keys = list(connections.keys())
    wanted: Dict[str, int] = {}
    if not all_keys:
        return {"add": [], "remove": []}

    def rank(k: str) -> Sequence[int]:
        return ranks[k] if k in ranks else (0, 0)

    active = active_priority(all_keys, dead, ranks)

    # Monitor slots for the tiers we failed away from.
    lower = sorted((k for k in all_keys if rank(k)[0] < active),
                   key=lambda k: rank(k)[0])
    monitors = lower[:max(maximum - 1, 0)]
    for k in monitors:
        wanted[k] = 1
    maximum -= len(monitors)
    if target > maximum:
        target = maximum

    tier = [k for k in all_keys if rank(k)[0] == active]
    if singleton:
        tier.sort(key=lambda k: -max(rank(k)[1], 1))
        weights = [1] * len(tier)
    else:
        raw = [max(rank(k)[1], 1) for k in tier]
        div = math.gcd(*raw)
        weights = [1 if dead.get(k, False) else w // div
                   for k, w in zip(tier, raw)]
    cycle = _WeightedCycle(tier, weights)

    replacements = 0
    done = 0

    # Pass 1: spread `target` connections by weight; dead backends get
    # exactly one (the monitor) and queue a replacement.
    for _ in range(target):
        k = cycle.next()
        if k not in wanted:
            wanted[k] = 0
        if not dead.get(k, False):
            if singleton:
                if wanted[k] == 0:
                    wanted[k] = 1
                    done += 1
            else:
                wanted[k] += 1
                done += 1
            continue
        if wanted[k] == 0:
            wanted[k] = 1
            done += 1
        replacements += 1

    if done + replacements > maximum:
        replacements = maximum - done

    # Pass 2: allocate replacements, with the same starvation control
    # under the max cap as plan_rebalance.
    i = 0
    while i < replacements:
        k = cycle.next()
        if k not in wanted:
            wanted[k] = 0
        alive = not dead.get(k, False)
        if alive:
            if singleton:
                if wanted[k] == 0:
                    wanted[k] = 1
                    done += 1
                    i += 1
                    continue
            else:
                wanted[k] += 1
                done += 1
                i += 1
                continue

        count = done + replacements - i
        if singleton:
            empties = [kk for kk in tier
                       if not dead.get(kk, False) and kk not in wanted]
        else:
            empties = [kk for kk in tier
                       if not dead.get(kk, False) or kk not in wanted]

        if count + 1 <= maximum:
            if wanted[k] == 0:
                wanted[k] = 1
                done += 1
            if empties:
                replacements += 1
        elif count <= maximum and empties:
            replacements += 1
        elif count <= maximum:
            if wanted[k] == 0:
                wanted[k] = 1
                done += 1
        else:
            break
        i += 1

    return _diff_plan(connections, wanted)


def create_error_metrics(options: Mapping[str, Any]) -> mod_metrics.Collector:
    """Get (or make) the shared collector and register the cueball_events
    counter (idempotent, lib/utils.js:395-418)."""
    collector = options.get("collector")
    if collector is None:
        collector = mod_metrics.create_collector(labels={
            "component": "cueball",
        })
    collector.counter(
        name=METRIC_CUEBALL_EVENT_COUNTER,
        help="Total number of cueball error events",
    )
    return collector


def update_error_metrics(collector: mod_metrics.Collector, uuid: str,
                         err_str: str) -> None:
    """Count one tracked error event (lib/utils.js:420-444)."""
    if err_str not in TRACKED_ERROR_EVENTS:
        return
    errors = collector.get_collector(METRIC_CUEBALL_EVENT_COUNTER)
    errors.increment({
        "hostname": socket.gethostname(),
        "uuid": uuid,
        "type": "error",
        "evt": err_str,
    })
