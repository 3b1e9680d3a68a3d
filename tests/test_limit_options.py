"""``concurrencyLimit``: validation, and a pool without the option is
what it was."""

import random

import pytest

from cueball_amd import utils as mod_utils
from cueball_amd.testing import settle
from conftest import run_vt
from balance_kit import PLAIN_POOL_VARS, Kit, instance_vars
from limit_kit import LimitKit


def check(cl, maximum=16):
    return mod_utils.assert_concurrency_limit(
        {"maximum": maximum, "concurrencyLimit": cl})


@pytest.mark.parametrize("off", [None, False])
def test_none_and_false_mean_off(off):
    assert check(off) is None
    assert mod_utils.assert_concurrency_limit({"maximum": 16}) is None


@pytest.mark.parametrize("on", [True, {}])
def test_true_and_empty_mean_every_default_which_is_gradient(on):
    assert check(on) == {
        "algorithm": "gradient", "window": 1000, "minSamples": 10,
        "minLimit": 1, "maxLimit": 16, "initialLimit": 16,
        "tolerance": 1.5, "smoothing": 0.2, "probeInterval": 30000,
        "probeSpread": 0.15, "probeLimit": 3, "probeSamples": 10,
        "random": None}


def test_aimd_defaults_and_probe_samples_follow_min_samples():
    assert check({"algorithm": "aimd", "latencyThreshold": 75}) == {
        "algorithm": "aimd", "window": 1000, "minSamples": 10,
        "minLimit": 1, "maxLimit": 16, "initialLimit": 16,
        "latencyThreshold": 75, "backoffRatio": 0.9}
    assert check({"minSamples": 4})["probeSamples"] == 4
    assert check({"maxLimit": 8})["initialLimit"] == 8
    rng = random.Random(1)
    assert check({"random": rng})["random"] is rng
    # what comes out goes in again unchanged (an agent hands it on)
    for cl in ({}, {"algorithm": "aimd", "latencyThreshold": 75}):
        assert check(check(cl)) == check(cl)


@pytest.mark.parametrize("cl", [
    {"bogus": 1},
    {"algorithm": "vegas"},
    {"algorithm": "aimd"},                              # no threshold
    {"algorithm": "aimd", "latencyThreshold": 0},
    {"algorithm": "aimd", "latencyThreshold": 75, "backoffRatio": 0.4},
    {"algorithm": "aimd", "latencyThreshold": 75, "backoffRatio": 1},
    {"algorithm": "aimd", "latencyThreshold": 75, "tolerance": 2},
    {"latencyThreshold": 75},                           # gradient has none
    {"window": 0},
    {"minSamples": 0},
    {"minLimit": 0},
    {"minLimit": 5, "maxLimit": 4},
    {"maxLimit": 17},                                   # over maximum
    {"initialLimit": 17},
    {"minLimit": 3, "initialLimit": 2},
    {"tolerance": 0.9},
    {"smoothing": 0},
    {"smoothing": 1.1},
    {"probeInterval": 0},
    {"probeSpread": -0.1},
    {"probeSpread": 1},
    {"probeLimit": 0},
    {"probeSamples": 0},
    {"window": float("inf")},
])
def test_bad_values_are_value_errors(cl):
    with pytest.raises(ValueError):
        check(cl)


@pytest.mark.parametrize("cl", [
    7, "gradient", ["aimd"],
    {"algorithm": 3},
    {"window": "1000"},
    {"window": True},
    {"minSamples": 2.5},
    {"minLimit": 1.0},
    {"maxLimit": "16"},
    {"initialLimit": "4"},
    {"tolerance": "1.5"},
    {"smoothing": None, "probeLimit": 2.0},
    {"probeSamples": True},
    {"random": 4},
    {"algorithm": "aimd", "latencyThreshold": "75"},
    {"algorithm": "aimd", "latencyThreshold": 75, "backoffRatio": "0.9"},
])
def test_wrong_types_are_type_errors(cl):
    with pytest.raises(TypeError):
        check(cl)


def test_a_plain_pool_is_what_it_was():
    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert pool.get_limit_stats() == {"enabled": False}
        assert pool.p_cl is None
        box = kit.claim()
        await settle(loop)
        box["hdl"].release()
        await settle(loop)
        assert set(instance_vars(pool)) == PLAIN_POOL_VARS
        assert not any(k.startswith("limit-")
                       for k in pool.get_stats()["counters"])
        await kit.stop()
    run_vt(body)


def test_an_opted_in_pool_says_so_and_a_bad_option_fails_the_pool():
    async def body(loop):
        kit = await LimitKit(loop, True).up()
        st = kit.limit()
        assert set(st) == {
            "enabled", "algorithm", "limit", "allowed", "inFlight",
            "probing", "baselineMs", "lastWindowMeanMs", "windows",
            "probes", "samples", "discarded", "raised", "lowered"}
        assert st["enabled"] is True and st["algorithm"] == "gradient"
        assert st["limit"] == 16.0 and st["inFlight"] == 0
        # the limiter starts in a probe
        assert st["probing"] is True and st["allowed"] == 3
        assert set(kit.pool.get_stats()) == {
            "counters", "totalConnections", "idleConnections",
            "pendingConnections", "waiterCount"}
        await kit.stop()
        with pytest.raises(ValueError):
            LimitKit(loop, {"maxLimit": 17})
        with pytest.raises(TypeError):
            LimitKit(loop, "on")
    run_vt(body)
