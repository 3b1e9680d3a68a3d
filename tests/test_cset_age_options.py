"""``maxConnectionAge`` / ``connectionAgeSpread`` on a ConnectionSet:
validated exactly as on a pool, and off means off."""

import math

import pytest

from cueball_amd.connection_set import ConnectionSet
from cueball_amd.testing import DummyConnection, DummyResolver, settle
from conftest import run_vt
from cset_age_kit import RECOVERY, Kit, instance_vars


def make(loop, **opts):
    base = {"constructor": DummyConnection, "recovery": RECOVERY,
            "target": 1, "maximum": 1, "resolver": DummyResolver(),
            "loop": loop}
    base.update(opts)
    return ConnectionSet(base)


BAD = [
    ({"maxConnectionAge": True}, TypeError),
    ({"maxConnectionAge": "60000"}, TypeError),
    ({"maxConnectionAge": [60000]}, TypeError),
    ({"maxConnectionAge": 0}, ValueError),
    ({"maxConnectionAge": -1}, ValueError),
    ({"maxConnectionAge": math.inf}, ValueError),
    ({"maxConnectionAge": math.nan}, ValueError),
    ({"maxConnectionAge": 1000, "connectionAgeSpread": False}, TypeError),
    ({"maxConnectionAge": 1000, "connectionAgeSpread": "0.2"}, TypeError),
    ({"maxConnectionAge": 1000, "connectionAgeSpread": -0.1}, ValueError),
    ({"maxConnectionAge": 1000, "connectionAgeSpread": 1}, ValueError),
    ({"maxConnectionAge": 1000, "connectionAgeSpread": 1.5}, ValueError),
    ({"maxConnectionAge": 1000, "connectionAgeSpread": math.nan},
     ValueError),
    ({"connectionAgeSpread": 0.2}, ValueError),
]


@pytest.mark.parametrize("opts,exc", BAD, ids=[repr(o) for o, _ in BAD])
def test_bad_options_are_refused(vloop, opts, exc):
    with pytest.raises(exc):
        make(vloop, **opts)


def test_good_options_and_the_default_spread(vloop):
    cset = make(vloop, maxConnectionAge=1000)
    assert cset.cs_age_max == 1000 and cset.cs_age_spread == 0.2
    cset = make(vloop, maxConnectionAge=2.5, connectionAgeSpread=0)
    assert cset.cs_age_max == 2.5 and cset.cs_age_spread == 0
    assert cset.get_connection_ages() == {
        "maxAgeMs": 2.5, "oldestMs": None, "connections": []}


def test_off_means_not_one_attribute_and_not_one_listener():
    async def body(loop):
        kit = Kit(loop)
        cset = kit.cset
        await settle(loop)
        await kit.connect_new()
        assert kit.log == ["added b1.1"]
        assert not any(n.startswith("cs_age") for n in instance_vars(cset))
        # a set with the option, in the same state, has exactly one
        # listener more on the slot's socket manager: the age watch
        with_age = Kit(loop, maxConnectionAge=1000)
        await settle(loop)
        await with_age.connect_new()
        assert with_age.log == ["added b1.1"]
        off = cset.cs_fsm["b1"]
        on = with_age.cset.cs_fsm["b1"]
        assert on.csf_smgr.listener_count("stateChanged") == \
            off.csf_smgr.listener_count("stateChanged") + 1
        assert on.listener_count("stateChanged") == \
            off.listener_count("stateChanged")
        report = cset.get_connection_ages()
        assert report["maxAgeMs"] is None
        assert report["oldestMs"] == 0
        assert report["connections"] == [
            {"backend": "b1", "ckey": "b1.1", "state": "busy", "ageMs": 0,
             "expiresInMs": None, "recycling": False}]
        # reading the report switches nothing on
        assert not any(n.startswith("cs_age") for n in instance_vars(cset))
        await kit.stop()
        await with_age.stop()
    run_vt(body)
