"""The host wrappers of ops hand the library what they handed it before they were folded into one body per entry point:
the call records of tests/ops_call_recorder.py against the golden recorded from the commit before (abfee84)."""
import json
import os

import ops_call_recorder as rec
from conftest import GOLDEN


def test_host_wrappers_reproduce_the_recorded_calls():
    import spline_trajectory_optimization_amd as pkg
    from spline_trajectory_optimization_amd import ops  # noqa: F401
    want = json.load(open(os.path.join(GOLDEN, "ops_calls_host.json")))
    got = json.loads(json.dumps(rec.record_host(pkg)))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_recorder_refuses_what_ctypes_would():
    """The stand-in is as strict as the binding: a wrong argument count or a float for an int does not get recorded."""
    import pytest
    from spline_trajectory_optimization_amd import _lib
    r = rec.Recorder(_lib._SIGNATURES)
    with pytest.raises(AssertionError):
        r.rl_ctx_set_arith(None)
    with pytest.raises(TypeError):
        r.rl_ctx_set_arith(None, 1.0)
    assert r.rl_ctx_set_arith(None, 1) == 0 and r.events[0]["args"] == ["null", ["int", 1]]
