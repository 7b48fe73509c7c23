"""The torch wrappers of ops against the call records of the commit before they shared a body with the host forms (abfee84),
with real cuda tensors and the recording stand-in for the library: no kernel is launched."""
import json
import os

import pytest

import ops_call_recorder as rec
from conftest import GOLDEN


@pytest.mark.gpu
def test_torch_wrappers_reproduce_the_recorded_calls_and_match_the_host_forms():
    import spline_trajectory_optimization_amd as pkg
    from spline_trajectory_optimization_amd import _lib, ops  # noqa: F401
    want = json.load(open(os.path.join(GOLDEN, "ops_calls_torch.json")))
    got = json.loads(json.dumps(rec.record_torch(pkg)))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name   # the "@other_device" entries: refused wherever it was refused before
    host = rec.record_host(pkg)
    for name in rec.strict_cases(_lib):
        rec.same_marshalling(host[name], got[name])
        for where, raised in got[name + "@other_device"].items():
            assert raised in (None, "ValueError"), (name, where, raised)
