"""Tables of a solved batch, what can be checked without a device: the CPU twin against the reference-generated fixtures, the
C ABI's declarations against the Python binding, the argument checks of the wrappers, the summary twin."""
import os
import re
import types

import numpy as np
import pytest

import tables_twin as tw
from conftest import ROOT, golden, spline

ENTRY_POINTS = ("rl_tables_batch_dev", "rl_tables_batch_host", "rl_table_summary_dev", "rl_table_summary_host")


@pytest.mark.parametrize("N", [500, 2000])
def test_twin_reproduces_the_reference_fixtures(fits, rings, N):
    """The yardstick is pinned to the reference before anything is judged by it (tolerances of
    tests/test_hip_parity.py::test_sample_along_golden / ::test_fill_bounds)."""
    t, cx, cy, k, length = spline(fits, "c100")
    pts = tw.table(t, cx, cy, k, length, N, rings[0], rings[1])
    ref = golden("G2_sample_along.npz")[f"N{N}_cols"]
    np.testing.assert_allclose(pts[:, [0, 1]], ref[:, :2], rtol=0, atol=1e-10)
    np.testing.assert_allclose(pts[:, 3], ref[:, 2], rtol=0, atol=1e-13)
    np.testing.assert_allclose(pts[:, 5], ref[:, 3], rtol=1e-10)
    atol = 1e-9 if N >= 2000 else 1e-7   # scipy's quad bisects at N = 500
    np.testing.assert_allclose(pts[:, 6], ref[:, 4], rtol=0, atol=atol)
    np.testing.assert_allclose(pts[:, 7], ref[:, 5], rtol=0, atol=atol)
    assert np.all(pts[:, 17] == np.arange(N)) and np.all(pts[:, 18] == -1) and not pts[:, tw.ZERO_COLS + [13]].any()
    if N == 500:
        np.testing.assert_allclose(pts[:, 9:13], golden("G4_track_constraint.npz")["c100_N500_bounds"], rtol=0, atol=1e-10)


def test_header_declares_and_binding_matches():
    """The four entry points are declared, and _lib binds each with the declaration's number of parameters."""
    from spline_trajectory_optimization_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rl_mincurv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/rl_mincurv.h"
        assert name in _lib._SIGNATURES, f"{name} is not bound in _lib.py"
        res, args = _lib._SIGNATURES[name]
        assert len(args) == len(m.group(1).split(",")), name
    assert len(_lib._SIGNATURES["rl_tables_batch_dev"][1]) == 10 and len(_lib._SIGNATURES["rl_table_summary_dev"][1]) == 6


def _fake_track(n=66, N=40):
    return types.SimpleNamespace(n=n, N=N, k=5, ctx=None, h=None)


def test_wrappers_reject_bad_arguments_before_any_device_call():
    """ctx = None in the stand-in track: anything that got as far as the library would raise AttributeError, not these."""
    from spline_trajectory_optimization_amd import _lib, batch, ops
    trk = _fake_track()
    ctrl = np.zeros((3, trk.n, 2)); w = np.ones((3, trk.N, 2))
    bad = [
        dict(ctrl=np.zeros((3, trk.n + 1, 2)), bounds=w),                      # wrong shape
        dict(ctrl=ctrl.astype(np.float32), bounds=w),                          # wrong dtype
        dict(ctrl=np.zeros((3, trk.n, 4))[:, :, ::2], bounds=w),               # not contiguous
        dict(ctrl=ctrl, bounds=np.ones((3, trk.N, 4))),                        # points where widths are announced
        dict(ctrl=ctrl, bounds=None),                                          # widths without bounds
        dict(ctrl=ctrl, bounds=w, bank=np.zeros(trk.N + 1)),                   # bank of the wrong length
        dict(ctrl=ctrl, bounds=w, bank=np.zeros((2, trk.N))),
        dict(ctrl=np.zeros((trk.n, 2)), bounds=w),                             # no batch axis
    ]
    veh = (np.zeros(3), np.zeros((4, 2)), np.zeros(3), np.zeros((4, 2)), np.zeros(6))
    for kw in bad:
        with pytest.raises((AssertionError, ValueError)):
            ops.tables_host(trk, kw["ctrl"], _lib.BOUNDS_WIDTHS, kw["bounds"], 100.0, bank=kw.get("bank"))
        with pytest.raises((AssertionError, ValueError)):
            batch.lap_times_host(trk, kw["ctrl"], _lib.BOUNDS_WIDTHS, kw["bounds"], 100.0, veh, bank=kw.get("bank"))
    with pytest.raises((AssertionError, ValueError)):
        ops.tables_host(trk, ctrl, _lib.BOUNDS_SHARED_RINGS, w, 100.0)          # shared rings take no bounds
    with pytest.raises((AssertionError, ValueError)):
        ops.tables_host(trk, ctrl, 7, w, 100.0)
    with pytest.raises((AssertionError, ValueError)):
        batch.lap_times_host(trk, ctrl, _lib.BOUNDS_WIDTHS, w, 100.0, (1, 2, 3))   # not a vehicle
    for pts in (np.zeros((2, 10, 18)), np.zeros((10, 19)), np.zeros((2, 10, 19), dtype=np.float32),
                np.zeros((2, 10, 38))[:, :, ::2]):
        with pytest.raises((AssertionError, ValueError)):
            ops.table_summary(pts)
    with pytest.raises((AssertionError, ValueError)):
        ops.table_summary(np.zeros((2, 10, 19)), iters=np.zeros(2, dtype=np.int64))
    with pytest.raises((AssertionError, ValueError)):
        ops.table_summary(np.zeros((2, 10, 19)), iters=np.zeros(3, dtype=np.int32))
    # the torch forms: host tensors, wrong dtype, wrong shape
    import torch
    tc, tw_ = torch.zeros((3, trk.n, 2), dtype=torch.float64), torch.ones((3, trk.N, 2), dtype=torch.float64)
    with pytest.raises((AssertionError, ValueError)):
        ops.tables_torch(trk, tc, _lib.BOUNDS_WIDTHS, tw_, 100.0)
    with pytest.raises((AssertionError, ValueError)):
        batch.lap_times_torch(trk, tc, _lib.BOUNDS_WIDTHS, tw_, 100.0, veh)
    with pytest.raises((AssertionError, ValueError)):
        ops.table_summary_torch(torch.zeros((2, 10, 19), dtype=torch.float64))
    with pytest.raises((AssertionError, ValueError)):
        ops.table_summary_torch(torch.zeros((10, 19), dtype=torch.float64))
    assert len(ops.SUMMARY_COLUMNS) == 8 and ops.SUMMARY_COLUMNS[0] == "lap_time"


def test_summary_twin_equals_the_simulator_summary():
    """The seven fields the summary shares with SimulationResult, on the reference's own simulated table (G6): equal exactly."""
    try:
        from spline_trajectory_optimization_amd.models.trajectory import Trajectory
        from spline_trajectory_optimization_amd.simulator import simulator
    except Exception as e:   # the package needs no device to import (tests/test_host_cpu.py); anything else is reported
        pytest.skip(f"package not importable here: {e}")
    g = golden("G6_simulator.npz")
    N = len(g["speed"])
    traj = Trajectory(N)
    traj.points[:, [0, 1, 5, 6, 7, 13]] = g["cols_in"]
    traj.points[:, 4] = g["speed"]; traj.points[:, 14] = g["lon_acc"]; traj.points[:, 15] = g["lat_acc"]
    traj.points[:, 16] = g["time"]; traj.points[:, 18] = g["iter_flag"]
    r = simulator._summarise(traj, 0.0)
    s = tw.summary(traj.points)
    assert [r.total_time, r.average_speed, r.max_speed, r.min_speed, r.max_lat_acc, r.max_lon_acc, r.max_lon_dcc] == list(s[1:])
    assert s[0] == np.cumsum(g["time"])[-1] and s[0] > 10 * s[1]
    ref = g["summary"]   # the reference's own result object: total_time, average_speed, max / min speed, max lat, max / min lon
    np.testing.assert_allclose(s[1:], ref, rtol=1e-12)
