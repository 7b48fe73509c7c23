"""The weighted min-curvature cost without a device: the CPU twin (tests/weighted_twin.py: the weighted cost, and the sweep
built on it, which pins what a weighted sweep kernel will have to reproduce) against the oracle, the ABI, and the argument
checks of the Python layer."""
import os
import re
import types

import numpy as np
import pytest

import weighted_twin as tw
from conftest import ROOT, spline
from oracle import oracle as orc

TAG, N, I_START = "c100", 200, [17]


@pytest.fixture(scope="module")
def unweighted(fits, rings):
    """The twin with w = 1 on c100, N = 200, one outer iteration from control point 17."""
    t, cx, cy, k, length = spline(fits, TAG)
    return tw.sweep_cached(("cpu", "ones"), t, cx, cy, k, length, N, rings[0], rings[1], I_START, np.ones(N))


def test_twin_cost_with_ones_is_the_oracles_cost(fits):
    t, cx, cy, k, _ = spline(fits, TAG)
    with orc.cr_variant():
        for n_samples in (200, 1600):
            for idx in (2, 10, 33, 60, 62, 5, 50):
                z = np.array([cx[idx] + 0.1, cy[idx] - 0.2])
                H, g, M = tw.cost(z, idx, t, cx, cy, k, n_samples, np.ones(n_samples))
                Ho, go, Mo = orc.min_curvature_cost(z, idx, t, cx, cy, k, n_samples)
                assert M == Mo and M > 0
                np.testing.assert_array_equal(H, Ho)
                np.testing.assert_array_equal(g, go)


def test_twin_sweep_with_ones_is_the_oracles_sweep(fits, rings, unweighted):
    t, cx, cy, k, length = spline(fits, TAG)
    with orc.cr_variant():
        ocx, ocy, opts, ons = orc.run_min_curvature_qp(t, cx, cy, k, length, N, rings[0], rings[1], np.array(I_START, dtype=np.int32))
        assert orc.last_raised() == 0
    tcx, tcy, tpts, tns = unweighted
    np.testing.assert_array_equal(tns, ons)
    assert tns.tolist() == [[61, 61]]
    np.testing.assert_array_equal(tcx, ocx); np.testing.assert_array_equal(tcy, ocy)
    np.testing.assert_array_equal(tpts[:, :2], opts[:, :2])


def test_a_constant_power_of_two_changes_no_bit(fits, rings, unweighted):
    t, cx, cy, k, length = spline(fits, TAG)
    q = tw.sweep_cached(("cpu", "quarter"), t, cx, cy, k, length, N, rings[0], rings[1], I_START, np.full(N, 0.25))
    for a, b in zip(q, unweighted):
        np.testing.assert_array_equal(a, b)


def test_nonuniform_weights_move_the_line(fits, rings, unweighted):
    """What the GPU tests count on: the weights matter by far more than their 1e-3 m threshold."""
    t, cx, cy, k, length = spline(fits, TAG)
    w = tw.case_weights(N)[2]
    s = tw.sweep_cached(("cpu", "smooth"), t, cx, cy, k, length, N, rings[0], rings[1], I_START, w)
    moved = float(np.abs(s[2][:, :2] - unweighted[2][:, :2]).max())
    print("1/linspace(20, 80): line moved by", moved, "m")
    assert moved > 0.1


# ------------------------------------------------------------------------------------------------ ABI
NEW = ("rl_mincurv_cost_weighted",)


def test_abi_is_additive():
    from spline_trajectory_optimization_amd import _lib
    header = open(os.path.join(ROOT, "include", "rl_mincurv.h")).read()
    lib = _lib.load()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, bare)
        assert decl and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == decl.group(1).count(",") + 1
    assert len(_lib._SIGNATURES["rl_mincurv_cost_weighted"][1]) == 9
    assert re.search(r"#define RL_VERSION 103\b", header) and lib.rl_version() == 103


# ------------------------------------------------------------------------------------------------ argument checks, no device
def fake_track(n=66, n_samples=N, k=5):
    return types.SimpleNamespace(ctx=None, h=None, n=n, N=n_samples, k=k)


def test_ops_checks_weights_before_anything_runs():
    from spline_trajectory_optimization_amd import _lib, ops
    trk = fake_track()
    for bad_shape in (np.ones(N + 1), np.ones((3, N)), np.ones((N, 1))):
        with pytest.raises(ValueError, match="weights: expected shape"):
            ops.mincurv_cost(trk, [10], weights=bad_shape)
    for bad_value in (np.nan, np.inf, 0.0, -1.0, 2.0 ** 31, 2.0 ** -31):
        w = np.ones(N); w[7] = bad_value
        with pytest.raises(ValueError, match="finite and within"):
            ops.mincurv_cost(trk, [10], weights=w)
    assert (_lib.WEIGHT_MIN, _lib.WEIGHT_MAX) == (2.0 ** -30, 2.0 ** 30)


def test_speed_weights_need_a_simulated_table():
    """A table fresh from sample_along has SPEED = 0: ValueError."""
    from spline_trajectory_optimization_amd.models.trajectory import Trajectory
    from spline_trajectory_optimization_amd.optimization.optimizer import TrajectoryOptimizer
    tab = Trajectory(N)
    with pytest.raises(ValueError, match="SPEED"):
        TrajectoryOptimizer.speed_weights(tab)
    for bad in (np.nan, np.inf, -3.0):
        tab.points[:, Trajectory.SPEED] = 40.0
        tab.points[5, Trajectory.SPEED] = bad
        with pytest.raises(ValueError, match="SPEED"):
            TrajectoryOptimizer.speed_weights(tab)
    tab.points[:, Trajectory.SPEED] = np.linspace(20.0, 80.0, N)
    np.testing.assert_array_equal(TrajectoryOptimizer.speed_weights(tab), 1.0 / np.linspace(20.0, 80.0, N))

