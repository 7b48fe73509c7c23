"""The weighted min-curvature cost on the device: rl_mincurv_cost_weighted through ops.mincurv_cost(weights=) and
TrajectoryOptimizer.min_curvature_cost(weights=).  Need a real MI355X:  pytest -m gpu

Reference: tests/weighted_twin.py (the oracle's pieces with the weighted cost loop in Python floats; pinned to the oracle in
tests/test_weighted_sweep_cpu.py).  Reference-order arithmetic: bit for bit.  Fast arithmetic: the tolerance
tests/test_hip_parity.py holds rl_mincurv_cost to.  Shapes: c100 (n = 66, k = 5), N = 200, and N = 1600 where the widest support
spans more than one chunk of 256 cost terms.

The weighted SWEEP (the issue's rl_mincurv_solve_batch_weighted_*) is not part of this change: see DESIGN.md section 6j."""
import numpy as np
import pytest

import weighted_twin as tw
from conftest import spline
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
FAST, REF = 0, 1
TAG, N = "c100", 200
TERM_CHUNK = 256                     # csrc/rl_kernels.hpp: kTermChunkA
IDX = (2, 10, 33, 60, 62, 5, 50)     # at N = 1600 control point 2 fills a chunk of cost terms exactly (256), 5 and 50 cross it (268, 277)


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    ctx = _lib.Context.get(0)
    ctx.set_arith(_lib.ARITH_DEFAULT)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch, ns.ctx = _lib, ops, batch, ctx
    assert (_lib.ARITH_FAST, _lib.ARITH_REFERENCE) == (FAST, REF)
    return ns


def track(rl, fits, rings, n_samples=N):
    t, cx, cy, k, _ = spline(fits, TAG)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, n_samples)
    trk.set_rings(rings[0], rings[1])
    return trk


# ------------------------------------------------------------------------------------------------ 1. the cost entry
@pytest.mark.parametrize("n_samples", [200, 1600])
def test_weighted_cost_entry(rl, fits, rings, n_samples):
    t, cx, cy, k, _ = spline(fits, TAG)
    trk = track(rl, fits, rings, n_samples)
    idx = np.array(IDX)
    z = np.stack([cx[idx] + 0.1, cy[idx] - 0.2], axis=1)
    w = np.exp2(np.random.default_rng(3).uniform(-3.0, 3.0, n_samples))
    with orc.cr_variant():
        twin = [tw.cost(z[j], int(i), t, cx, cy, k, n_samples, w) for j, i in enumerate(idx)]
        plain = [tw.cost(z[j], int(i), t, cx, cy, k, n_samples, np.ones(n_samples)) for j, i in enumerate(idx)]
    with rl.ctx.arith(REF):
        H, g, M = rl.ops.mincurv_cost(trk, idx, z=z, weights=w)
        H1, g1, _ = rl.ops.mincurv_cost(trk, idx, z=z, weights=np.ones(n_samples))
        H0, g0, _ = rl.ops.mincurv_cost(trk, idx, z=z)
    np.testing.assert_array_equal(H1, H0); np.testing.assert_array_equal(g1, g0)
    for j in range(len(idx)):
        assert M[j] == twin[j][2]
        np.testing.assert_array_equal(H[j], twin[j][0]); np.testing.assert_array_equal(g[j], twin[j][1])
        assert not np.array_equal(twin[j][0], plain[j][0])
    with rl.ctx.arith(FAST):   # the tolerance tests/test_hip_parity.py holds rl_mincurv_cost to against the oracle
        H, g, _ = rl.ops.mincurv_cost(trk, idx, z=z, weights=w)
        H1, g1, _ = rl.ops.mincurv_cost(trk, idx, z=z, weights=np.ones(n_samples))
        H0, g0, _ = rl.ops.mincurv_cost(trk, idx, z=z)
    np.testing.assert_array_equal(H1, H0); np.testing.assert_array_equal(g1, g0)
    for j in range(len(idx)):
        np.testing.assert_allclose(H[j], twin[j][0], rtol=1e-10)
        assert np.all(np.abs(g[j] - twin[j][1]) <= 1e-8 * np.abs(twin[j][1]).max())


def test_weights_cross_a_term_chunk(fits):
    """The N = 1600 case above holds a support of exactly one chunk of cost terms and two that cross it; N = 200 has neither."""
    t, cx, cy, k, _ = spline(fits, TAG)
    sizes = {idx: len(tw.support(t, k, idx, 1600)) for idx in IDX}
    assert sizes[2] == TERM_CHUNK and sizes[5] == 268 and sizes[50] == 277, sizes
    assert max(len(tw.support(t, k, idx, 200)) for idx in IDX) < TERM_CHUNK


def test_bad_host_weights_are_refused(rl, fits, rings):
    """The entry point itself (ops refuses such weights before it is reached): NaN, inf, 0, -1, 2^31 and NULL give RL_ERR_ARG."""
    import ctypes
    t, cx, cy, k, _ = spline(fits, TAG)
    trk = track(rl, fits, rings)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    idx = np.array([10], dtype=np.int32)
    H = np.zeros(4); g = np.zeros(2); M = np.zeros(1, dtype=np.int32)
    call = lambda wp: rl.ctx.lib.rl_mincurv_cost_weighted(rl.ctx.h, trk.h, idx.ctypes.data_as(ip), 1, None, wp,  # noqa: E731
                                                          H.ctypes.data_as(dp), g.ctypes.data_as(dp), M.ctypes.data_as(ip))
    for bad in (np.nan, np.inf, 0.0, -1.0, 2.0 ** 31):
        w = np.ones(N); w[123] = bad
        assert call(w.ctypes.data_as(dp)) == -1, bad
    assert call(None) == -1
    w = np.ones(N)
    assert call(w.ctypes.data_as(dp)) == 0 and M[0] > 0


def test_the_drop_in_takes_weights(rl, fits, rings):
    """TrajectoryOptimizer.min_curvature_cost(weights=1 / SPEED): the twin's bits (the class answers in reference-order)."""
    from scipy import interpolate
    from spline_trajectory_optimization_amd.models.trajectory import BSplineTrajectory, Trajectory
    from spline_trajectory_optimization_amd.optimization.optimizer import TrajectoryOptimizer
    t, cx, cy, k, length = spline(fits, TAG)
    spl = object.__new__(BSplineTrajectory)
    spl._spl_x = interpolate.BSpline(t, cx.copy(), k); spl._spl_y = interpolate.BSpline(t, cy.copy(), k); spl._length = length
    optm = object.__new__(TrajectoryOptimizer)
    optm._trk_cache = {}
    tab = Trajectory(N)
    tab.points[:, Trajectory.SPEED] = np.linspace(20.0, 80.0, N)
    w = TrajectoryOptimizer.speed_weights(tab)
    z = np.array([cx[33] + 0.1, cy[33] - 0.2])
    H, g = optm.min_curvature_cost(z, 33, spl, tab, weights=w)
    H1, g1 = optm.min_curvature_cost(z, 33, spl, tab)
    with orc.cr_variant():
        Ht, gt, _ = tw.cost(z, 33, t, cx, cy, k, N, w)
        Ho, go, _ = orc.min_curvature_cost(z, 33, t, cx, cy, k, N)
    np.testing.assert_array_equal(H, Ht); np.testing.assert_array_equal(g, gt)
    np.testing.assert_array_equal(H1, Ho); np.testing.assert_array_equal(g1, go)
    assert not np.array_equal(H, H1)
