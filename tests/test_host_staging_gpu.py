"""The host-pointer entry points stage their buffers through one object (csrc/rl_host.hpp: Staging).  What it must keep:
the host route returns the device route's bits, an output the caller declines changes nothing else, and a call that fails
after staging has begun gives its blocks back to the pool.

Everything runs on the smallest fixture the sweep is tested on: the Monza fit `c100` at N = 200 with the three-iteration order
of G7 `c100_N200_it3_seed1` (the global QPs on the smallest track tests/test_global_qp.py runs them on, `c100` at N = 500)."""
import numpy as np
import pytest

from conftest import golden, spline
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

N, B = 200, 3
KEY = "c100_N200_it3_seed1"


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch = _lib, ops, batch
    return ns


def half_widths(rl, fits, rings, n_samples):
    t, cx, cy, k, length = spline(fits, "c100")
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, n_samples, endpoint=False))
    orc.fill_bounds(pts, rings[0], rings[1], 100.0)
    return rl.batch.half_widths_from_bounds(pts)


@pytest.fixture(scope="module")
def case(rl, fits, rings):
    """(spline, widths [B,N,2] of batch.width_batch, i_start of the G7 run) -- shared, never written to."""
    wl, wr = half_widths(rl, fits, rings, N)
    widths = np.ascontiguousarray(rl.batch.width_batch(wl, wr, B, seed=1234))
    widths.setflags(write=False)
    return spline(fits, "c100"), widths, golden("G7_run_min_curvature_qp.npz")[f"{KEY}_i_start"]


def new_track(rl, case, with_rings=None):
    (t, cx, cy, k, _), _, _ = case
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    if with_rings is not None:
        trk.set_rings(*with_rings)
    return trk


@pytest.mark.parametrize("arith", ["default", "fast"])
def test_sweep_host_route_equals_device_route(rl, case, arith):
    import torch
    _, widths, i_start = case
    arith = None if arith == "default" else rl.lib.ARITH_FAST
    trk = new_track(rl, case)
    ctrl, xy, ns, status, st = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, i_start, arith=arith)
    out = rl.ops.solve_batch_torch(trk, rl.lib.BOUNDS_WIDTHS, torch.from_numpy(np.array(widths)).cuda(), i_start, arith=arith)
    torch.cuda.synchronize()
    assert out["stats"].reserved[0] == st.reserved[0] == (rl.lib.ARITH_REFERENCE if arith is None else rl.lib.ARITH_FAST)
    assert np.array_equal(out["ctrl"].cpu().numpy(), ctrl)
    assert np.array_equal(out["xy"].cpu().numpy(), xy)
    assert np.array_equal(out["n_success"].cpu().numpy(), ns)
    assert np.array_equal(out["status"].cpu().numpy(), status)
    assert np.isfinite(ctrl).all() and ns.sum() > 0


@pytest.mark.parametrize("dof", [1, 2])
def test_global_qp_declined_xy_changes_nothing_else(rl, fits, rings, dof):
    t, cx, cy, k, _ = spline(fits, "c100")
    wl, wr = half_widths(rl, fits, rings, 500)
    W = rl.batch.width_batch(wl, wr, B, seed=3)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, 500)
    ctrl, xy, off, st, _ = rl.ops.global_batch_host(trk, W, 0.5, 3, want_xy=True, dof=dof)
    ctrl2, xy2, off2, st2, _ = rl.ops.global_batch_host(trk, W, 0.5, 3, want_xy=False, dof=dof)
    assert xy is not None and np.isfinite(xy).all() and xy2 is None
    assert np.array_equal(ctrl2, ctrl) and np.array_equal(off2, off) and np.array_equal(st2, st)
    assert np.abs(off).max() > 0.0


def test_sweep_declined_points_changes_nothing_else(rl, case, rings):
    (t, cx, cy, k, length), _, i_start = case
    trk = new_track(rl, case, rings)
    trk.set_length(length)
    cx1, cy1, pts, ns1, _ = rl.ops.mincurv_sweep(trk, cx, cy, i_start, want_points=True)
    cx2, cy2, none, ns2, _ = rl.ops.mincurv_sweep(trk, cx, cy, i_start, want_points=False)
    assert pts is not None and np.isfinite(pts).all() and none is None
    assert np.array_equal(cx2, cx1) and np.array_equal(cy2, cy1) and np.array_equal(ns2, ns1)
    assert not np.array_equal(cx1, cx) and ns1.sum() > 0


def test_failed_call_gives_its_staging_blocks_back(rl, case):
    _, widths, i_start = case
    trk = new_track(rl, case)       # no rings
    solve = lambda: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, i_start)   # noqa: E731
    ctrl, xy, ns, status, _ = solve()
    tables = lambda: rl.ops.tables_host(trk, ctrl, rl.lib.BOUNDS_WIDTHS, np.array(widths), 5793.0)   # noqa: E731
    pts = tables()
    assert np.isfinite(ctrl).all() and np.isfinite(pts).all()
    # fails inside the _dev entry, behind the copies of `ctrl` to the device
    with pytest.raises(rl.lib.RlError, match="rl_track_set_rings was not called"):
        rl.ops.tables_host(trk, ctrl, rl.lib.BOUNDS_SHARED_RINGS, None, 5793.0)
    # fails in the sweep's argument checks, behind the allocations and the copy of the widths
    bad = np.array(i_start)
    bad[1] = trk.n
    with pytest.raises(rl.lib.RlError, match="i_start outside"):
        rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, bad)
    ctrl2, xy2, ns2, status2, _ = solve()
    assert np.array_equal(ctrl2, ctrl) and np.array_equal(xy2, xy) and np.array_equal(ns2, ns) and np.array_equal(status2, status)
    assert np.array_equal(tables(), pts)
