"""The sparse-support cases of tests/sparse_cases.py, on the CPU: that they reach the edges they are meant to reach (empty and
small supports, the sizes around the in-order sums' unrolling), and the convention the GPU tests rely on -- the CR oracle runs
every case to the end with finite output, and an empty support is always a failed step."""
import numpy as np
import pytest

from conftest import spline
from oracle import oracle as orc
from sparse_cases import CASES, NO_EMPTY, UNROLL_EDGES, case_id, empty_points, i_start, support_sizes


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_has_a_small_support(fits, case):
    tag, N = case
    t, cx, cy, k, length = spline(fits, tag)
    idx, m = support_sizes(t, k, len(cx), N)
    assert m.min() < 8, (case, m.min())
    if case in NO_EMPTY:
        assert m.min() > 0
    else:
        assert (m == 0).any(), case


def test_the_cases_cover_the_edges_of_the_unrolled_sums(fits):
    seen = set()
    for tag, N in CASES:
        t, cx, cy, k, length = spline(fits, tag)
        seen |= set(support_sizes(t, k, len(cx), N)[1].tolist())
    missing = UNROLL_EDGES - seen
    assert not missing, sorted(missing)


def test_support_sizes_match_the_mask_written_out(fits):
    """The helper's mask against the reference's expression with a scalar loop (t[idx] <= u < t[idx + k + 1])."""
    t, cx, cy, k, length = spline(fits, "c0p8")
    N = 48
    idx, m = support_sizes(t, k, len(cx), N)
    ts = np.linspace(0.0, 1.0, N, endpoint=False)
    for i, mi in zip(idx, m):
        assert mi == sum(1 for u in ts if t[i] <= u < t[i + k + 1])
    np.testing.assert_array_equal(empty_points(t, k, len(cx), N), [11, 12, 13, 14, 54, 147])


def _widths(fits, rings, tag, N, B, seed):
    from spline_trajectory_optimization_amd import batch
    t, cx, cy, k, length = spline(fits, tag)
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    orc.fill_bounds(pts, rings[0], rings[1], 100.0)
    wl, wr = batch.half_widths_from_bounds(pts)
    return batch.width_batch(wl, wr, B, seed=seed)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_oracle_runs_the_sparse_cases(fits, rings, case):
    """An empty support is a failed step: per pass at most steps - #empty supports succeed, on the shared Monza rings and on
    width-built rings; nothing non-finite comes out."""
    tag, N = case
    t, cx, cy, k, length = spline(fits, tag)
    n = len(cx)
    steps = n - k
    n_empty = len(empty_points(t, k, n, N))
    ist = i_start(n, k, N)
    with orc.cr_variant():
        ocx, ocy, opts, ons = orc.run_min_curvature_qp(t, cx, cy, k, length, N, rings[0], rings[1], ist)
        widths = _widths(fits, rings, tag, N, 4, seed=N)
        octrl, oxy, wns = orc.solve_width_batch(t, cx, cy, k, length, N, widths, ist, nthreads=4)
    assert ons.shape == (len(ist), 2) and wns.shape == (4, len(ist), 2)
    assert np.isfinite(ocx).all() and np.isfinite(ocy).all() and np.isfinite(opts[:, :2]).all()
    assert np.isfinite(octrl).all() and np.isfinite(oxy).all()
    assert (ons <= steps - n_empty).all() and (wns <= steps - n_empty).all(), (ons, wns.max(), steps, n_empty)
    assert ons.sum() > 0 and (wns.sum(axis=(1, 2)) > 0).all()   # the sweep does move the line
