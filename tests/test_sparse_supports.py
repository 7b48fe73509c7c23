"""The sweep on SPARSE samplings (tests/sparse_cases.py): grid sizes at which free control points have empty supports or
supports of a few samples.  Dense samplings (every other test) never take these paths: the step with no support samples
(no chunk of the reference-order cost pass runs), the tail of the in-order sums' unrolling, width-built rings too short for the
windowed search (N <= 48) or for its staged stretch (48 < N < 96), N below one wave and N odd.

The reference-order arithmetic is held to the CR oracle's bits, as in tests/test_reference_order.py; the fast and branch
arithmetics to the nearest-branch rule of tests/parity_rule.py, the branch arithmetic also to its own bits across residencies
and search modes."""
import numpy as np
import pytest

from conftest import spline
from oracle import oracle as orc
from sparse_cases import CASES, NO_EMPTY, case_id, empty_points, i_start, support_sizes

pytestmark = pytest.mark.gpu
REF = 1  # _lib.ARITH_REFERENCE


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    _lib.Context.get(0)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch = _lib, ops, batch
    assert _lib.ARITH_REFERENCE == REF
    return ns


def _case(fits, case):
    """Spline, sweep order and the case's own edge: an empty support (or, for the one case without, a small one)."""
    tag, N = case
    t, cx, cy, k, length = spline(fits, tag)
    n = len(cx)
    idx, m = support_sizes(t, k, n, N)
    n_empty = int((m == 0).sum())
    assert (n_empty == 0) == (case in NO_EMPTY) and m.min() < 8, (case, n_empty, m.min())
    return t, cx, cy, k, length, i_start(n, k, N), n_empty


def _widths(rl, fits, rings, tag, N, B, seed):
    t, cx, cy, k, length = spline(fits, tag)
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    orc.fill_bounds(pts, rings[0], rings[1], 100.0)
    wl, wr = rl.batch.half_widths_from_bounds(pts)
    return rl.batch.width_batch(wl, wr, B, seed=seed)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_single_sweep_sparse_bitwise(rl, fits, rings, monkeypatch, case):
    """Reference-order single sweep on the Monza rings, two outer iterations: the CR oracle's control points, success counts and
    table columns -- with the state in global scratch and in LDS, and in each of the three search modes."""
    tag, N = case
    t, cx, cy, k, length, ist, n_empty = _case(fits, case)
    steps = len(cx) - k
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    trk.set_rings(rings[0], rings[1])
    with orc.cr_variant():
        ocx, ocy, opts, ons = orc.run_min_curvature_qp(t, cx, cy, k, length, N, rings[0], rings[1], ist)
    assert (ons <= steps - n_empty).all() and ons.sum() > 0
    for residency in ("0", "1"):
        monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
        hcx, hcy, pts, ns, st = rl.ops.mincurv_sweep(trk, cx, cy, ist, arith=REF)
        assert st.rings_in_lds == int(residency) and st.reserved[0] == REF
        label = f"{case} residency {residency}"
        np.testing.assert_array_equal(ns, ons, err_msg=label)
        np.testing.assert_array_equal(hcx, ocx, err_msg=label); np.testing.assert_array_equal(hcy, ocy, err_msg=label)
        for col in (0, 1, 3, 5, 9, 10, 11, 12):
            np.testing.assert_array_equal(pts[:, col], opts[:, col], err_msg=f"{label} column {col}")
        for search in (0, 1, 2):
            ctrl, xy, ns2, status, st = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_SHARED_RINGS, None, ist, search=search, B=2,
                                                                arith=REF)
            label = f"{case} residency {residency} search {search}"
            for b in range(2):
                np.testing.assert_array_equal(ns2[b], ons, err_msg=label)
                np.testing.assert_array_equal(ctrl[b, :, 0], ocx, err_msg=label)
                np.testing.assert_array_equal(ctrl[b, :, 1], ocy, err_msg=label)
                np.testing.assert_array_equal(xy[b], opts[:, :2], err_msg=label)
            np.testing.assert_array_equal(status, 2 * len(ist) * steps - ns2.reshape(2, -1).sum(axis=1))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_width_batch_sparse_bitwise(rl, fits, rings, monkeypatch, case):
    """Reference-order width batch (rings built from per-sample widths: ring length N, so N <= 48 takes the brute-force search
    in place of the windowed one, and 48 < N < 96 is below the staged stretch of global residency) in both residencies and
    the three search modes: the CR oracle's bits, status = steps - successes.  c0p8 / 48 also through the default arithmetic."""
    tag, N = case
    t, cx, cy, k, length, ist, n_empty = _case(fits, case)
    B = 16
    steps = 2 * len(ist) * (len(cx) - k)
    widths = _widths(rl, fits, rings, tag, N, B, seed=N)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    with orc.cr_variant():
        octrl, oxy, ons = orc.solve_width_batch(t, cx, cy, k, length, N, widths, ist, nthreads=16)
    assert (ons <= (len(cx) - k) - n_empty).all()
    for residency in ("0", "1"):
        monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
        for search in (0, 1, 2):
            ctrl, xy, ns, status, st = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, search=search, arith=REF)
            assert st.rings_in_lds == int(residency) and st.reserved[0] == REF
            label = f"{case} residency {residency} search {search}"
            np.testing.assert_array_equal(ns, ons, err_msg=label)
            np.testing.assert_array_equal(ctrl, octrl, err_msg=label)
            np.testing.assert_array_equal(xy, oxy, err_msg=label)
            np.testing.assert_array_equal(status, steps - ns.reshape(B, -1).sum(axis=1), err_msg=label)
        if case == ("c0p8", 48):   # nothing chosen on the context: the default (reference-order) arithmetic
            ctrl, xy, ns, status, st = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist)
            assert st.reserved[0] == REF
            np.testing.assert_array_equal(ns, ons); np.testing.assert_array_equal(ctrl, octrl)
            np.testing.assert_array_equal(xy, oxy)


@pytest.mark.parametrize("case", [("c100", 46), ("c0p8", 48), ("c0p8", 179)], ids=case_id)
def test_sliding_window_driver_sparse_bitwise(rl, fits, rings, case):
    """run_joint_min_curvature_qp in the reference-order arithmetic, windows that hold empty supports: the CR oracle's bits."""
    tag, N = case
    t, cx, cy, k, length, ist, n_empty = _case(fits, case)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    trk.set_rings(rings[0], rings[1])
    hcx, hcy, _, ns, st = rl.ops.mincurv_sweep_joint(trk, cx, cy, ist, want_points=False, arith=REF)
    assert st.reserved[0] == REF
    with orc.cr_variant():
        ocx, ocy, _, ons = orc.run_joint_min_curvature_qp(t, cx, cy, k, length, N, rings[0], rings[1], ist)
    np.testing.assert_array_equal(ns, ons)
    np.testing.assert_array_equal(hcx, ocx); np.testing.assert_array_equal(hcy, ocy)


def test_cost_and_constraint_on_empty_supports_bitwise(rl, fits, rings):
    """rl_mincurv_cost / rl_track_constraint under RL_ARITH_REFERENCE at c0p8 / 48, every free control point: the oracle's bits,
    and at the six empty supports M = 0, H = g = 0 exactly and no rows -- without an error."""
    t, cx, cy, k, length = spline(fits, "c0p8")
    N = 48
    ctx = rl.lib.Context.get(0)
    trk = rl.lib.Track(ctx, t, cx, cy, k, N)
    idx = np.arange(2, len(cx) - 3)
    empty = set(empty_points(t, k, len(cx), N).tolist())
    assert len(empty) == 6
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    orc.fill_bounds(pts, rings[0], rings[1], 100.0)
    rng = np.random.default_rng(7)
    z = np.stack([cx[idx], cy[idx]], axis=1) + rng.normal(0.0, 2.0, (len(idx), 2))
    with ctx.arith(REF):
        H, g, M = rl.ops.mincurv_cost(trk, idx, z=z)
        rows = [rl.ops.track_constraint(trk, pts, int(i)) for i in idx]
    small = 0
    for q, i in enumerate(idx):
        oH, og, oM = orc.min_curvature_cost(z[q], int(i), t, cx, cy, k, N)
        assert M[q] == oM, i
        np.testing.assert_array_equal(H[q], oH, err_msg=f"H of control point {i}")
        np.testing.assert_array_equal(g[q], og, err_msg=f"g of control point {i}")
        A, lba, uba = rows[q]
        oA, olba, ouba = orc.track_constraint(int(i), t, cx, cy, k, pts)
        np.testing.assert_array_equal(A, oA); np.testing.assert_array_equal(lba, olba); np.testing.assert_array_equal(uba, ouba)
        assert A.shape == (2 * M[q], 2)
        if i in empty:
            assert M[q] == 0 and (H[q] == 0.0).all() and (g[q] == 0.0).all() and len(lba) == 0, i
        small += int(0 < M[q] < 8)
    assert small > 0


def _branch_and_fast(rl, fits, rings, monkeypatch, case, B, judge):
    from parity_rule import ParityOracle, batch_parity
    tag, N = case
    t, cx, cy, k, length, ist, n_empty = _case(fits, case)
    widths = _widths(rl, fits, rings, tag, N, B, seed=N + 1)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    BR = rl.lib.ARITH_BRANCH
    res = {}
    for residency in ("0", "1"):
        monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
        for search in (0, 1, 2):
            r = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, search=search, arith=BR)
            assert r[4].reserved[0] == BR and r[4].rings_in_lds == int(residency)
            res[(residency, search)] = r
    monkeypatch.delenv("RL_FORCE_RESIDENCY")
    first = res[("0", 2)]
    for key, r in res.items():
        np.testing.assert_array_equal(r[0], first[0], err_msg=str(key)); np.testing.assert_array_equal(r[1], first[1], err_msg=str(key))
        np.testing.assert_array_equal(r[2], first[2], err_msg=str(key))
    fast = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, arith=rl.lib.ARITH_FAST)
    assert fast[4].reserved[0] == rl.lib.ARITH_FAST
    np.testing.assert_array_equal(fast[3], 2 * len(ist) * (len(cx) - k) - fast[2].reshape(B, -1).sum(axis=1))
    assert (first[2] <= (len(cx) - k) - n_empty).all() and (fast[2] <= (len(cx) - k) - n_empty).all()
    if not judge:
        return
    po = ParityOracle(t, cx, cy, k, length, N, widths, ist)
    assert (po.ns0 <= (len(cx) - k) - n_empty).all()
    batch_parity(first[1], po, f"branch arithmetic {case} B={B}")
    batch_parity(fast[1], po, f"fast arithmetic {case} B={B}")


@pytest.mark.parametrize("case,B", [(("c100", 58), 64), (("c0p8", 48), 16), (("c0p8", 179), 16), (("c30", 179), 16)],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else f"B{v}")
def test_branch_and_fast_arithmetic_sparse(rl, fits, rings, monkeypatch, case, B):
    """The branch and fast arithmetics on sparse samplings, by the nearest-branch rule; the branch arithmetic also bit-identical
    across the two residencies (global scratch at a batch of 64 included) and the three search modes."""
    _branch_and_fast(rl, fits, rings, monkeypatch, case, B, judge=True)


def test_branch_arithmetic_sparse_chaotic_bits(rl, fits, rings, monkeypatch):
    """c0p8 at N = 97 (four empty supports) is chaotic: the oracle's own FMA build moves some of these lines by metres, so the
    nearest-branch rule cannot decide them.  What is decidable is checked: the branch arithmetic's bits across residencies and
    search modes, and that no empty support is counted as a success, in either arithmetic."""
    _branch_and_fast(rl, fits, rings, monkeypatch, ("c0p8", 97), 16, judge=False)


def test_degree3_fast_arithmetic_with_an_empty_support(rl, fits):
    """l10 (degree 3, fast arithmetic only) at N = 120: control point 6 has an empty support."""
    from parity_rule import ParityOracle, batch_parity
    t, cx, cy, k, length = spline(fits, "l10")
    N, B = 120, 8
    n = len(cx)
    n_empty = len(empty_points(t, k, n, N))
    assert k == 3 and n_empty > 0
    ist = i_start(n, k, N)
    widths = rl.batch.width_batch(np.full(N, 4.0), np.full(N, 3.0), B, seed=5)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    ctrl, xy, ns, status, st = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, arith=rl.lib.ARITH_FAST)
    assert st.reserved[0] == rl.lib.ARITH_FAST
    np.testing.assert_array_equal(status, 2 * len(ist) * (n - k) - ns.reshape(B, -1).sum(axis=1))
    assert (ns <= (n - k) - n_empty).all() and ns.sum() > 0
    po = ParityOracle(t, cx, cy, k, length, N, widths, ist)
    assert (po.ns0 <= (n - k) - n_empty).all()
    batch_parity(xy, po, f"k=3 N={N}")
