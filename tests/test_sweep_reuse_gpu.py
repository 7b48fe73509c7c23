"""The sweep's rows read the table's X, Y where the refresh stored them (csrc/rl_sweep.hpp: pXY, next to the bound points, in
LDS or in the instance's global scratch) instead of summing them again, and the prologue's separation pass is pruned
(csrc/rl_sep.hpp).  Neither may move a bit: the reference-order arithmetic against the CR oracle -- control points, sampled
line, success counts, status -- and the branch arithmetic, which the oracle does not have, against what it is documented to
be: one result whatever the search mode and the residency (tests/test_reference_order.py::test_branch_arithmetic_small_batches).
Every case runs in the three search modes and with the per-instance state in LDS and in global scratch.

The cases are the ones in which a row reads a position stored long before: empty supports and failed steps (no refresh
follows: the next rows read what an earlier step stored), alias steps at both ends of the spline (two ranges re-sampled),
per-instance start lines (the first fill stores each instance's own line) and numpy's raise mode (the plain kernel hands the
instance to the raise instantiation, which starts again from the prologue and reads its snapshot while the table is stale)."""
import concurrent.futures

import numpy as np
import pytest

from conftest import golden, spline
from oracle import oracle as orc
from sparse_cases import empty_points, i_start as sparse_i_start

pytestmark = pytest.mark.gpu
REF, BRANCH = 1, 2   # _lib.ARITH_REFERENCE, _lib.ARITH_BRANCH
VARIANTS = [(residency, search) for residency in ("1", "0") for search in (0, 1, 2)]


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    _lib.Context.get(0)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch = _lib, ops, batch
    assert _lib.ARITH_REFERENCE == REF and _lib.ARITH_BRANCH == BRANCH
    return ns


def _half_widths(rl, fits, rings, tag, N):
    t, cx, cy, k, length = spline(fits, tag)
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    orc.fill_bounds(pts, rings[0], rings[1], 100.0)
    return rl.batch.half_widths_from_bounds(pts)


def _every_variant(monkeypatch, run, want, label):
    """run(search, arith) -> (ctrl, xy, ns, status, stats) in every residency and search mode.  Reference-order: `want`
    = (ctrl, xy, ns, status or None), bit for bit.  Branch: every variant equals the first one."""
    first = None
    for residency, search in VARIANTS:
        monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
        what = f"{label} residency {residency} search {search}"
        ctrl, xy, ns, status, st = run(search, REF)
        assert st.rings_in_lds == int(residency) and st.reserved[0] == REF, what
        np.testing.assert_array_equal(ns, want[2], err_msg=what)
        np.testing.assert_array_equal(ctrl, want[0], err_msg=what)
        np.testing.assert_array_equal(xy, want[1], err_msg=what)
        if want[3] is not None:
            np.testing.assert_array_equal(status, want[3], err_msg=what)
        ctrl, xy, ns, status, st = run(search, BRANCH)
        assert st.rings_in_lds == int(residency) and st.reserved[0] == BRANCH, what
        if first is None:
            first = (ctrl, xy, ns, status)
            assert ns.sum() > 0 and np.isfinite(ctrl).all()
        for got, exp in zip((ctrl, xy, ns, status), first):
            np.testing.assert_array_equal(got, exp, err_msg="branch arithmetic, " + what)


@pytest.mark.parametrize("tag,N", [("c0p8", 48), ("c100", 46)])
def test_sparse_width_batches(rl, fits, rings, monkeypatch, tag, N):
    """Empty supports: a step on one runs no refresh, and the rows of the steps behind it read positions that were stored
    several steps earlier.  Width rings of N <= 48 vertices: the windowed search falls back, every search mode stores."""
    t, cx, cy, k, length = spline(fits, tag)
    assert len(empty_points(t, k, len(cx), N)) > 0
    ist = sparse_i_start(len(cx), k, N)
    B = 4
    wl, wr = _half_widths(rl, fits, rings, tag, N)
    widths = rl.batch.width_batch(wl, wr, B, seed=N)
    with orc.cr_variant():
        octrl, oxy, ons = orc.solve_width_batch(t, cx, cy, k, length, N, widths, ist, nthreads=4)
    steps = 2 * len(ist) * (len(cx) - k)
    ostatus = steps - ons.reshape(B, -1).sum(axis=1)
    assert (ostatus > 0).all()
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    _every_variant(monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, search=search,
                                                                              arith=arith),
                   (octrl, oxy, ons, ostatus), f"{tag} N={N}")


def test_monza_alias_steps_on_the_shared_rings(rl, fits, rings, monkeypatch):
    """Monza c100, N = 200, three outer iterations in fixture G7's sweep order: every pass walks over both ends of the spline,
    where a step re-samples the support of the control point AND of its periodic alias."""
    t, cx, cy, k, length = spline(fits, "c100")
    N, B = 200, 2
    ist = golden("G7_run_min_curvature_qp.npz")["c100_N200_it3_seed1_i_start"]
    with orc.cr_variant():
        ocx, ocy, opts, ons = orc.run_min_curvature_qp(t, cx, cy, k, length, N, rings[0], rings[1], ist)
    want = (np.stack([np.column_stack([ocx, ocy])] * B), np.stack([opts[:, :2]] * B), np.stack([ons] * B),
            np.full(B, 2 * len(ist) * (len(cx) - k) - ons.sum()))
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    trk.set_rings(rings[0], rings[1])
    _every_variant(monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_SHARED_RINGS, None, ist, search=search,
                                                                              B=B, arith=arith),
                   want, "monza N=200")


def test_corridors_so_narrow_that_steps_fail(rl, fits, rings, monkeypatch):
    """A fifth of Monza's half-widths, floored at 0.3 m: the line leaves the corridor of a neighbouring sample, whose row then
    has no feasible clamp interval (s4 > s5) -- about one step in twelve fails in the oracle's run, no refresh follows it, and
    the success counts must be the oracle's."""
    t, cx, cy, k, length = spline(fits, "c100")
    N, B = 200, 4
    ist = golden("G7_run_min_curvature_qp.npz")["c100_N200_it3_seed1_i_start"]
    wl, wr = _half_widths(rl, fits, rings, "c100", N)
    widths = rl.batch.width_batch(0.2 * wl, 0.2 * wr, B, seed=7, floor=0.3)
    with orc.cr_variant():
        octrl, oxy, ons = orc.solve_width_batch(t, cx, cy, k, length, N, widths, ist, nthreads=4)
    steps = 2 * len(ist) * (len(cx) - k)
    ostatus = steps - ons.reshape(B, -1).sum(axis=1)
    print("steps", steps, "failed in the oracle's run, per instance:", ostatus.tolist())
    assert (ostatus > 10).all()
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    _every_variant(monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, search=search,
                                                                              arith=arith),
                   (octrl, oxy, ons, ostatus), "narrow corridors")


def test_start_lines_one_from_the_track_one_shifted(rl, fits, rings, monkeypatch):
    """rl_mincurv_solve_batch_from_*: instance 0 starts from the track's own control points, instance 1 from a line shifted by
    up to 0.3 m, each in its own sweep order; the width rings are built about the TRACK's line for both.  The table's X, Y of
    instance 1 come from its own line from the first fill on."""
    t, cx, cy, k, length = spline(fits, "c100")
    N, B, max_iter = 200, 2, 2
    m = len(cx) - k
    d = 0.3 * np.sin(2.0 * np.pi * np.arange(m) / m)
    x1, y1 = cx[:m] + d, cy[:m] - d
    ctrl0 = np.stack([np.column_stack([cx, cy]),
                      np.column_stack([np.concatenate([x1, x1[:k]]), np.concatenate([y1, y1[:k]])])])
    rows = rl.batch.default_i_start_batch(len(cx), k, max_iter, B, seed=0)
    wl, wr = _half_widths(rl, fits, rings, "c100", N)
    widths = rl.batch.width_batch(wl, wr, B, seed=1234)

    def one(b):
        rL, rR = orc.width_rings(t, cx, cy, k, N, widths[b])
        ocx, ocy, opts, ons = orc.run_min_curvature_qp(t, ctrl0[b, :, 0], ctrl0[b, :, 1], k, length, N, rL, rR, rows[b])
        return np.column_stack([ocx, ocy]), opts[:, :2].copy(), ons

    with orc.cr_variant():
        orc.lib()
        with concurrent.futures.ThreadPoolExecutor(max_workers=B) as ex:
            res = list(ex.map(one, range(B)))
    want = tuple(np.stack([r[i] for r in res]) for i in range(3))
    ostatus = 2 * max_iter * m - want[2].reshape(B, -1).sum(axis=1)
    assert not np.array_equal(want[0][0], want[0][1])
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    _every_variant(monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, rows, search=search,
                                                                              arith=arith, ctrl0=ctrl0),
                   want + (ostatus,), "start lines")


def test_numpy_raise_at_start_g12(rl, monkeypatch):
    """Fixture G12's track (a stretch of exactly zero curvature) with numpy's raise mode on from the start: the plain
    reference-order kernel flags the instance, the raise instantiation redoes it from the prologue -- its rows read the stored
    X, Y while the table is current and the snapshot while it is stale -- and agrees with the oracle."""
    g = golden("G12_numpy_raise_semantics.npz")
    t, cx, cy, k, length = g["t"], g["cx"], g["cy"], int(g["k"]), float(g["length"])
    N, B = 300, 2
    ist = g["sweep_N300_i_start"]
    with orc.cr_variant():
        ocx, ocy, opts, ons = orc.run_min_curvature_qp(t, cx, cy, k, length, N, g["ringL"], g["ringR"], ist, numpy_raise=True)
        assert orc.last_raised() > 0
    ctx = rl.lib.Context.get(0)
    trk = rl.lib.Track(ctx, t, cx, cy, k, N)
    trk.set_rings(g["ringL"], g["ringR"])
    ctx.set_numpy_raise(True)
    try:
        for residency, search in VARIANTS:
            monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
            what = f"G12 residency {residency} search {search}"
            ctrl, xy, ns, status, st = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_SHARED_RINGS, None, ist, search=search, B=B, arith=REF)
            assert st.rings_in_lds == int(residency) and st.reserved[0] == REF, what
            for b in range(B):
                np.testing.assert_array_equal(ns[b], ons, err_msg=what)
                np.testing.assert_array_equal(ctrl[b, :, 0], ocx, err_msg=what)
                np.testing.assert_array_equal(ctrl[b, :, 1], ocy, err_msg=what)
    finally:
        ctx.set_numpy_raise(False)
