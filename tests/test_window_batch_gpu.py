"""The batched sliding-window driver (rl_mincurv_solve_batch_joint_*): per-instance bounds, start lines and start indices
in one launch, against the oracle run per instance (reference-order arithmetic), against rl_mincurv_sweep_joint (both
arithmetics) and against itself (position independence, continuation).  Every comparison is bit for bit; the cases and
their premises are those of tests/window_batch_cases.py, certified on the CPU by tests/test_window_batch_cpu.py."""
import ctypes

import numpy as np
import pytest

import window_batch_cases as wc
from conftest import spline

pytestmark = pytest.mark.gpu
FAST, REF, BRANCH = 0, 1, 2
ERR_ARG, ERR_UNSUPPORTED = "error -1", "error -4"


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    ctx = _lib.Context.get(0)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch, ns.ctx = _lib, ops, batch, ctx
    assert (_lib.ARITH_FAST, _lib.ARITH_REFERENCE, _lib.ARITH_BRANCH) == (FAST, REF, BRANCH)
    return ns


def make_track(rl, case):
    trk = rl.lib.Track(rl.ctx, case["t"], case["cx"], case["cy"], case["k"], case["N"])
    if case["form"] == "shared":
        rL, rR = case["pairs"][0]
        trk.set_rings(rL, rR)
    return trk


def bform(rl, case):
    return {"shared": rl.lib.BOUNDS_SHARED_RINGS, "widths": rl.lib.BOUNDS_WIDTHS, "points": rl.lib.BOUNDS_POINTS}[case["form"]]


def solve(rl, trk, case, rows=None, ctrl0="case", arith=REF, B=None):
    rows = case["rows"] if rows is None else rows
    ctrl0 = case["ctrl0"] if isinstance(ctrl0, str) else ctrl0
    return rl.ops.solve_batch_host(trk, bform(rl, case), case["bounds"], rows, arith=arith, ctrl0=ctrl0, driver="window",
                                   B=len(case["pairs"]) if B is None else B)


def assert_oracle_bits(case, got, oracle, residency=None):
    ctrl, xy, ns, status, st = got
    octrl, oxy, ons, oraised = oracle
    if residency is not None:
        assert st.rings_in_lds == int(residency)
    assert st.reserved[0] == REF
    assert ns.shape == ons.shape
    np.testing.assert_array_equal(ns, ons)
    np.testing.assert_array_equal(ctrl, octrl)
    np.testing.assert_array_equal(xy, oxy)
    total = wc.windows_per_iteration(len(case["cx"]), case["k"]) * ons.shape[1]
    np.testing.assert_array_equal(status, total - ons.sum(axis=1))
    return total


# ---- 1. the oracle's bits
@pytest.mark.parametrize("residency", ["0", "1"])
@pytest.mark.parametrize("N,form", wc.MONZA_CASES)
def test_oracle_bits(rl, fits, rings, monkeypatch, N, form, residency):
    """B = 6 from per-instance start lines (the track's line, moved copies, one instance equal to another's) with per-instance
    rows that hold the smallest and the largest valid start index, two outer iterations, in the three bounds forms: control
    points, samples, counts and status are the oracle's, instance by instance, with the state in global scratch and in LDS."""
    case = wc.monza_case(fits, rings, N, form)
    trk = make_track(rl, case)
    monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
    got = solve(rl, trk, case)
    oracle = wc.oracle_window(case)
    assert_oracle_bits(case, got, oracle, residency)
    B = len(case["ctrl0"])
    np.testing.assert_array_equal(got[0][B - 1], got[0][2])
    assert oracle[2].sum() > 0


# ---- 2. the kart circuit
@pytest.mark.parametrize("residency", ["0", "1"])
def test_kart_circuit(rl, monkeypatch, residency):
    """Four width variants of the kart circuit, one outer iteration of 58 windows: many windows have no feasible QP; the
    oracle's bits, and status = 58 - the updated count per instance."""
    case = wc.kart_case()
    trk = make_track(rl, case)
    monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
    got = solve(rl, trk, case)
    oracle = wc.oracle_window(case)
    total = assert_oracle_bits(case, got, oracle, residency)
    assert total == 58
    np.testing.assert_array_equal(got[3], 58 - got[2][:, 0])
    print("kart circuit: windows updated per instance", got[2][:, 0].tolist(), "of 58")
    assert (got[3] > 0).all() and (got[2] > 0).all()


# ---- 3. the single call, position independence
@pytest.mark.parametrize("arith", [FAST, REF])
def test_equals_the_single_call_and_is_position_independent(rl, fits, rings, arith):
    """B = 1 from the track's line with a shared index list equals rl_mincurv_sweep_joint in cx, cy and the counts; five
    identical instances give five times row 0; permuting a batch of different instances permutes the output.  Both
    residencies."""
    t, cx, cy, k, length = spline(fits, "c100")
    N, n = 200, len(cx)
    i_start = rl.batch.default_i_start(n, k, 2, seed=5, driver="window")
    trk, trk2 = (rl.lib.Track(rl.ctx, t, cx, cy, k, N) for _ in range(2))
    for q in (trk, trk2):
        q.set_rings(rings[0], rings[1])
    S = rl.lib.BOUNDS_SHARED_RINGS
    case = wc.monza_case(fits, rings, N, "widths")
    wtrk = make_track(rl, case)
    perm = np.array([3, 0, 5, 1, 4, 2])
    for residency in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("RL_FORCE_RESIDENCY", residency)
            scx, scy, _, sns, sst = rl.ops.mincurv_sweep_joint(trk2, cx, cy, i_start, arith=arith)
            one = rl.ops.solve_batch_host(trk, S, None, i_start, arith=arith, driver="window", B=1)
            assert one[4].reserved[0] == arith == sst.reserved[0] and one[4].rings_in_lds == int(residency)
            np.testing.assert_array_equal(one[0][0, :, 0], scx); np.testing.assert_array_equal(one[0][0, :, 1], scy)
            np.testing.assert_array_equal(one[2][0], sns)
            assert one[2].shape == (1, 2) and sns.sum() > 0 and one[3][0] == 2 * 56 - sns.sum()
            five = rl.ops.solve_batch_host(trk, S, None, i_start, arith=arith, driver="window", B=5)
            for q in range(4):
                np.testing.assert_array_equal(five[q], np.broadcast_to(one[q], five[q].shape))
            a = solve(rl, wtrk, case, arith=arith)
            pcase = dict(case, bounds=case["bounds"][perm], ctrl0=case["ctrl0"][perm], rows=case["rows"][perm])
            p = solve(rl, wtrk, pcase, arith=arith)
            for q in range(4):
                np.testing.assert_array_equal(p[q], a[q][perm])
            assert not np.array_equal(a[0][1], a[0][0])


# ---- 4. continuation
@pytest.mark.parametrize("residency", ["0", "1"])
@pytest.mark.parametrize("arith", [REF, FAST])
def test_continuation_bitwise(rl, fits, rings, monkeypatch, arith, residency):
    """3 outer iterations against 2, then 1 more from the first run's control points with the remaining start index (under
    numpy's raise mode, which only the reference-order arithmetic models): the same control points, samples and counts.  The
    case meets the contract's conditions (tests/test_window_batch_cpu.py); in the reference-order arithmetic the whole run is
    the oracle's."""
    case = wc.continuation_case(fits, rings)
    a = case["split"]
    trk = make_track(rl, case)
    i_start = case["rows"][0]
    monkeypatch.setenv("RL_FORCE_RESIDENCY", residency)
    full = solve(rl, trk, case, rows=i_start, ctrl0=None, arith=arith)
    first = solve(rl, trk, case, rows=i_start[:a], ctrl0=None, arith=arith)
    rl.ctx.set_numpy_raise(True)
    try:
        second = solve(rl, trk, case, rows=i_start[a:], ctrl0=first[0], arith=arith)
    finally:
        rl.ctx.set_numpy_raise(False)
    assert second[4].rings_in_lds == int(residency) and second[4].reserved[0] == arith
    np.testing.assert_array_equal(second[0], full[0])
    np.testing.assert_array_equal(second[1], full[1])
    np.testing.assert_array_equal(second[2], full[2][:, a:])
    np.testing.assert_array_equal(first[2], full[2][:, :a])
    np.testing.assert_array_equal(first[3] + second[3], full[3])
    assert not np.array_equal(first[0], full[0]) and first[2].sum() > 0
    if arith == REF:
        oracle = wc.oracle_window(case)
        assert (oracle[3] == 0).all()
        assert_oracle_bits(case, full, oracle)


# ---- 5. numpy's raise mode
def test_under_numpy_raise(rl):
    """Fixture G12 at N = 240 with rl_ctx_set_numpy_raise(1): windows raise on the instances that start from G12's own line
    (the control points written, the table stale, the window not counted) -- the oracle's bits, and its raised count through
    status = windows - updated, of which the oracle tells how many raised.  Without raise mode at the start the run differs and is
    again the oracle's."""
    for numpy_raise in (True, False):
        case = wc.raise_case(numpy_raise)
        trk = make_track(rl, case)
        rl.ctx.set_numpy_raise(numpy_raise)
        try:
            got = solve(rl, trk, case)
            shared = solve(rl, trk, case, rows=case["rows"][0])
        finally:
            rl.ctx.set_numpy_raise(False)
        oracle = wc.oracle_window(case)
        total = assert_oracle_bits(case, got, oracle)
        for q in range(4):
            np.testing.assert_array_equal(shared[q], got[q])
        print(f"G12 raise={numpy_raise}: updated {got[2].sum(axis=1).tolist()} raised (oracle) {oracle[3].tolist()} of {total}")
        if numpy_raise:
            assert oracle[3][0] > 0 and oracle[3][2] == oracle[3][0]
            assert (got[3] >= oracle[3]).all()          # status counts the raised windows and the infeasible ones
            with_raise = got
    assert not np.array_equal(with_raise[0][0], got[0][0])


# ---- 6. device-side validation
def test_device_start_indices_are_validated(rl, fits, rings):
    """Rows that never were on the host: k//2 - 1, n-(k-k//2)-5 and n-(k-k//2)-1 (valid for the sweep, not for the window)
    give status -1, the start line and its samples back (bit for bit) and zero counts; the neighbours are bit-identical to a batch without
    the bad rows.  The host entry refuses the same rows with RL_ERR_ARG."""
    import torch
    case = wc.monza_case(fits, rings, 200, "widths")
    k, N = case["k"], case["N"]
    n = len(case["cx"])
    lo, hi = wc.window_range(n, k)
    rows, ctrl0, widths = case["rows"], case["ctrl0"], case["bounds"]
    bad = rows.copy(); bad[1, 1] = lo - 1; bad[2, 0] = hi; bad[4, 1] = n - (k - k // 2) - 1
    trk = make_track(rl, case)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    W = rl.lib.BOUNDS_WIDTHS
    # "the start line's samples", bit for bit: what the same library returns in the same arithmetic for an instance that starts
    # from the same line with VALID rows and updates nothing -- half-widths of 1 cm put samples of the moved lines outside
    # their boxes all round the track, so every window is refused (tests/test_window_batch_cpu.py fixes that on the oracle);
    # in the reference-order arithmetic also the oracle's own sampling of that line
    still = wc.refused_case(fits, rings)
    np.testing.assert_array_equal(still["ctrl0"], ctrl0)
    ostill = wc.oracle_window(still)
    for arith in (REF, FAST):
        kept = solve(rl, trk, still, arith=arith)
        for b in (1, 2, 4):
            assert (kept[2][b] == 0).all() and kept[3][b] == 2 * (hi - lo)
            np.testing.assert_array_equal(kept[0][b], ctrl0[b])
        if arith == REF:
            np.testing.assert_array_equal(kept[1], ostill[1])
            for b in (1, 2, 4):
                np.testing.assert_array_equal(kept[1][b], wc.oracle_samples(still, ctrl0[b]))
        good = rl.ops.solve_batch_torch(trk, W, up(widths), up(rows), arith=arith, ctrl0=up(ctrl0), driver="window")
        got = rl.ops.solve_batch_torch(trk, W, up(widths), up(bad), arith=arith, ctrl0=up(ctrl0), driver="window")
        torch.cuda.synchronize()
        g_ = {q: v.cpu().numpy() for q, v in good.items() if q != "stats"}
        r_ = {q: v.cpu().numpy() for q, v in got.items() if q != "stats"}
        assert g_["n_success"].shape == (6, 2) and (g_["status"] >= 0).all() and (g_["n_success"].sum(axis=1) > 0).all()
        for b in (1, 2, 4):
            assert r_["status"][b] == -1 and (r_["n_success"][b] == 0).all()
            np.testing.assert_array_equal(r_["ctrl"][b], ctrl0[b])
            np.testing.assert_array_equal(r_["xy"][b], kept[1][b])
        for b in (0, 3, 5):
            for q in ("ctrl", "xy", "n_success", "status"):
                np.testing.assert_array_equal(r_[q][b], g_[q][b])
        host = solve(rl, trk, case, arith=arith)
        np.testing.assert_array_equal(host[0], g_["ctrl"]); np.testing.assert_array_equal(host[2], g_["n_success"])
    # the host entry itself (ops checks host rows first, with a ValueError)
    with pytest.raises(ValueError, match="i_start"):
        solve(rl, trk, case, rows=bad)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    B = len(rows)
    ctrl = np.zeros((B, n, 2)); xy = np.zeros((B, N, 2)); ns = np.zeros((B, 2), dtype=np.int32); status = np.zeros(B, dtype=np.int32)
    for col, val in ((1, lo - 1), (0, hi), (1, n - (k - k // 2) - 1)):
        one_bad = np.ascontiguousarray(rows.copy()); one_bad[3, col] = val
        rc = rl.ctx.lib.rl_mincurv_solve_batch_joint_host(
            rl.ctx.h, trk.h, W, widths.ctypes.data_as(dp), B, ctrl0.ctypes.data_as(dp), one_bad.ctypes.data_as(ip), 1, 2,
            rl.lib.SEARCH_WINDOWED, ctrl.ctypes.data_as(dp), xy.ctypes.data_as(dp), ns.ctypes.data_as(ip), status.ctypes.data_as(ip), None)
        assert rc == -1 and b"i_start outside" in rl.ctx.lib.rl_last_error()
        shared_bad = np.array([rows[0, 0], val], dtype=np.int32)
        rc = rl.ctx.lib.rl_mincurv_solve_batch_joint_host(
            rl.ctx.h, trk.h, W, widths.ctypes.data_as(dp), B, None, shared_bad.ctypes.data_as(ip), 0, 2,
            rl.lib.SEARCH_WINDOWED, ctrl.ctypes.data_as(dp), xy.ctypes.data_as(dp), ns.ctypes.data_as(ip), status.ctypes.data_as(ip), None)
        assert rc == -1 and b"i_start outside" in rl.ctx.lib.rl_last_error()


# ---- 7. refusals
def test_refusals(rl, fits, rings):
    """RL_ARITH_BRANCH, a degree-3 track and a window wider than 768 samples: RL_ERR_UNSUPPORTED, each with a message that
    names the limit.  rl_mincurv_solve_batch_from_* is what it was: the sweep driver, n_success [B,max_iter,2], the sweep's
    index range."""
    t, cx, cy, k, length = spline(fits, "c100")
    n = len(cx)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, 200)
    trk.set_rings(rings[0], rings[1])
    S = rl.lib.BOUNDS_SHARED_RINGS
    with pytest.raises(rl.lib.RlError, match=ERR_UNSUPPORTED + ".*branch arithmetic"):
        rl.ops.solve_batch_host(trk, S, None, [10], arith=BRANCH, driver="window", B=2)
    t3, cx3, cy3, k3, _ = spline(fits, "l10")
    trk3 = rl.lib.Track(rl.ctx, t3, cx3, cy3, k3, 200)
    for arith in (None, FAST, REF):
        with pytest.raises(rl.lib.RlError, match=ERR_UNSUPPORTED + ".*degree"):
            rl.ops.solve_batch_host(trk3, rl.lib.BOUNDS_WIDTHS, np.full((2, 200, 2), 5.0), [3], arith=arith, driver="window")
    dense = rl.lib.Track(rl.ctx, t, cx, cy, k, 8000)
    dense.set_rings(rings[0], rings[1])
    for arith in (FAST, REF):
        with pytest.raises(rl.lib.RlError, match=ERR_UNSUPPORTED + ".*768 samples"):
            rl.ops.solve_batch_host(dense, S, None, [10], arith=arith, driver="window", B=2)
    with pytest.raises(ValueError, match="driver"):
        rl.ops.solve_batch_host(trk, S, None, [10], driver="joint", B=2)
    # the sweep's own per-instance entry: the index n-(k-k//2)-1 is valid there, the output has the sweep's layout
    c0 = np.broadcast_to(np.column_stack([cx, cy]), (2, n, 2))
    last = n - (k - k // 2) - 1
    rows = np.array([[last], [7]], dtype=np.int32)
    new = rl.ops.solve_batch_host(trk, S, None, rows, arith=FAST, ctrl0=c0)
    assert new[2].shape == (2, 1, 2) and (new[3] >= 0).all() and new[2].sum() > 0
    for b in range(2):
        scx, scy, _, sns, _ = rl.ops.mincurv_sweep(trk, cx, cy, rows[b], arith=FAST)
        np.testing.assert_array_equal(new[0][b, :, 0], scx); np.testing.assert_array_equal(new[2][b], sns)
    with pytest.raises(rl.lib.RlError, match=ERR_ARG):
        rl.ops.solve_batch_host(trk, S, None, np.array([[last + 1], [7]], dtype=np.int32), arith=FAST, ctrl0=c0)


# ---- 8. the chain
def test_polish_chain(rl, fits, rings):
    """spline_fit_torch -> solve_batch_torch(driver="window", ctrl0 = the fit) -> tables_torch enqueued on one stream with no
    host synchronisation in between, against the same steps through host calls."""
    import torch
    case = wc.continuation_case(fits, rings, B=4)
    t, cx, cy, k, length, N = case["t"], case["cx"], case["cy"], case["k"], case["length"], case["N"]
    n, B = len(cx), 4
    widths = case["bounds"]
    trk = make_track(rl, case)
    W = rl.lib.BOUNDS_WIDTHS
    rows = rl.batch.default_i_start_batch(n, k, 1, B, seed=30, driver="window")
    first = solve(rl, trk, case, rows=case["rows"][0][:1], ctrl0=None)        # lines that are not the track's: one iteration solved
    dev = torch.device("cuda", 0)
    dw, dxy = torch.from_numpy(widths).to(dev), torch.from_numpy(first[1]).to(dev)
    u = np.arange(N) / N
    du = torch.from_numpy(u).to(dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        out = rl.batch.polish_lines_torch(trk, dxy, W, dw, rows, u=du, driver="window")
        pts = rl.ops.tables_torch(trk, out["ctrl"], W, dw, length)
    stream.synchronize()
    fit_stats = out["fit_stats"].cpu().numpy()
    assert (fit_stats[:, 0] == 0).all() and (fit_stats[:, 1] < 1e-6).all()
    f_ctrl, f_stats = rl.ops.spline_fit_host(trk, first[1], u)
    np.testing.assert_array_equal(out["fit_ctrl"].cpu().numpy(), f_ctrl); np.testing.assert_array_equal(fit_stats, f_stats)
    p = solve(rl, trk, case, rows=rows, ctrl0=f_ctrl)
    assert tuple(out["n_success"].shape) == (B, 1)
    np.testing.assert_array_equal(out["ctrl"].cpu().numpy(), p[0]); np.testing.assert_array_equal(out["xy"].cpu().numpy(), p[1])
    np.testing.assert_array_equal(out["n_success"].cpu().numpy(), p[2]); np.testing.assert_array_equal(out["status"].cpu().numpy(), p[3])
    assert p[2].sum() > 0
    h_pts = rl.ops.tables_host(trk, p[0], W, widths, length)
    np.testing.assert_array_equal(pts.cpu().numpy(), h_pts)


# ---- 9. the step dump
def test_step_dump_stays_silent(rl, fits, rings):
    """rl_debug_dump_enable(1) changes nothing a batch call returns, in the default arithmetic (which stays the
    reference-order one) and in the fast one."""
    case = wc.monza_case(fits, rings, 200, "shared")
    trk = make_track(rl, case)
    for arith in (None, FAST):
        plain = solve(rl, trk, case, arith=arith)
        rl.lib.check(rl.lib.load().rl_debug_dump_enable(1))
        try:
            dumped = solve(rl, trk, case, arith=arith)
        finally:
            rl.lib.check(rl.lib.load().rl_debug_dump_enable(0))
        assert dumped[4].reserved[0] == plain[4].reserved[0] == (REF if arith is None else FAST)
        for q in range(4):
            np.testing.assert_array_equal(dumped[q], plain[q])
    assert plain[2].sum() > 0
