"""rl_frenet_batch_* / rl_frenet_resample_* / batch.min_time_guess_from_lines_torch / optimise_track_batch(start_points=...) on
the device against the CPU twin (tests/frenet_twin.py) and against RaceTrack.frenet_to_global.

Tolerance (frenet_twin.TOL) against the twin and for round trips: 1e-9 m for s (cyclic difference) and n, 1e-9 rad for xi, 1e-9
for g.  The error of a Newton root is eps (|coordinates| + L) / g, about 1e-12 under g >= 0.1, and the twin measured 6e-14 m on
these inputs; 1e-9 leaves three orders and is five below the 1e-4 m the project's parity figure is stated in.  Every test
asserts on its own inputs that the projection is well conditioned there: the twin's best local minimum ahead of the second best
by >= 1e-6 m and g >= 0.1.  Every case has B <= 5, P <= 257, M about 100.

Measured on the MI355X (first run): against the twin and on the round trips s <= 1.14e-13 m, n <= 3.2e-14 m, xi <= 1.04e-14 rad,
g <= 4.2e-15 over every case (gaps >= 19 m, g >= 0.57); the resample against the twin 8.7e-19; X0 / T0 of the chain 2e-14 /
1.7e-15; interior-point iterations of the chain 73 / 78 / 76 from the centre line, 41 / 63 / 78 from the lines."""
import ctypes

import numpy as np
import pytest

import frenet_twin as ft
import pose_tables_twin as ptw
from mintime_problem import width_scales

pytestmark = pytest.mark.gpu
TOL = ft.TOL


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    ctx = _lib.Context.get(0)
    ctx.set_arith(_lib.ARITH_DEFAULT)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch, ns.ctx = _lib, ops, batch, ctx
    yield ns
    ctx.set_option("frenet_search", 1)


@pytest.fixture(scope="module")
def rt():
    return ptw.mgkt_race_track(8.0)


def compare(tag, fr, ref, L):
    """fr [.., 4] of the device against ref; prints each figure before it asserts."""
    ds = float(ft.cyclic(fr[..., 0], ref[..., 0], L).max())
    dn, dxi, dg = (float(np.abs(fr[..., c] - ref[..., c]).max()) for c in (1, 2, 3))
    print(f"[frenet {tag}] s {ds:.2e} m  n {dn:.2e} m  xi {dxi:.2e} rad  g {dg:.2e}")
    assert ds <= TOL and dn <= TOL and dxi <= TOL and dg <= TOL
    assert (fr[..., 0] >= 0).all() and (fr[..., 0] < L).all()


def check_stats(fr, status, stats):
    assert (status == 0).all() and (stats[:, 0] == 0).all()
    np.testing.assert_array_equal(stats[:, 1], fr[..., 3].min(axis=1))
    np.testing.assert_array_equal(stats[:, 2], np.abs(fr[..., 1]).max(axis=1))
    assert (stats[:, 3] >= 0).all() and (stats[:, 3] <= 49).all()          # kFrenetIters + 1 evaluations at most


@pytest.fixture(scope="module")
def round_trip(rl, rt):
    """Cases 1 and 2 share it: synthetic (s, n, xi) -> k_pose_tables (POSE_FRENET) -> k_frenet, the twin on the same tables."""
    t, cx, cy, k, _ = ptw.mgkt_fits()["c"]
    rings = (rt.left_r.vertices, rt.right_r.vertices)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, len(rings[0]))
    trk.set_rings(*rings)
    pieces = rt.centerline_pieces()
    out = {}
    for amp in (0.3, 4.0):
        X = np.ascontiguousarray(ptw.synthetic_frenet(rt, len(rt.abscissa), 3, shift=0.37, amp_n=amp))
        pts = rl.ops.pose_tables_host(trk, rl.lib.POSE_FRENET, X, pieces, rl.lib.BOUNDS_SHARED_RINGS, None)
        fr, status, stats = rl.ops.frenet_host(pieces, pts)
        ref, gap = ft.project_batch(pieces, pts)
        ft.assert_well_conditioned(f"round trip amp_n={amp}", ref, gap)
        out[amp] = dict(X=X, pts=pts, fr=fr, status=status, stats=stats, ref=ref)
    return out


@pytest.mark.parametrize("amp", [0.3, 4.0])
def test_round_trip_through_pose_tables(rl, rt, round_trip, amp):
    c = round_trip[amp]
    L = rt.center_s.get_length()
    X = c["X"]
    assert (X[-1, :, 0] < 0).sum() > 5 and (X[-1, :, 0] > L).sum() > 5     # the shifted instance
    want = np.stack([np.mod(X[..., 0], L), X[..., 1], X[..., 2], c["ref"][..., 3]], axis=-1)
    compare(f"round trip amp_n={amp}", c["fr"], want, L)
    check_stats(c["fr"], c["status"], c["stats"])


@pytest.mark.parametrize("amp", [0.3, 4.0])
def test_against_the_twin(rl, rt, round_trip, amp):
    c = round_trip[amp]
    compare(f"twin amp_n={amp}", c["fr"], c["ref"], rt.center_s.get_length())


@pytest.mark.parametrize("B,P", [(1, 1), (5, 1), (1, 63), (5, 63), (1, 257), (5, 257)])
def test_shapes_against_the_twin(rl, rt, B, P):
    pieces = rt.centerline_pieces()
    pts = np.ascontiguousarray(ft.line_tables(rt, ptw.synthetic_frenet(rt, P, B, shift=0.37, amp_n=2.0, seed=P)))
    ref, gap = ft.project_batch(pieces, pts)
    ft.assert_well_conditioned(f"B={B} P={P}", ref, gap)
    fr, status, stats = rl.ops.frenet_host(pieces, pts)
    compare(f"B={B} P={P}", fr, ref, rt.center_s.get_length())
    check_stats(fr, status, stats)


@pytest.mark.parametrize("n", [1.0, -1.0])
def test_feet_on_breakpoints(rl, rt, n):
    pieces = rt.centerline_pieces()
    ss = pieces[0]
    L = ss[-1]
    s = np.r_[ss[:-1], np.nextafter(L, 0.0)]                              # every breakpoint, s = 0 and the largest double below L
    pts = np.ascontiguousarray(ft.line_tables(rt, np.stack([s, np.full(len(s), n), np.zeros(len(s))] + [np.zeros(len(s))] * 3, 1)[None]))
    ref, gap = ft.project_batch(pieces, pts)
    ft.assert_well_conditioned(f"breakpoints n={n}", ref, gap)
    fr, status, stats = rl.ops.frenet_host(pieces, pts)
    want = np.stack([s, np.full(len(s), n), np.zeros(len(s)), ref[0, :, 3]], 1)[None]
    compare(f"breakpoints n={n}", fr, want, L)
    check_stats(fr, status, stats)


def test_global_not_local_and_both_searches(rl):
    """Two parallel legs 6 m apart: a point 4 m off one leg towards the other belongs to the other.  257 points per line, so
    that a thread owns two consecutive points and the second starts from the first one's piece."""
    pieces = ft.two_leg_pieces()
    L = pieces[0][-1]
    P = 257
    pts = np.zeros((1, P, 2))
    pts[0, :, 0] = np.linspace(20.0, 80.0, P) + 0.0123
    pts[0, :, 1] = 4.0
    ref, gap = ft.project_batch(pieces, pts)
    ft.assert_well_conditioned("two legs", ref, gap)
    _, yfoot = ft.curve(pieces, ref[0, :, 0])
    assert (np.abs(yfoot - 6.0) < 0.05).all() and (np.abs(np.abs(ref[0, :, 1]) - 2.0) < 0.05).all()   # the twin: the other leg
    perm = np.random.default_rng(0).permutation(P)
    shuffled = np.ascontiguousarray(pts[:, perm])
    got = {}
    for search in (1, 0):
        rl.ctx.set_option("frenet_search", search)
        got[search] = rl.ops.frenet_host(pieces, pts)
        got[search, "shuffled"] = rl.ops.frenet_host(pieces, shuffled)
    rl.ctx.set_option("frenet_search", 1)
    compare("two legs", got[1][0], ref, L)
    for key in (0, (1, "shuffled"), (0, "shuffled")):
        order = perm if isinstance(key, tuple) else np.arange(P)
        np.testing.assert_array_equal(got[key][0][0], got[1][0][0, order])
        np.testing.assert_array_equal(got[key][1][0], got[1][1][0, order])
    np.testing.assert_array_equal(got[0][2], got[1][2])                   # the stats too
    np.testing.assert_array_equal(got[0, "shuffled"][2], got[1][2])


def test_both_searches_on_the_track(rl, rt):
    pieces = rt.centerline_pieces()
    pts = np.ascontiguousarray(ft.line_tables(rt, ptw.synthetic_frenet(rt, 257, 3, shift=0.37, amp_n=4.0)))
    rl.ctx.set_option("frenet_search", 0)
    full = rl.ops.frenet_host(pieces, pts)
    rl.ctx.set_option("frenet_search", 1)
    fast = rl.ops.frenet_host(pieces, pts)
    for a, b in zip(full, fast):
        np.testing.assert_array_equal(a, b)


def test_invariances_bitwise(rl, rt):
    pieces = rt.centerline_pieces()
    B, P = 5, 257
    pts = ft.line_tables(rt, ptw.synthetic_frenet(rt, P, B, amp_n=2.0, seed=3))
    pts[B - 1] = pts[0]                                                   # the same line at batch positions 0 and B - 1
    pts = np.ascontiguousarray(pts)
    fr, status, stats = rl.ops.frenet_host(pieces, pts)
    np.testing.assert_array_equal(fr[0], fr[B - 1])
    np.testing.assert_array_equal(stats[0], stats[B - 1])
    again = rl.ops.frenet_host(pieces, pts)                               # a repeated call
    for a, b in zip((fr, status, stats), again):
        np.testing.assert_array_equal(a, b)
    xy, yaw = np.ascontiguousarray(pts[:, :, :2]), np.ascontiguousarray(pts[:, :, 3])
    fr2, status2, stats2 = rl.ops.frenet_host(pieces, xy, yaw)            # stride 2 with the heading apart
    np.testing.assert_array_equal(fr2, fr)
    np.testing.assert_array_equal(stats2, stats)
    fr0, _, _ = rl.ops.frenet_host(pieces, xy)                            # no heading: xi = 0, nothing else moves
    assert (fr0[..., 2] == 0).all()
    np.testing.assert_array_equal(fr0[..., [0, 1, 3]], fr[..., [0, 1, 3]])
    import torch
    dev = torch.device("cuda", 0)
    out = rl.ops.frenet_torch(tuple(torch.from_numpy(a).to(dev) for a in pieces), torch.from_numpy(pts).to(dev))
    torch.cuda.synchronize()
    for a, b in zip((fr, status, stats), out):
        np.testing.assert_array_equal(a, b.cpu().numpy())


def test_status_of_bad_points(rl, rt):
    pieces = rt.centerline_pieces()
    B, P = 3, 257
    pts = np.ascontiguousarray(ft.line_tables(rt, ptw.synthetic_frenet(rt, P, B, amp_n=2.0, seed=4)))
    fr, status, stats = rl.ops.frenet_host(pieces, pts)
    bad = pts.copy()
    bad[0, 10, 0] = np.nan                                                # an even point: its thread's second point starts afresh
    bad[2, 101, 1] = np.inf
    bad[2, 256, 0] = -np.inf
    fr2, status2, stats2 = rl.ops.frenet_host(pieces, bad)
    hit = np.zeros((B, P), dtype=bool)
    hit[0, 10] = hit[2, 101] = hit[2, 256] = True
    assert (status2[hit] == 1).all() and (status2[~hit] == 0).all()
    assert np.isnan(fr2[hit]).all()
    np.testing.assert_array_equal(fr2[~hit], fr[~hit])                    # every other point to the bit
    np.testing.assert_array_equal(stats2[:, 0], [1, 0, 2])
    np.testing.assert_array_equal(stats2[1], stats[1])
    assert np.isfinite(stats2[:, 1:3]).all()
    with pytest.raises(ValueError, match="point 10 "):
        rt.global_to_frenet(bad[0, :, 0], bad[0, :, 1])
    got = rt.global_to_frenet(pts[1, :, 0], pts[1, :, 1], pts[1, :, 3])   # the public counterpart of frenet_to_global
    np.testing.assert_array_equal(got, fr[1, :, :3])


def test_argument_errors(rl, rt):
    lib, h = rl.ctx.lib, rl.ctx.h
    ss, cxs, cys = rt.centerline_pieces()
    M = len(ss) - 1
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    pts, out = np.zeros((2, 4, 19)), np.zeros((2, 4, 4))

    def call(points=pts, B=2, P=4, stride=19, ss_=ss, M_=M, out_=out):
        return lib.rl_frenet_batch_host(h, None if points is None else dp(points), B, P, stride, None,
                                        None if ss_ is None else dp(ss_), dp(cxs), dp(cys), M_, None if out_ is None else dp(out_),
                                        None, None)
    assert call() == 0
    for kw in (dict(points=None), dict(ss_=None), dict(out_=None), dict(B=0), dict(P=0), dict(M_=2), dict(stride=3), dict(stride=6)):
        assert call(**kw) == -1, kw                                        # RL_ERR_ARG
    fr, nodes, o2, st = np.zeros((2, 4, 4)), np.zeros(3), np.zeros((2, 3, 2)), np.zeros(2, dtype=np.int32)
    fr[:, :, 0] = np.arange(4.0)

    def rcall(fr_=fr, C=0, B=2, P=4, Nn=3, L=10.0, st_=st):
        return lib.rl_frenet_resample_host(h, None if fr_ is None else dp(fr_), None, C, B, P, dp(nodes), Nn, L, dp(o2),
                                           None if st_ is None else ip(st_))
    assert rcall() == 0 and (st == 0).all()
    for kw in (dict(fr_=None), dict(st_=None), dict(C=-1), dict(C=1), dict(B=0), dict(P=0), dict(Nn=0), dict(L=0.0)):
        assert rcall(**kw) == -1, kw
    with pytest.raises(rl.lib.RlError):
        rl.ctx.set_option("frenet_search", 2)


def test_resample_against_the_twin(rl, rt):
    pieces = rt.centerline_pieces()
    L = rt.center_s.get_length()
    B, P = 4, 257
    X = ptw.synthetic_frenet(rt, P, B, shift=0.37, amp_n=0.3, seed=6)
    pts = np.ascontiguousarray(ft.line_tables(rt, X))
    pts[1] = np.roll(pts[B - 1], P // 3, axis=0)                          # the shifted line, its first point rotated by P / 3
    pts[2, [40, 41]] = pts[2, [41, 40]]                                   # two points swapped
    fr, status, _ = rl.ops.frenet_host(pieces, pts)
    assert (status == 0).all()
    vals = np.ascontiguousarray(np.stack([pts[..., 4], np.cos(0.01 * fr[..., 0])], axis=-1))
    nodes = np.array(rt.abscissa, dtype=np.float64)                       # Nn = 103 != P
    nodes[5] = fr[0, 3, 0]                                                # a node exactly on a sample's s
    nodes = np.sort(nodes)
    smin = np.sort(fr[B - 1, :, 0])[0]
    assert nodes[0] == 0.0 and smin > 0.0                                 # node 0 lies inside the shifted line's wrap pair
    nodes[-1] = 0.5 * (np.sort(fr[B - 1, :, 0])[-1] + L)                  # and so does the last one, from the other side
    out, st = rl.ops.frenet_resample_host(fr, vals, nodes, L)
    np.testing.assert_array_equal(st, [0, 0, 1, 0])
    assert (out[2] == 0).all()
    for b in (0, 1, 3):
        ref, rst = ft.resample(fr[b], vals[b], nodes, L)
        d = float(np.abs(out[b] - ref).max())
        print(f"[frenet resample line {b}] against the twin {d:.2e}")
        assert rst == 0 and d <= TOL
    j = int(np.nonzero(nodes == fr[0, 3, 0])[0][0])
    assert out[0, j, 0] == fr[0, 3, 1] and out[0, j, 2] == vals[0, 3, 0]   # the sample itself
    np.testing.assert_array_equal(out[1], out[3])                         # where a line starts does not matter
    o0, s0 = rl.ops.frenet_resample_host(fr, None, nodes, L)              # no channels
    np.testing.assert_array_equal(o0, out[..., :2])
    np.testing.assert_array_equal(s0, st)


def _vehicle():
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    est = defaults.ESTIMATES
    return Vehicle(VehicleParams(np.array(est["acc_speed_loopup"]), np.array(est["dcc_speed_lookup"]), est["max_lon_acc_mpss"],
                                 est["max_lon_dcc_mpss"], est["max_left_acc_mpss"], est["max_right_acc_mpss"],
                                 est["max_speed_mps"], est["max_jerk_mpsc"]))


def test_chain_warm_start_from_lines(rl):
    """sweep-like lines -> tables -> QSS -> optimise_track_batch(start_points=...) on the MGKT problem at 8 m, B = 3."""
    import torch
    from mintime_problem import _load
    from test_optimality_cpu import TOL as KKT_TOL, double_track_nlp
    from test_optimality_gpu import _check_nlp
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    from spline_trajectory_optimization_amd.min_time_optm.min_time_optimizer import optimise_track_batch
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack
    from spline_trajectory_optimization_amd.simulator.simulator import Simulator
    rt = RaceTrack("MGKT", _load("MGKT_OUT_BOUND_enu.csv"), _load("MGKT_IN_BOUND_enu.csv"), _load("MGKT_CENTER_enu.csv"),
                   s=1.0, interval=8.0)
    veh = _vehicle()
    B, P = 3, 120
    s = np.ascontiguousarray(rt.abscissa, dtype=np.float64)
    N, L = len(s), float(rt.center_s.get_length())
    scales = width_scales(B)
    left = np.ascontiguousarray(rt.left_intp(s)[None] * scales[:, None])
    right = np.ascontiguousarray(rt.right_intp(s)[None] * scales[:, None])
    kw = dict(average_track_width=defaults.SOLVER["average_track_width"], speed_cap=defaults.SOLVER["speed_cap"], max_iter=160,
              tol=KKT_TOL)
    numpy_of = lambda res: {k_: v.cpu().numpy() for k_, v in res.items() if k_ != "track"}  # noqa: E731
    before = optimise_track_batch(rt, veh, defaults.MODEL, left, right, **kw)
    trk = before["track"]
    torch.cuda.synchronize()
    before = numpy_of(before)
    assert "start_status" not in before
    # the start lines: synthetic (s, n, xi) -> pose tables -> turn radius from the tables' own headings and distances -> QSS
    from spline_trajectory_optimization_amd.models.trajectory import _ring_coords
    pieces = rt.centerline_pieces()
    X = np.ascontiguousarray(ptw.synthetic_frenet(rt, P, B, amp_n=0.3, seed=8))
    trk.set_rings(_ring_coords(rt.left_r), _ring_coords(rt.right_r))
    lines = rl.ops.pose_tables_host(trk, rl.lib.POSE_FRENET, X, pieces, rl.lib.BOUNDS_SHARED_RINGS, None)
    for b in range(B):
        kap = rl.batch.signed_curvature(lines[b])
        lines[b, :, 5] = 1.0 / np.maximum(np.abs(kap), 1e-6)                # CURVATURE holds the unsigned turn radius
    lines, iters = rl.ops.qss_sim(lines, *rl.batch.vehicle_tables(veh))
    assert (iters >= 0).all() and (lines[..., 4] > 0).all()
    lines = np.ascontiguousarray(lines)
    # the guess itself against the twin
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    qss = rt.center_d.copy(); rt.fill_trajectory_boundaries(qss)
    base = Simulator(veh).run_simulation(qss, False).trajectory.points
    kappa = np.ascontiguousarray(rt.curvature_intp(s))
    swapped = lines.copy()
    swapped[2, [30, 31]] = swapped[2, [31, 30]]
    X0, U0, T0, st0 = (v.cpu().numpy() for v in rl.batch.min_time_guess_from_lines_torch(rt, up(swapped), up(s), up(kappa), up(base)))
    np.testing.assert_array_equal(st0, [0, 0, 1])
    ref, gap = ft.project_batch(pieces, swapped)
    ft.assert_well_conditioned("chain", ref, gap)
    for b in range(B):
        Xr, Tr, sr = ft.guess(ref[b], swapped[b, :, 4], s, kappa, L, base[:, 4], base[:, 16])
        dx, dt = float(np.abs(X0[b] - Xr).max()), float(np.abs(T0[b] - Tr).max())
        print(f"[frenet chain] guess of line {b}: status {st0[b]}, X0 against the twin {dx:.2e}, T0 {dt:.2e}")
        assert sr == st0[b] and dx <= TOL and dt <= TOL
    np.testing.assert_array_equal(U0, np.broadcast_to([1.0, -1.0, 0.001, 0.0], U0.shape))
    # the solves
    good = numpy_of(optimise_track_batch(rt, veh, defaults.MODEL, left, right, track=trk, start_points=lines, **kw))
    fall = numpy_of(optimise_track_batch(rt, veh, defaults.MODEL, left, right, track=trk, start_points=swapped, **kw))
    after = numpy_of(optimise_track_batch(rt, veh, defaults.MODEL, left, right, track=trk, **kw))
    np.testing.assert_array_equal(good["start_status"], [0, 0, 0])
    np.testing.assert_array_equal(fall["start_status"], [0, 0, 1])
    print(f"[frenet chain] iterations from the centre line {before['stats'][:, 0]}, from the lines {good['stats'][:, 0]}; "
          f"lap times {before['stats'][:, 4]} / {good['stats'][:, 4]}")
    assert (good["stats"][:, 5] == 1.0).all() and (fall["stats"][:, 5] == 1.0).all()
    for b in range(B):
        nlp = double_track_nlp(dict(s=s, kappa=kappa, left=left[b], right=right[b], L=L))
        _check_nlp(f"frenet chain row {b}", nlp, nlp.to_w(good["X"][b], good["U"][b], good["T"][b]), good["stats"][b])
    for k_ in ("X", "U", "T", "stats", "points", "summary"):
        np.testing.assert_array_equal(fall[k_][2], before[k_][2])          # the rejected line: the centre-line start, to the bit
        np.testing.assert_array_equal(after[k_], before[k_])               # and without the argument nothing has changed
