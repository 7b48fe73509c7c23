"""The optimiser kernels' OUTPUTS certified against reference-pinned functions (tests/kkt_certificate.py): the returned point of
k_global_qp / k_global_qp2 / k_global_xy, k_bk_iter and k_mt_* is a first-order optimum of the problem as the independent
evaluators state it -- no CPU twin takes part.  Bounds and the CPU measurements behind them: tests/test_optimality_cpu.py.

For n_outer = m > 1 the QP that the last linearisation solved is the one assembled at the run's own a_{m-1}.  That is NOT the
result of a plain call with n_outer = m - 1 (it converges its last QP further: 1.16e-2 m apart on Monza c30, margin 2 m): the
(m-1)-call is made with the test hook "global_last_as_mid" on, which returns the run's a_{m-1} bit for bit (the kernels are
bit-reproducible: test_global_qp.py::test_global_batch_properties_full_size), and a_m is certified on qp_at(a_{m-1}).  With both
coordinates free the kernel then takes the whole or the half step (stats[7] counts the halved ones); the QP's own answer is
recovered from either.  The shared case list, the procedure and the exact optimum a* beside each certificate:
tests/global_kkt_cases.py.

Measured on the MI355X (first run with the hook; stat / compl / viol, in brackets stat and compl as shares of their bounds;
iterations; |a - a*|_inf against the bound of 1e-4 m):
  two-front k3_np56 N=1000        n_outer 1 / 3: 2.26e-07 / 2.30e-11 / 8.9e-16 (0.005 / 0.000), 7.94e-09 / 2.18e-10 / 0
  two-front k5_few_knots N=1000   n_outer 1 / 3: 1.89e-09 / 8.04e-10 / 2.0e-12, 1.31e-09 / 8.97e-10 / 4.4e-12
  Monza c100 N=500 margin 0.25    n_outer 1 / 3 / 6: 2.06e-08 / 6.85e-11, 2.05e-09 / 9.40e-11, 1.74e-09 / 9.38e-11 (all 0.000 / 0.000);
                                  c30 n_outer 3: 9.05e-09 / 3.04e-11 / 2.1e-12
  xy Monza c100 N=500             n_outer 1 / 3: 2.62e-05 / 1.67e-10 / 5.0e-13 (0.109 / 0.000), 1.00e-06 / 1.70e-10 / 4.4e-12 (0.004)
  the shared list (X = expected failure, strict):
  one-kart_c-N400-m2.0-o1       X 1.37e-05 / 2.46e-08 / 0   (1.234 / 0.421)  ipm 14  1.09e-04 m
  one-kart_c-N400-m2.0-o2         4.06e-08 / 2.06e-11 / 0   (0.003 / 0.000)  ipm 25  2.38e-07 m
  one-kart_c-N400-m2.0-o3         5.79e-09 / 7.16e-12 / 0   (0.000 / 0.000)  ipm 34  2.98e-08 m
  one-kart_c-N800-m0.25-o3      X 2.74e-05 / 4.44e-08 / 0   (1.062 / 1.419)  ipm 40  1.46e-04 m
  one-kart_c-N800-m2.0-o2         3.17e-09 / 7.30e-12 / 0   (0.000 / 0.000)  ipm 27  1.06e-08 m
  one-kart_c-N200-m1.0-o2         8.40e-09 / 6.50e-12 / 0   (0.000 / 0.000)  ipm 21  7.30e-09 m
  one-kart_c-N400-m1.0-o3         2.89e-06 / 6.16e-10 / 0   (0.138 / 0.016)  ipm 30  6.00e-05 m
  one-kart_cb-N400-m1.5-o2        1.19e-08 / 9.88e-12 / 0   (0.001 / 0.000)  ipm 24  5.55e-09 m   (generic kernel, n_p = 67)
  one-kart_c-N400-m0.25-o1        1.79e-08 / 9.80e-11 / 0   (0.002 / 0.004)  ipm 13  1.63e-08 m
  one-kart_c-N400-m0.25-o6        2.00e-09 / 7.70e-12 / 0   (0.000 / 0.000)  ipm 50  3.96e-09 m
  one-kart_c-N400-m0.25-o3-v1     2.18e-09 / 3.71e-11 / 0   (0.000 / 0.001)  ipm 35  5.50e-09 m   (RL_GLOBAL_V1=1, child process)
  one-monza_c30-N500-m2.0-o3      1.15e-08 / 2.81e-11 / 1.2e-12 (0.000 / 0.000)  ipm 41  2.79e-06 m
  one-monza_c100-N500-m2.0-o3   X 1.16e-05 / 1.69e-10 / 2.2e-12 (0.063 / 0.000)  ipm 49  1.13e-03 m
  one-monza_c100_off1.05 o1 / o3  5.19e-08 / 5.96e-11, 6.76e-09 / 7.59e-11 (0.000 / 0.000)  ipm 28, 53  8.11e-08, 8.30e-08 m
  one-monza_c100_off1.5  o1 / o3  5.11e-07 / 4.94e-10 (0.003 / 0.001), 8.26e-09 / 1.58e-10  ipm 27, 59  3.17e-06, 2.10e-07 m
  weighted kart_c m1.0 o1 speed / exp2   7.31e-09 / 7.43e-11, 1.08e-07 / 6.03e-12 (0.004)  ipm 14, 15  1.66e-07, 3.93e-08 m
  weighted kart_c m1.0 o3 speed / exp2   3.61e-09 / 1.04e-09 (0.000 / 0.017), 1.65e-08 / 1.80e-11  ipm 35, 41  1.67e-06, 1.30e-08 m
  weighted monza_c100 o3 speed           1.35e-09 / 1.15e-10 / 3.0e-12 (0.000 / 0.000)  ipm 45  1.57e-07 m
  weighted monza_c100 o3 exp2          X 1.55e-06 / 8.94e-11 / 2.9e-12 (0.002 / 0.000)  ipm 51  3.13e-04 m
  xy-kart_c-N400-m0.25 o1 / o3    1.93e-08 / 1.09e-11 (0.001), 3.60e-08 / 2.23e-10 (0.001 / 0.005)  ipm 18, 56  6.36e-07, 1.40e-05 m
  xy-kart_c-N400-m1.0  o1 / o3    8.51e-08 / 1.32e-09 (0.005 / 0.018), 4.66e-08 / 8.90e-12 (0.002)  ipm 19, 56  2.85e-05, 6.46e-07 m
  xy-kart_c-N400-m2.0-o1        X 4.51e-06 / 6.95e-09 / 0   (0.261 / 0.083)  ipm 17  7.65e-04 m
  xy-kart_c-N400-m2.0-o3        X 1.86e-06 / 7.32e-10 / 0   (0.106 / 0.008)  ipm 52  9.49e-04 m
  batch of four (kart_c m1.0 o3, widths x 1.0 / 0.9 / 1.1 / 1.0): stat 0.138 / 0.001 / 0.150 / 0.138 of the bound,
                                  6.00e-05 / 1.47e-07 / 1.10e-06 / 6.00e-05 m, rows 0 and 3 bit-identical with and without the hook
The six X cases fail on the CPU twins with the same figures: the last linearisation leaves at complementarity 1e-10 (a mean over
2N rows), which is not enough there; 1e-12 cures the four one-offset cases on the twins and is not survived by the kernels (NaN
on one Monza instance, 5.5e-6 m between k_global_xy and its twin), so the rule stays and the cases stay, strict.  The
hooked and the plain (m-1)-result of Monza c30 margin 2 m: 1.16e-2 m apart.  Empty corridor (test_global_qp.py): 0.3 m short ->
stats[3] = 0.150 m, 240 iterations, finite."""
import numpy as np
import pytest

import os
import subprocess
import sys

import bicycle_problem as bp
import bicycle_twin as bt
import global_kkt_cases as gk
import kkt_certificate as kc
from test_global_qp import MARGIN, NumpyGlobal, monza_widths
from test_global_qp_xy import LON, NumpyGlobalXY
from test_optimality_cpu import TOL, double_track_nlp, nlp_bounds, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch = _lib, ops, batch
    return ns


# ---------------------------------------------------------------------------------------------------------- the QPs
def _check_qp(tag, cert, bounds, st):
    report(tag, cert, bounds)
    assert cert.viol <= bounds[2]
    assert cert.stat <= bounds[0] and cert.compl <= bounds[1]
    assert cert.viol <= st[3] + bounds[2]                    # the kernel's own violation figure does not under-report


def _certify_global(rl, tag, t, cx, cy, k, u, wl, wr, n_outer):
    N = len(u)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    W = np.stack([wl, wr], 1)[None]
    ng = NumpyGlobal(t, cx, cy, k, u)
    a_prev = np.zeros(ng.np)
    if n_outer > 1:                    # the run's own a_{m-1}: the (m-1)-call with the hook on (tests/global_kkt_cases.py)
        with gk.hook(trk.ctx):
            a_prev = rl.ops.global_batch_host(trk, W, MARGIN, n_outer - 1)[2][0]
    _, _, a, st, rs = rl.ops.global_batch_host(trk, W, MARGIN, n_outer)
    P, q, A = ng.qp_at(a_prev)
    cert, bounds = kc.certify_qp(P, q, A, -(wr - MARGIN), wl - MARGIN, a[0])
    _check_qp(f"global qp {tag} N={N} n_p={ng.np} outer={n_outer} block={rs.block_threads}", cert, bounds, st[0])
    return rs


@pytest.mark.parametrize("n_outer", [1, 3])
@pytest.mark.parametrize("shape", ["k3_np56", "k5_few_knots"])
def test_two_front_kernel_output_is_a_kkt_point(rl, shape, n_outer):
    """k_global_qp2 (n_p <= 64): the shapes of test_global_qp.py::test_two_front_factorisation_shapes."""
    from spline_trajectory_optimization_amd.models.trajectory import BSplineTrajectory
    N = 1000
    centre, _, _ = rl.batch.load_monza()
    s_, k_ = {"k3_np56": (100.0, 3), "k5_few_knots": (1e5, 5)}[shape]
    t, cx, cy, k = BSplineTrajectory(centre, s_, k_)._tck()
    assert len(cx) - k <= 64
    wl = np.full(N, 5.0) + np.sin(np.arange(N) * 0.02); wr = np.full(N, 4.5) + np.cos(np.arange(N) * 0.03)
    rs = _certify_global(rl, shape, t, cx, cy, k, np.linspace(0, 1, N, endpoint=False), wl, wr, n_outer)
    assert rs.block_threads > 64 and rs.block_threads % 64 == 0          # the wave-specialised kernel ran


@pytest.mark.parametrize("tag,n_outer", [("c100", 1), ("c100", 3), ("c100", 6), ("c30", 3)])
def test_global_kernel_output_is_a_kkt_point(rl, fits, tag, n_outer):
    t, cx, cy, k, u, wl, wr = monza_widths(fits, tag, 500)
    _certify_global(rl, tag, t, cx, cy, k, u, wl, wr, n_outer)


@pytest.mark.parametrize("n_outer", [1, 3])
def test_global_xy_kernel_output_is_a_kkt_point(rl, fits, n_outer):
    """k_global_xy (dof = 2), lateral and +-1 m longitudinal rows."""
    N = 500
    t, cx, cy, k, u, wl, wr = monza_widths(fits, "c100", N)
    trk = rl.lib.Track(rl.lib.Context.get(0), t, cx, cy, k, N)
    W = np.stack([wl, wr], 1)[None]
    ng = NumpyGlobalXY(t, cx, cy, k, u)
    z_prev, halved_before = np.zeros((ng.np, 2)), 0
    if n_outer > 1:                    # the run's own z_{m-1}: the (m-1)-call with the hook on
        with gk.hook(trk.ctx):
            _, _, zp, stp, _ = rl.ops.global_batch_host(trk, W, MARGIN, n_outer - 1, dof=2, lon=LON)
        z_prev, halved_before = zp[0], int(stp[0, 7])
    _, _, z, st, rs = rl.ops.global_batch_host(trk, W, MARGIN, n_outer, dof=2, lon=LON)
    halved = int(st[0, 7]) - halved_before
    assert halved in (0, 1)
    x = z_prev + (z[0] - z_prev) * (2.0 if halved else 1.0)               # the QP's own answer
    P, q, A = ng.qp_at(z_prev)
    lo = np.concatenate([-(wr - MARGIN), -LON * np.ones(N)]); hi = np.concatenate([wl - MARGIN, LON * np.ones(N)])
    cert, bounds = kc.certify_qp(P, q, A, lo, hi, x)
    report(f"global xy c100 N={N} outer={n_outer} last step halved={halved}", cert, bounds)
    assert cert.viol <= bounds[2] and cert.stat <= bounds[0] and cert.compl <= bounds[1]
    lat, lon = ng.offsets(z[0])                                           # the RETURNED line (whole or half step) is inside
    viol = max((lat - (wl - MARGIN)).max(), (-(wr - MARGIN) - lat).max(), np.abs(lon).max() - LON, 0.0)
    assert viol <= bounds[2] and viol <= st[0, 3] + bounds[2]


# ------------------------------------------------------------------ the shared case list (tests/global_kkt_cases.py)
@pytest.fixture(scope="module")
def kernels(rl):
    return gk.KernelSolver()


@pytest.mark.parametrize("c", gk.params())
def test_global_kernel_output_is_a_kkt_point_of_its_own_linearisation(kernels, c, tmp_path):
    """Every case on the kernels; the RL_GLOBAL_V1 case (the generic kernel on n_p <= 64; the switch is read when the context is
    created) solves in a process of its own, tests/global_kkt_run.py, and is certified here."""
    if c.env:
        f = str(tmp_path / "r.npz")
        subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "global_kkt_run.py"), f, c.id],
                       check=True, env=dict(os.environ, **c.env), timeout=300)
        d = np.load(f)
        r = d["x"], d["st"], d["xp"], d["stp"]
        plain = gk.case(c.kind, c.track, c.N, c.margin, c.n_outer)
        gk.solve_case(kernels, plain)
        assert int(d["block_threads"]) != kernels.last_rs.block_threads                  # another kernel ran in the child
    else:
        r = gk.solve_case(kernels, c)
    print(f"    block {kernels.last_rs.block_threads} lds {kernels.last_rs.lds_bytes}")
    gk.assert_case(c, *r, gk.certify_case(c, *r, report))


def test_hook_off_is_the_context_that_never_set_it(rl, kernels):
    """A context of its own that never saw the option against the cached one after the hook was on and off again: the same
    bits, all three entries.  The hooked (m-1)-result is another point than the plain one, by far more than any bound (Monza c30
    N = 500 margin 2.0: measured on the twin 1.2e-2 m) -- which is why certifying on the plain one failed off Monza c100."""
    c = gk.by_id(gk.OLD_PREMISE_CASE)
    inp, W = gk.inputs(c.track, c.N), gk.widths_of(c)
    w = gk.weights_of("speed", c.N)
    fresh = gk.KernelSolver(rl.lib.Context(0))
    on = kernels.one(inp, W, c.margin, c.n_outer - 1, True)
    d = np.abs(on[0] - fresh.one(inp, W, c.margin, c.n_outer - 1, False)[0]).max()
    print(f"[{c.id}] hooked against unhooked (m-1)-result: {d:.2e} m")
    assert d > 1e-5
    for strict, call in ((True, lambda s, h: s.one(inp, W, c.margin, 2, h)),
                         (True, lambda s, h: s.one(inp, W, c.margin, 2, h, weights=w)),
                         (False, lambda s, h: s.xy(inp, W, c.margin, LON, 2, h))):   # (1e-9 against 1e-10: one iteration may pass both)
        never, hooked, off = call(fresh, False), call(kernels, True), call(kernels, False)
        assert never[0].tobytes() == off[0].tobytes() and never[1].tobytes() == off[1].tobytes()
        assert hooked[1][0, 0] <= off[1][0, 0]
        if strict:
            assert hooked[1][0, 0] < off[1][0, 0] and hooked[0].tobytes() != off[0].tobytes()
    with pytest.raises(rl.lib.RlError):
        kernels.ctx.set_option("global_last_as_mid", 2)


# --------------------------------------------------------------------------------------------------------- the NLPs
def _check_nlp(tag, nlp, w, st):
    inp, err = nlp.certificate_inputs(w)
    cert = kc.certify(**inp)
    prod = kc.fd_error_in_stationarity(err, cert)
    bounds = nlp_bounds(cert, prod)
    j, k, r = kc.worst_block(nlp, cert)
    report(tag, cert, bounds, prod)
    print(f"    kernel's own dual / viol / compl {st[1]:.2e} / {st[2]:.2e} / {st[3]:.2e}, iterations {st[0]:.0f}; "
          f"largest stationarity entry at node {j}, unknown {k}")
    assert st[5] == 1.0
    assert cert.viol <= bounds[2]
    assert cert.stat <= bounds[0] and cert.compl <= bounds[1]
    # the kernel's own residuals do not under-report: the independent ones stay within the same factor of 10 of them
    assert max(cert.viol, cert.stat / cert.s_d, cert.compl / cert.s_c) <= 10 * max(st[1], st[2], st[3])


def _bicycle_data(track):
    pts = {"oval48": lambda: bp.oval_table(48), "ring128": lambda: bp.ring_table(128),
           "monza20": lambda: bp.monza_table(20.0)[0]}[track]()
    return bp.table_data(pts)


@pytest.mark.parametrize("track", ["oval48", "ring128", "monza20"])
def test_bicycle_kernel_output_is_a_kkt_point(rl, track):
    P0, yaw, dl, dr = _bicycle_data(track)
    X0, U0, T0 = bt.initial_guess("centerline", P0, yaw)
    X, U, T, st = rl.ops.bicycle_solve_batch(bp.MODEL, P0, yaw, dl, dr, X0[None], U0[None], T0[None], max_iter=200, tol=TOL)
    nlp = kc.BicycleNLP(bp.MODEL, P0, yaw, dl, dr)
    _check_nlp(f"bicycle {track} N={len(yaw)}", nlp, nlp.to_w(X[0], U[0], T[0]), st[0])


def test_bicycle_batch_rows_are_kkt_points_of_their_own_widths(rl):
    """One B = 4 launch with per-instance widths: instances 0 and 3 against THEIR bounds."""
    P0, yaw, dl, dr = _bicycle_data("oval48")
    B = 4
    DL, DR = bp.perturbed_widths(dl, dr, B, seed=3)
    X0, U0, T0 = bt.initial_guess("centerline", P0, yaw)
    rep = lambda a: np.repeat(a[None], B, axis=0)  # noqa: E731
    X, U, T, st = rl.ops.bicycle_solve_batch(bp.MODEL, P0, yaw, DL, DR, rep(X0), rep(U0), rep(T0), max_iter=200, tol=TOL)
    assert np.abs(DL[0] - DL[3]).max() > 0.05                             # the instances do differ
    for b in (0, 3):
        nlp = kc.BicycleNLP(bp.MODEL, P0, yaw, DL[b], DR[b])
        _check_nlp(f"bicycle oval48 batch row {b}", nlp, nlp.to_w(X[b], U[b], T[b]), st[b])


@pytest.fixture(scope="module")
def mgkt8():
    from mintime_problem import mgkt_problem
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    d = mgkt_problem(8.0, defaults.ESTIMATES)
    nlp = double_track_nlp(d)
    X0 = np.zeros((nlp.N, 6)); X0[:, 0] = d["s"]; X0[:, 5] = np.maximum(d["speed"], 1.5)       # the reference's guess
    U0 = np.tile(np.array([1.0, 0.0, 0.001, 0.0]), (nlp.N, 1))                               # (min_time_optimizer.py:146-151)
    T0 = np.maximum(d["seg_time"], 1e-3)
    return d, nlp, X0, U0, T0


def _solve_dt(rl, d, nlp, left, right, X0, U0, T0):
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    return rl.ops.mintime_solve_batch(nlp.m, d["s"], d["kappa"], left, right, nlp.margin, d["L"], X0, U0, T0,
                                      average_track_width=defaults.SOLVER["average_track_width"],
                                      speed_cap=defaults.SOLVER["speed_cap"], max_iter=150, tol=TOL)


def test_double_track_kernel_output_is_a_kkt_point(rl, mgkt8):
    d, nlp, X0, U0, T0 = mgkt8
    X, U, T, st = _solve_dt(rl, d, nlp, d["left"], d["right"], X0[None], U0[None], T0[None])
    assert np.abs(U[0, :, 1]).max() == 0.0                                # the control that the formulation holds at 0
    _check_nlp(f"double track mgkt 8 m N={nlp.N}", nlp, nlp.to_w(X[0], U[0], T[0]), st[0])


def test_double_track_batch_rows_are_kkt_points_of_their_own_widths(rl, mgkt8):
    d, nlp0, X0, U0, T0 = mgkt8
    scale = np.array([1.0, 0.92, 1.1, 1.2])
    B = len(scale)
    left, right = d["left"][None] * scale[:, None], d["right"][None] * scale[:, None]
    rep = lambda a: np.repeat(a[None], B, axis=0)  # noqa: E731
    X, U, T, st = _solve_dt(rl, d, nlp0, left, right, rep(X0), rep(U0), rep(T0))
    for b in (0, 3):
        nlp = double_track_nlp(dict(d, left=left[b], right=right[b]))
        _check_nlp(f"double track mgkt 8 m batch row {b}", nlp, nlp.to_w(X[b], U[b], T[b]), st[b])
