"""The optimality certificate of tests/kkt_certificate.py discriminates (CPU only; the kernels' outputs are certified in
tests/test_optimality_gpu.py).

Accepted: the SLSQP solution of the 16-node bicycle oval (a point that neither the twin nor the kernel computed) and the
twins' converged answers (global QP c100 N = 500 n_outer = 1, bicycle oval 48, double track on MGKT at 8 m).  Rejected:
each of those moved 1e-4 along the null space of its active constraints, each with its most loaded binding row pushed 1e-3
inside, and for the QP the unconstrained minimiser clipped into the bounds.  Self-consistent: on a 6-unknown convex QP with a
closed-form solution the multipliers come back to 1e-10, and the module's sparse solver agrees with scipy's lsq_linear.

Bounds.  QPs: stationarity 1e-6 |q|_inf, complementarity 1e-8 max(1, |z|_inf), violation 1e-9 m (kkt_certificate.certify_qp).
NLPs, solved to the scaled KKT error tol = 1e-6: stationarity 10 tol s_d, complementarity 10 tol s_c, violation 1e-6, with
IPOPT's s_d, s_c from the certificate's own multipliers; the stationarity bound is raised to the finite-difference Jacobians'
own error times the multipliers (entry by entry) should that ever be larger.

Measured here, on the CPU, before any bound was fixed (stat / compl / viol; NLP bound 1e-5 with s_d = s_c = 1):
  SLSQP, bicycle oval 16          2.0e-11 / 5.5e-11 / 4.1e-12
  bicycle twin, oval 16, tol 1e-9 4.8e-11 / 1.3e-10 / 5.0e-14
  bicycle twin, oval 48, tol 1e-9 1.0e-11 / 1.1e-10 / 1.4e-11       tol 1e-6: 9.8e-09 / 1.1e-07 / 7.9e-13
  bicycle twin, ring 128, tol 1e-6 1.8e-12 / 1.0e-07 / 1.2e-10      Monza 20 m, tol 1e-6: 3.5e-08 / 1.5e-07 / 2.6e-11
  double-track twin, MGKT 8 m, tol 1e-6: 4.5e-08 / 1.8e-07 / 1.4e-14;  at tol 1e-9 the twin runs out of its 150 iterations
      (dual infeasibility 4.8e-6 by its own count) at a point with 1.1e-09 / 1.1e-08 / 1.1e-13, s_d = 3.3
  global QP twin c100 N = 500: n_outer 1 / 3 / 6: stat 2.1e-08 / 1.3e-06 / 4.8e-09 of 1.7e-04, compl 6.9e-11 .. 9.5e-11 of
      5.4e-07 .. 8.6e-07;  c30 N = 500 n_outer 1 / 2 / 3: stat 2.2e-06 / 4.0e-05 / 1.3e-06 of 5.8e-05 .. 9.0e-05
      -- the n_outer > 1 figures of this line were taken on the WRONG QP (below); on the right one the kernels give 2.1e-09 /
      1.7e-09 for c100 n_outer 3 / 6 and 9.1e-09 for c30 n_outer 3 (tests/test_optimality_gpu.py's docstring)
so the points solved to 1e-9 and SLSQP's sit 4 decades under the NLP bound and the 1e-6 twins 55 times under it.  The
Jacobians' own error times the multipliers: 6e-11 (bicycle), 1.4e-07 (double track: the tanh and max rows), under every bound.

The global QPs on the linearisation they solved (tests/global_kkt_cases.py; the case list is shared with the GPU module).
This docstring used to say that the c30 QP after TWO linearisations uses 45 % of its stationarity bound because the
interior-point loop leaves on the complementarity alone.  That diagnosis was wrong.  The 45 % came from certifying a_m on the
QP assembled at the result of a plain (m-1)-call, which is not the point that the m-run linearised about: the plain call
leaves its last QP at mu < 1e-10, the m-run left the same QP at 1e-7, and the two points differ by 3.0e-4 .. 1.2e-2 m
(measured: Monza c30 N = 500 margin 2.0, 1.16e-2 m, 28 against 30 iterations).  Off Monza c100 / margin 0.25 the wrong point
fails correct output: kart c N = 400 margin 2.0 n_outer 2 1.63x the stationarity bound, Monza c30 margin 2.0 n_outer 3 2.39x
(test_old_premise_is_rejected); with the twins' switch for the library's hook "global_last_as_mid" the (m-1)-call returns the
run's own a_{m-1} and the same cases sit at 0.003x and 0.000x.
Measured with the hook (stationarity, complementarity as shares of their bounds; |a - a*|_inf, bound 1e-4 m), X = fails:
  kart c N=400 m 2.0 n_outer 1 / 2 / 3     X 1.234 0.421 1.09e-4 | 0.003 0.000 2.4e-7 | 0.000 0.000 3.0e-8
  kart c N=800 m 0.25 o3 / m 2.0 o2        X 1.060 1.418 1.46e-4 | 0.000 0.000 1.1e-8
  kart c N=200 m 1.0 o2, N=400 m 1.0 o3      0.000 0.000 7.7e-9  | 0.138 0.016 6.0e-5;   cb N=400 m 1.5 o2: 0.001 0.000 5.6e-9
  kart c N=400 m 0.25 n_outer 1 / 6 / 3      0.002 0.004 1.6e-8  | 0.000 0.000 4.0e-9 | 0.000 0.001 5.5e-9
  Monza m 2.0 o3: c30 / c100                 0.000 0.000 2.9e-6  | X 0.063 0.000 1.13e-3
  corridor moved off 1.05 o1 / o3, 1.5 o1 / o3: 0.000 8.1e-8 | 0.000 1.2e-7 | 0.003 3.2e-6 | 0.000 2.4e-7
  weighted kart c m 1.0 o1 speed / exp2, o3 speed / exp2: 0.001 1.7e-7 | 0.004 3.9e-8 | 0.000 (compl 0.017) 1.7e-6 | 0.000 1.3e-8
  weighted Monza c100 o3 speed / exp2        0.000 4.7e-7 | X 0.002 0.000 3.13e-4
  xy kart c N=400 m 0.25 o1 / o3, 1.0 o1 / o3: 0.001 6.4e-7 | 0.001 1.4e-5 | 0.005 2.9e-5 | 0.002 6.4e-7
  xy kart c N=400 m 2.0 o1 / o3            X 0.261 0.083 7.65e-4 | X 0.106 0.008 9.49e-4
  the polished optimum a* itself: stationarity <= 9.7e-9 of its bound in every case (asserted: 1e-3)
The six X cases are real: the solver's own residuals are at 1e-12 there, what remains is complementarity, whose mean over the 2N
rows the exit rule bounds and whose maximum the certificate bounds.  With the last linearisation left at 1e-11 / 1e-12 / 1e-13
the distances are 6.9e-6 / 1.6e-8 / 1.6e-8, 2.5e-6 / 2.5e-6 / 1.2e-8, 1.08e-4 / 8.1e-7 / 8.1e-7, 2.3e-6 / 2.3e-6 / 5.6e-8 m for the
four one-offset cases (1e-12 is the loosest power of ten at which all pass: test_last_threshold_1e12_would_certify) and
2.85e-4 / 1.02e-4 / NaN, 1.85e-4 / 1.85e-4 / 7.3e-6 m for the two with both coordinates free, which no threshold cures.  The
kernels do not survive 1e-12, so the rule stays at 1e-10 and the cases stay in the list, xfail(strict=True).

Measured on the MI355X (first run of tests/test_optimality_gpu.py): see that module's docstring."""
import numpy as np
import pytest
from scipy.linalg import null_space

import bicycle_problem as bp
import bicycle_twin as bt
import global_kkt_cases as gk
import kkt_certificate as kc
from oracle import oracle as orc
from test_global_qp import MARGIN, NumpyGlobal, monza_widths

TOL = 1e-6


def nlp_bounds(cert, fd_prod, tol=TOL):
    """(stat, compl, viol) bounds of an NLP solved to the scaled KKT error `tol`."""
    return max(10 * tol * cert.s_d, fd_prod), 10 * tol * cert.s_c, 1e-6


class NlpCase:
    def __init__(self, name, nlp, w, me):
        self.name, self.nlp, self.x, self.me = name, nlp, w.reshape(-1), me

    def run(self, x):
        inp, err = self.nlp.certificate_inputs(x.reshape(self.nlp.N, self.nlp.nv))
        cert = kc.certify(**inp)
        prod = kc.fd_error_in_stationarity(err, cert)
        return cert, nlp_bounds(cert, prod), inp, prod


class QpCase:
    def __init__(self, name, P, q, A, lo, hi, a):
        self.name, self.P, self.q, self.A, self.lo, self.hi, self.x = name, P, q, A, lo, hi, a.reshape(-1)

    def run(self, x):
        cert, bounds = kc.certify_qp(self.P, self.q, self.A, self.lo, self.hi, x)
        return cert, bounds, kc.qp_rows(self.P, self.q, self.A, self.lo, self.hi, x), 0.0


def report(tag, cert, bounds, prod=0.0):
    print(f"[{tag}] stat {cert.stat:.2e} (bound {bounds[0]:.2e})  compl {cert.compl:.2e} (bound {bounds[1]:.2e})  "
          f"viol {cert.viol:.2e} (bound {bounds[2]:.0e})  s_d {cert.s_d:.2f}  jacobian error x multipliers {prod:.1e}")


def accepted(cert, bounds):
    return cert.stat <= bounds[0] and cert.compl <= bounds[1] and cert.viol <= bounds[2]


# ------------------------------------------------------------------------------------------------- the accepted points
def _bicycle(N):
    P0, yaw, dl, dr = bp.table_data(bp.oval_table(N))
    return bt.Problem(bp.MODEL, P0, yaw, dl, dr), kc.BicycleNLP(bp.MODEL, P0, yaw, dl, dr), P0, yaw


@pytest.fixture(scope="module")
def slsqp_oval16():
    """The set-up of test_bicycle_cpu.py::test_twin_matches_slsqp_on_a_16_node_oval, with the rows and their derivatives from
    the mirrors (kkt_certificate.BicycleNLP) so that the point owes nothing to the twin."""
    from scipy.optimize import minimize
    prob, nlp, P0, yaw = _bicycle(16)
    X0, U0, T0 = bt.initial_guess("centerline", P0, yaw)
    w0 = nlp.to_w(X0, U0, T0).ravel()
    nbox = nlp.rows(w0.reshape(1, 16, 8))[1].shape[2] - 3

    def fun(w):
        c, d = nlp.rows(w.reshape(1, 16, 8))
        return c[0].ravel(), d[0, :, :3].ravel()

    def jac(w):
        inp, _ = nlp.certificate_inputs(w.reshape(16, 8))
        keep = (np.arange(16)[:, None] * (3 + nbox) + np.arange(3)[None]).ravel()
        return inp["Jc"].toarray(), inp["Jd"].toarray()[keep]
    lo = np.r_[nlp.lo, 0.0]; hi = np.r_[nlp.hi, np.inf]
    bounds = [(None if not np.isfinite(a) else a, None if not np.isfinite(b) else b) for a, b in zip(np.tile(lo, 16), np.tile(hi, 16))]
    grad = np.zeros(128); grad[7::8] = 1.0
    res = minimize(lambda w: w[7::8].sum(), w0, jac=lambda w: grad, method="SLSQP", bounds=bounds,
                   constraints=[{"type": "eq", "fun": lambda w: fun(w)[0], "jac": lambda w: jac(w)[0]},
                                {"type": "ineq", "fun": lambda w: -fun(w)[1], "jac": lambda w: -jac(w)[1]}],
                   options={"maxiter": 1000, "ftol": 1e-14})
    assert res.status in (0, 8), res.message     # 8: its line search ran out of digits at the optimum (test_bicycle_cpu.py)
    X, U, T, st = bt.solve(prob, X0, U0, T0, max_iter=200, tol=1e-9)
    assert abs(res.fun - T.sum()) <= 1e-6 * T.sum()          # the same optimum as the twin's, found another way
    return NlpCase("slsqp oval16", nlp, res.x, 6)


@pytest.fixture(scope="module")
def twin_oval48():
    prob, nlp, P0, yaw = _bicycle(48)
    X0, U0, T0 = bt.initial_guess("centerline", P0, yaw)
    X, U, T, st = bt.solve(prob, X0, U0, T0, max_iter=200, tol=TOL)
    assert st[5] == 1.0
    return NlpCase("bicycle twin oval48", nlp, nlp.to_w(X, U, T), 6)


@pytest.fixture(scope="module")
def twin_qp(fits):
    t, cx, cy, k, u, wl, wr = monza_widths(fits, "c100", 500)
    a = orc.global_mincurv(t, cx, cy, k, 500, wl, wr, MARGIN, 1)[3]
    ng = NumpyGlobal(t, cx, cy, k, u)
    P, q, A = ng.qp_at(np.zeros(ng.np))
    return QpCase("global qp twin c100 N=500", P, q, A, -(wr - MARGIN), wl - MARGIN, a)


def double_track_nlp(d):
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    return kc.DoubleTrackNLP(defaults.MODEL, d["s"], d["kappa"], d["left"], d["right"], d["L"],
                             defaults.SOLVER["average_track_width"], defaults.SOLVER["speed_cap"])


@pytest.fixture(scope="module")
def twin_mgkt():
    from mintime_problem import mgkt_problem
    from oracle import sqp_twin as tw
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    d = mgkt_problem(8.0, defaults.ESTIMATES)
    P = tw.Problem(defaults.MODEL, d["s"], d["kappa"], d["left"], d["right"], d["L"],
                   defaults.SOLVER["average_track_width"], defaults.SOLVER["speed_cap"])
    w, info = tw.solve(P, tw.initial_point(P, d["speed"], d["seg_time"]), max_iter=150, tol=TOL)
    assert info["status"] == 1
    nlp = double_track_nlp(d)
    X, U, T = P.unpack(w)
    return NlpCase("double-track twin mgkt 8 m", nlp, nlp.to_w(X, U, T), 7)


CASES = ["slsqp_oval16", "twin_oval48", "twin_qp", pytest.param("twin_mgkt", marks=pytest.mark.slow)]


@pytest.fixture(params=CASES)
def case(request):
    return request.getfixturevalue(request.param)


def _binding(inp, cert):
    """The rows the PERTURBATIONS below treat as binding: the multiplier's pull on the gradient, z |J_i|, larger than the row's
    distance in the unknowns, |d_i| / |J_i| (an interior-point answer leaves a binding row mu / z inside and gives every
    other row mu / slack; the certificate itself has no such rule)."""
    Jd = inp["Jd"].toarray() if hasattr(inp["Jd"], "toarray") else np.asarray(inp["Jd"])
    nrm = np.maximum(np.linalg.norm(Jd, axis=1), 1e-300)      # (a row without any derivative binds nothing)
    return np.where(cert.z * nrm > np.abs(inp["d"]) / nrm)[0]


def _active_jacobian(inp, cert):
    act = _binding(inp, cert)
    Jc = inp["Jc"].toarray() if hasattr(inp["Jc"], "toarray") else np.asarray(inp["Jc"])
    Jd = inp["Jd"].toarray() if hasattr(inp["Jd"], "toarray") else np.asarray(inp["Jd"])
    return Jc, Jd, act


# ---------------------------------------------------------------------------------------------------------- accepts
def test_accepts_reference_points(case):
    cert, bounds, inp, prod = case.run(case.x)
    report(case.name, cert, bounds, prod)
    assert accepted(cert, bounds)
    assert len(_binding(inp, cert)) > 0                          # rows do bind at every one of these points
    if isinstance(case, NlpCase):
        # the reference points sit at least 10 x under the bound, and so does the Jacobians' own error
        assert cert.stat <= TOL * cert.s_d and cert.compl <= TOL * cert.s_c and prod <= TOL * cert.s_d


# ---------------------------------------------------------------------------------------------------------- rejects
def test_rejects_a_move_along_the_active_constraints(case, scale=1e-4):
    """1e-4 (in the scaled unknowns) along a null-space direction of the binding rows' Jacobian: feasible to first order,
    not stationary."""
    cert0, _, inp, _ = case.run(case.x)
    Jc, Jd, act = _active_jacobian(inp, cert0)
    Z = null_space(np.vstack([Jc, Jd[act]]))
    assert Z.shape[1] > 0
    # the direction of largest curvature of the Lagrangian in that null space: a move of 1e-4 there changes the gradient by
    # 1e-4 times that curvature, and nothing tangent to the binding rows can take it up
    if isinstance(case, QpCase):
        HZ = case.P @ Z
    else:
        def lagrangian_gradient(x):
            inp1 = case.nlp.certificate_inputs(x.reshape(case.nlp.N, case.nlp.nv))[0]
            return inp1["gf"] + inp1["Jc"].T @ cert0.y + inp1["Jd"].T @ cert0.z
        e = 1e-5
        HZ = np.stack([(lagrangian_gradient(case.x + e * z) - lagrangian_gradient(case.x - e * z)) / (2 * e) for z in Z.T], axis=1)
    R = Z.T @ HZ
    v = Z @ np.linalg.eigh(0.5 * (R + R.T))[1][:, -1]
    cert, bounds, _, prod = case.run(case.x + scale * v / np.abs(v).max())
    report(case.name + ", moved along the null space", cert, bounds, prod)
    assert cert.stat > bounds[0]


def test_rejects_a_binding_row_pushed_inside(case, push=1e-3):
    """The binding row with the largest multiplier moved 1e-3 inside, all other binding rows held to first order: its
    multiplier either stays (complementarity) or goes (stationarity)."""
    cert0, _, inp, _ = case.run(case.x)
    Jc, Jd, act = _active_jacobian(inp, cert0)
    J = np.vstack([Jc, Jd[act]])
    for i in act[np.argsort(-cert0.z[act])]:      # ... among those that a small move does push (a row that is nearly a
        rhs = np.zeros(len(J))                    # combination of other binding rows cannot be moved alone)
        rhs[len(Jc) + int(np.where(act == i)[0][0])] = -push
        step = np.linalg.lstsq(J, rhs, rcond=None)[0]
        if np.abs(step).max() <= 100 * push:
            break
    assert cert0.z[i] > 0 and np.abs(step).max() <= 100 * push
    cert, bounds, inp1, prod = case.run(case.x + step)
    report(case.name + f", row {i} (z = {cert0.z[i]:.2e}) pushed inside", cert, bounds, prod)
    assert inp1["d"][i] < -0.5 * push or push == 0.0
    assert cert.stat > bounds[0] or cert.compl > bounds[1]


def test_rejects_the_clipped_unconstrained_minimiser(twin_qp, clip=True):
    """The unconstrained minimiser of the QP, shrunk towards the centre line until every row is inside: feasible, and on
    Monza not optimal."""
    c = twin_qp
    a = -np.linalg.solve(c.P, c.q)
    if clip:
        Aa = c.A @ a
        a = a / max(1.0, (Aa / c.hi).max(), (Aa / c.lo).max()) * (1 - 1e-12)
    else:
        a = c.x
    cert, bounds, _, _ = c.run(a)
    report(c.name + ", clipped unconstrained minimiser", cert, bounds)
    assert cert.viol <= bounds[2]
    assert cert.stat > bounds[0] or cert.compl > bounds[1]


# --------------------------------------------------------------------------------------------------- self-consistency
def closed_form_qp():
    """min 1/2 x'Hx + q'x (H diagonal), x0 + x1 = 1, x2 <= 1 (binds), x3 <= 1 (does not), x4 >= 0 (binds), -1 <= x5 <= 1
    (upper binds), in rotated unknowns u = Q'x so that no Jacobian is sparse.  Separable, hence closed form."""
    H = np.array([2.0, 3.0, 1.5, 2.5, 1.0, 4.0]); q = np.array([-1.0, 0.5, -4.5, -1.0, 3.0, -7.0])
    y = -(1.0 + q[0] / H[0] + q[1] / H[1]) / (1.0 / H[0] + 1.0 / H[1])
    x = np.array([-(q[0] + y) / H[0], -(q[1] + y) / H[1], 1.0, -q[3] / H[3], 0.0, 1.0])
    Jd = np.zeros((5, 6)); Jd[0, 2] = 1; Jd[1, 3] = 1; Jd[2, 4] = -1; Jd[3, 5] = 1; Jd[4, 5] = -1
    d = np.array([x[2] - 1, x[3] - 1, -x[4], x[5] - 1, -1 - x[5]])
    z = np.array([-(H[2] + q[2]), 0.0, q[4], -(H[5] + q[5]), 0.0])
    Q = np.linalg.qr(np.random.default_rng(5).normal(size=(6, 6)))[0]
    Jc = np.zeros((1, 6)); Jc[0, :2] = 1.0
    return dict(gf=Q.T @ (H * x + q), Jc=Jc @ Q, c=np.array([x[0] + x[1] - 1.0]), Jd=Jd @ Q, d=d), y, z


@pytest.mark.parametrize("scipy_bvls", [False, True])
def test_closed_form_qp_multipliers(scipy_bvls):
    inp, y, z = closed_form_qp()
    assert z.min() >= 0 and (z[[0, 2, 3]] > 0).all()
    cert = kc.certify(**inp, scipy_bvls=scipy_bvls)
    assert abs(cert.y[0] - y) <= 1e-10 and np.abs(cert.z - z).max() <= 1e-10
    assert cert.stat <= 1e-12 and cert.compl <= 1e-12 and cert.viol <= 1e-15


def test_sparse_solver_agrees_with_lsq_linear(slsqp_oval16, twin_qp):
    """The module's own bounded least-squares solve against scipy.optimize.lsq_linear on the same problems, at an accepted
    point and at a rejected one (where the residual is not small and the bounds decide the multipliers)."""
    for case in (slsqp_oval16, twin_qp):
        for x in (case.x, case.x + 1e-3 * np.sin(np.arange(len(case.x)))):
            inp = case.run(x)[2]
            a, b = kc.certify(**inp), kc.certify(**inp, scipy_bvls=True)
            fa, fb = np.hypot(np.linalg.norm(a.r_stat), np.linalg.norm(a.r_compl)), np.hypot(np.linalg.norm(b.r_stat), np.linalg.norm(b.r_compl))
            print(f"[{case.name}] least-squares residual {fa:.6e} (sparse) {fb:.6e} (lsq_linear)")
            assert fa <= fb * (1 + 1e-6) + 1e-11               # the objective both minimise: the sparse solve is no worse
            assert abs(a.stat - b.stat) <= 1e-6 * b.stat + 1e-12 and abs(a.compl - b.compl) <= 1e-6 * b.compl + 1e-12


def test_jacobian_colouring_and_cost_gradient(twin_mgkt):
    """The coloured finite differences on an ODD ring (MGKT at 8 m: 103 nodes, three colours) against one-node-at-a-time
    differences, and the double-track cost gradient against the checker's cost (quadratic: a central difference is exact)."""
    nlp = twin_mgkt.nlp
    assert nlp.N % 2 == 1 and len(kc.node_colours(nlp.N)) == 3
    w = twin_mgkt.x.reshape(nlp.N, nlp.nv)
    Jo, Jn, Eo, En = nlp.jacobian_blocks(w)
    h = 1e-5
    for j, k in ((0, 4), (nlp.N - 1, 5), (nlp.N - 2, 0), (51, 8)):
        wp, wm = w.copy(), w.copy(); wp[j, k] += h; wm[j, k] -= h
        fp = np.concatenate(nlp.rows(wp[None]), axis=2)[0]; fm = np.concatenate(nlp.rows(wm[None]), axis=2)[0]
        fd = (fp - fm) / (2 * h)
        np.testing.assert_allclose(fd[j], Jo[j, :, k], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(fd[j - 1], Jn[j - 1, :, k], rtol=1e-5, atol=1e-6)
        fd[j] = 0.0; fd[j - 1] = 0.0
        assert np.abs(fd).max() == 0.0                       # a pair's rows see its own two nodes only
    v = np.random.default_rng(1).normal(size=w.shape)
    assert (nlp.cost(w + 0.5 * v) - nlp.cost(w - 0.5 * v)) == pytest.approx((nlp.cost_gradient(w) * v).sum(), rel=1e-10)


# ------------------------------------------------------------- the global QPs on the linearisation that they solved
def test_polish_finds_the_closed_form_optimum():
    """kkt_certificate.polish_qp on a QP whose optimum is known: min 1/2 |x - c|^2, -1 <= x <= 1 (the clipped c), started from a
    point with a wrong working set (one row too many, one missing)."""
    c = np.array([2.0, -3.0, 0.25, 0.999, -1.5, 0.0])
    P, q, A = np.eye(6), -c, np.eye(6)
    start = np.array([1.0, -1.0, 1.0, 0.0, 0.0, 0.0])            # row 2 does not bind at the optimum, row 4 does and is missing
    x, nwork, _ = kc.polish_qp(P, q, A, -np.ones(6), np.ones(6), start)
    assert np.abs(x - np.clip(c, -1.0, 1.0)).max() <= 1e-14 and nwork == 3


@pytest.mark.parametrize("c", gk.params())
def test_global_twin_output_is_a_kkt_point_of_its_own_linearisation(c):
    """Every case of tests/global_kkt_cases.py on the CPU twins (the RL_GLOBAL_V1 case selects a kernel: the twin is the same)."""
    r = gk.solve_case(gk.TwinSolver(), c)
    gk.assert_case(c, *r, gk.certify_case(c, *r, report))


def test_hook_off_is_the_twin_that_never_set_it():
    """A thread of its own has never called the setter (it is thread-local); the hook changes the (m-1)-result, switching it
    off again does not."""
    import threading
    c = gk.by_id(gk.OLD_PREMISE_CASE)
    inp, W, s = gk.inputs(c.track, c.N), gk.widths_of(c), gk.TwinSolver()
    fresh = {}
    th = threading.Thread(target=lambda: fresh.update(r=orc.global_mincurv(inp.t, inp.cx, inp.cy, inp.k, c.N, inp.wl, inp.wr,
                                                                         c.margin, c.n_outer - 1)))
    th.start(); th.join()
    on = s.one(inp, W, c.margin, c.n_outer - 1, True)
    off = s.one(inp, W, c.margin, c.n_outer - 1, False)
    assert off[0][0].tobytes() == fresh["r"][3].tobytes() and np.array_equal(off[1][0, :6], fresh["r"][4])
    d = np.abs(on[0] - off[0]).max()
    print(f"[{c.id}] hooked against unhooked (m-1)-result: {d:.2e} m, ipm {int(on[1][0, 0])} / {int(off[1][0, 0])}")
    assert d > 1e-5 and on[1][0, 0] < off[1][0, 0]       # why the old premise failed: another point, by far more than the bound
    zon = s.xy(inp, W, c.margin, gk.LON, 1, True); zoff = s.xy(inp, W, c.margin, gk.LON, 1, False)
    assert zon[1][0, 0] <= zoff[1][0, 0]                  # (1e-9 against 1e-10: mu may pass both in one iteration)
    import weighted_global_twin as tw
    w = gk.weights_of("speed", c.N)
    a_on = tw.global_mincurv_weighted(inp.t, inp.cx, inp.cy, inp.k, c.N, inp.wl, inp.wr, c.margin, 2, weights=w, last_as_mid=True)
    a_off = tw.global_mincurv_weighted(inp.t, inp.cx, inp.cy, inp.k, c.N, inp.wl, inp.wr, c.margin, 2, weights=w)
    assert a_on[4][0] < a_off[4][0]


@pytest.mark.parametrize("tag", ["one-kart_c-N400-m2.0-o2", gk.OLD_PREMISE_CASE])
def test_old_premise_is_rejected(tag):
    """a_m certified on qp_at(result of a plain (m-1)-call), the procedure before the hook: stationarity beyond the bound."""
    c = gk.by_id(tag)
    r = gk.solve_case_with(gk.TwinSolver(), c, hooked=False)
    f = gk.certify_case(c, *r, report)
    assert f[0].cert.stat > f[0].bounds[0]


@pytest.mark.parametrize("tag", sorted(k for k in gk.KNOWN_FAILURES if k.startswith("one")))
def test_last_threshold_1e12_would_certify(tag, monkeypatch):
    """The one-offset cases on the list of known failures, on the statement-for-statement numpy twin (unit weights where the
    case has none): rejected at the exit rule as it is, accepted with the last linearisation left at complementarity 1e-12 --
    the threshold that the kernels do not survive.  The failures are the exit rule's, not the certificate's."""
    import weighted_global_twin as tw
    c = gk.by_id(tag)
    monkeypatch.setitem(gk.WEIGHTS, "ones", lambda N: np.ones(N))
    c1 = gk.case(c.kind, c.track, c.N, c.margin, c.n_outer, weights=c.weights or "ones")
    r = gk.solve_case(gk.TwinSolver(), c1)
    f = gk.certify_case(c1, *r, report)[0]
    assert f.dist > gk.DIST
    if tag in gk.EXIT_RULE_CASES:
        assert f.cert.stat > f.bounds[0] or f.cert.compl > f.bounds[1]
    monkeypatch.setattr(tw, "IPM_TOL_LAST", 1e-12)
    r = gk.solve_case(gk.TwinSolver(), c1)
    gk.assert_case(c1, *r, gk.certify_case(c1, *r, report))
