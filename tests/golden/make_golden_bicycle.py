#!/usr/bin/env python3
"""Generate tests/golden/G13_bicycle_nlp.npz by IMPORTING the reference's own bicycle NLP code
(models/dynamic_bicycle.py, utils/utils.py, utils/integrator.py, min_time_optm/min_time_optimizer.py:14-90) from
/root/reference (read-only), evaluated on numbers through make_golden's numeric casadi stand-in (G8).

The stand-in needs four more pieces for this code, patched in-process here (make_golden.py stays as it is):
matrix product (`@`, utils.py:7), `ca.tan` (dynamic_bicycle.py:17), `ca.norm_2` (:67 and min_time_optimizer.py:66-67),
and casadi's orientation rule for slicing a vector with one index range (`scale_x[0:2]` on a 1 x 5 row is 1 x 2).
Runs only where /root/reference exists; what it writes is numbers only.

usage:  python tests/golden/make_golden_bicycle.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import M, FakeOpti  # noqa: E402

MODEL = {"lr": 1.5, "L": 3.0, "delta_max": 0.314158999998341, "v_max": 80.0, "a_lon_max": 20.0, "a_lon_min": -20.0,
         "delta_dot_max": 1.0, "acc_max": 20.0}     # tests/test_min_time_optm.py:69-78


def patch_stand_in(ca):
    M.__matmul__ = lambda self, o: M(self.a @ M._v(o))
    M.__rmatmul__ = lambda self, o: M(M._v(o) @ self.a)
    ca.tan = lambda x: M(np.tan(M._v(x)))
    ca.norm_2 = lambda x: M(np.sqrt(np.sum(M._v(x) ** 2)))
    ca.DM = ca.DMnum            # numeric DM throughout (no QP solver is stood in for here)
    get = M.__getitem__

    def getitem(self, key):      # a single slice on a row vector slices its columns (casadi's orientation rule)
        if isinstance(key, slice) and self.a.shape[0] == 1:
            return M(self.a[:, key])
        return get(self, key)
    M.__getitem__ = getitem


def run_nlp(ca, ref_mt, dyn, traj_d, Xs, Us, Ts):
    """All constraint residuals and the cost of set_up_bicycle_problem at the scaled point (Xs, Us, Ts)."""
    N = len(traj_d)
    holder = {}
    real_Opti = ca.Opti

    def make_opti(*a):
        o = FakeOpti()
        o.values = [Xs, Us, Ts]
        holder["o"] = o
        return o
    ca.Opti = make_opti
    params = {"N": N, "traj_d": traj_d, "nu": dyn.nu(), "nx": dyn.nx(), "model": MODEL, "dynamics": dyn.dynamics,
              "x_l": dyn.x_l, "x_u": dyn.x_u, "u_l": dyn.u_l, "u_u": dyn.u_u, "verbose": False, "max_iter": 1, "tol": 0.1}
    try:
        ref_mt.set_up_bicycle_problem(params)
    finally:
        ca.Opti = real_Opti
    o = holder["o"]
    per = len(o.cons) // N
    assert per * N == len(o.cons) and per == 7, (len(o.cons), N)
    out = {k: np.zeros((N,) + s) for k, s in (("defect", (5,)), ("lon", ()), ("lat_lo", ()), ("lat_hi", ()),
                                               ("trac", ()), ("x_lo", (5,)), ("x_hi", (5,)), ("u_lo", (2,)),
                                               ("u_hi", (2,)), ("t_le", ()))}
    for i in range(N):
        c = o.cons[i * per:(i + 1) * per]
        assert [r[0] for r in c] == ["eq", "eq", "bounded", "le", "bounded", "bounded", "le"], [r[0] for r in c]
        j = (i - 1) % N
        out["defect"][j] = c[0][1].a.reshape(-1)
        out["lon"][j] = float(c[1][1])
        out["lat_lo"][j], out["lat_hi"][j] = float(c[2][1]), float(c[2][2])
        out["trac"][j] = float(c[3][1])
        out["x_lo"][j], out["x_hi"][j] = c[4][1].a.reshape(-1), c[4][2].a.reshape(-1)
        out["u_lo"][j], out["u_hi"][j] = c[5][1].a.reshape(-1), c[5][2].a.reshape(-1)
        out["t_le"][j] = float(c[6][1])
    out["cost"] = np.float64(float(o.cost))
    return out


def random_point(rng, N):
    Xs = np.column_stack([rng.uniform(-0.3, 0.3, N), rng.uniform(-0.3, 0.3, N), rng.uniform(-1.5, 1.5, N),
                          rng.uniform(-3, 3, N), rng.uniform(0.05, 0.9, N)])
    Us = np.column_stack([rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)])
    return Xs, Us, rng.uniform(0.05, 0.8, N)


def main():
    if not os.path.isdir(mg.REF):
        sys.exit("reference not present; fixtures are generated in the build container only")
    mg.install_shims()
    import casadi as ca
    patch_stand_in(ca)
    from spline_traj_optm.models.trajectory import BSplineTrajectory
    import spline_traj_optm.models.dynamic_bicycle as dyn
    import spline_traj_optm.utils.utils as ut
    import spline_traj_optm.utils.integrator as integ
    import spline_traj_optm.min_time_optm.min_time_optimizer as ref_mt
    rng = np.random.default_rng(13)
    kw = {"model_keys": np.array(list(MODEL)), "model_vals": np.array([MODEL[k] for k in MODEL])}
    # (a) dynamics, lat_acc at random states and controls
    S = 64
    Xr = np.column_stack([rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(-4, 4, S),
                          rng.uniform(-0.3, 0.3, S), rng.uniform(0, 80, S)])
    Ur = np.column_stack([rng.uniform(-20, 20, S), rng.uniform(-1, 1, S)])
    kw["dyn_X"], kw["dyn_U"] = Xr, Ur
    kw["dyn_xdot"] = np.array([dyn.dynamics(MODEL, M(Xr[q].reshape(1, 5)).T, M(Ur[q].reshape(1, 2)).T).a.reshape(-1)
                               for q in range(S)])
    kw["dyn_lat_acc"] = np.array([float(dyn.lat_acc(MODEL, M(Xr[q].reshape(5, 1)), M(Ur[q].reshape(2, 1)))) for q in range(S)])
    # (b) rk4 defects, headings of the end point shifted by about +-2 pi on some pairs
    X2 = Xr + rng.normal(size=Xr.shape) * [1, 1, 0.1, 0.02, 1]
    X2[::3, 2] += 2 * np.pi; X2[1::3, 2] -= 2 * np.pi
    dt = rng.uniform(0.05, 0.5, S)
    kw["rk4_X1"], kw["rk4_X2"], kw["rk4_U"], kw["rk4_dt"] = Xr, X2, Ur, dt
    kw["rk4_defect"] = np.array([integ.rk4(MODEL, dyn.dynamics, M(Xr[q].reshape(1, 5)), M(X2[q].reshape(1, 5)),
                                           M(Ur[q].reshape(1, 2)), dt[q]).a.reshape(-1) for q in range(S)])
    # (c) utils
    P = rng.normal(size=(S, 2)) * 20; yaw = rng.uniform(-7, 7, S)
    kw["g2f_p"], kw["g2f_yaw"] = P, yaw
    kw["g2f_out"] = np.array([(ut.global_to_frenet(M(P[q].reshape(2, 1)), M(np.zeros((2, 1))), yaw[q])).a.reshape(-1)
                              for q in range(S)])
    y1, y2 = rng.uniform(-10, 10, S), rng.uniform(-4, 4, S)
    kw["ay_y1"], kw["ay_y2"] = y1, y2
    kw["ay_out"] = np.array([float(ut.align_yaw(M(y1[q]), M(y2[q]))) for q in range(S)])
    s1, s2 = rng.uniform(0, 500, S), rng.uniform(0, 500, S)
    kw["aa_s1"], kw["aa_s2"], kw["aa_L"] = s1, s2, np.float64(500.0)
    kw["aa_out"] = np.array([float(ut.align_abscissa(M(s1[q]), M(s2[q]), 500.0)) for q in range(S)])
    # (d) the whole NLP at one random point on a synthetic closed track (oval, N = 48)
    N = 48
    ang = np.arange(N) * 2 * np.pi / N
    traj = np.zeros((N, 19))
    traj[:, 0], traj[:, 1] = 120 * np.cos(ang), 60 * np.sin(ang)
    tx, ty = -120 * np.sin(ang), 60 * np.cos(ang)
    traj[:, 3] = np.arctan2(ty, tx)
    nrm = np.hypot(tx, ty); nx_, ny_ = -ty / nrm, tx / nrm
    wl, wr = 5 + np.cos(2 * ang), 4.5 + 0.5 * np.sin(3 * ang)
    traj[:, 9], traj[:, 10] = traj[:, 0] + wl * nx_, traj[:, 1] + wl * ny_
    traj[:, 11], traj[:, 12] = traj[:, 0] - wr * nx_, traj[:, 1] - wr * ny_
    Xs, Us, Ts = random_point(rng, N)
    for k, v in run_nlp(ca, ref_mt, dyn, traj, Xs, Us, Ts).items():
        kw[f"oval_{k}"] = v
    kw["oval_traj"], kw["oval_Xs"], kw["oval_Us"], kw["oval_Ts"] = traj, Xs, Us, Ts
    # (e) the same on Monza at the reference test's 5 m (bspline s = 3.0, k = 5; FakeTrack's boundaries)
    centre = mg.load_xy("MONZA_UNOPTIMIZED_LINE_enu.csv")
    track = mg.FakeTrack(BSplineTrajectory, mg.load_xy("MONZA_LEFT_BOUNDARY_enu.csv"), mg.load_xy("MONZA_RIGHT_BOUNDARY_enu.csv"))
    traj_d = BSplineTrajectory(centre, 3.0, 5).sample_along(5.0)
    track.fill_trajectory_boundaries(traj_d)
    pts = np.array(traj_d.points)
    Xs, Us, Ts = random_point(rng, len(pts))
    for k, v in run_nlp(ca, ref_mt, dyn, pts, Xs, Us, Ts).items():
        kw[f"monza_{k}"] = v
    kw["monza_traj"], kw["monza_Xs"], kw["monza_Us"], kw["monza_Ts"] = pts, Xs, Us, Ts
    path = os.path.join(HERE, "G13_bicycle_nlp.npz")
    np.savez_compressed(path, **kw)
    print(f"wrote G13_bicycle_nlp.npz: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
