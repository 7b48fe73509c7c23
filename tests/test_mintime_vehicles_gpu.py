"""rl_mintime_solve_vehicles[_dev]: one vehicle model per instance in the batched min-time solve, on the device.

The problem is MGKT at 8 m (N = 103), the vehicles those of tests/mintime_vehicle_cases.py.  The per-instance kernels evaluate
the same expressions in the same order as the shared-model ones on the same doubles (the host computes every instance's
scales with the shared entry's expressions), so wherever a vehicles call is compared with shared-model calls the comparison
is bit for bit (assert_array_equal) on X, U, T and all twelve stats columns.  Against the CPU twin the bounds are the
existing ones of tests/test_mintime.py: 1e-5 scaled deviation after 1 and 3 iterations (the twin's Hessian is a finite
difference), 1e-6 s on the converged lap time against the twin's constants of the case file.

Measured on the MI355X (first run, 11 tests in 8.7 s): every bit-for-bit comparison holds; against the twin 7.7e-9 / 8.1e-9
(mass, mu) after one iteration and 4.5e-7 / 4.1e-8 after three; converged laps within 2.7e-10 s of the twin's constants
(iterations 52 / 65 / 43 / 50 / 51, the twin's 53 / 64 / 44 / 51 / 52); certificates: stationarity <= 5.2e-8, complementarity
<= 1.9e-7, violation <= 1.9e-8; the tables' lap time against the solver's 4.4e-16 relative.  The chain starts from the
reference's guess (controls (1, -1, 0.001, 0), times unshifted) and ends, for the modified vehicles, in other local optima
than the guess of the case file does (laps 49.189 / 47.856 / 48.618 / 47.540 s there): compare like with like."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mintime_vehicle_cases as vc
from mintime_problem import width_scales
from oracle import sqp_twin as tw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("X", "U", "T", "st")
SOLVER = dict(average_track_width=vc.defaults.SOLVER["average_track_width"], speed_cap=vc.defaults.SOLVER["speed_cap"])
IT12 = dict(max_iter=12, tol=1e-12, **SOLVER)
B13 = 13   # the smallest batch that forks three sub-batches (4, 4 and 5 instances)


@pytest.fixture(scope="module")
def ops():
    from spline_trajectory_optimization_amd import _lib, ops
    _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing
    return ops


@pytest.fixture(scope="module")
def prob():
    d, X0, U0, T0 = vc.problem()
    assert len(d["s"]) == 103
    return d, X0, U0, T0


def _args(d, left=None, right=None, margin=None):
    return (d["s"], d["kappa"], d["left"] if left is None else left, d["right"] if right is None else right,
            vc.margin(vc.defaults.MODEL) if margin is None else margin, d["L"])


def _guess(prob, B):
    _, X0, U0, T0 = prob
    return vc.rep(X0, B), vc.rep(U0, B), vc.rep(T0, B)


def _cycled(B):
    return [vc.NAMES[b % len(vc.NAMES)] for b in range(B)]


def _equal(a, b, what=""):
    for k, x, y in zip(KEYS, a, b):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {k}")


@pytest.fixture(scope="module")
def singles12(ops, prob):
    """Twelve iterations of every vehicle as a shared-model call with B = 1: name -> (X, U, T, st), each [1, ...]."""
    d = prob[0]
    return {n: ops.mintime_solve_batch(vc.model(n), *_args(d), *_guess(prob, 1), **IT12) for n in vc.NAMES}


def test_equal_rows_are_the_shared_model_call_bit_for_bit(ops, prob):
    """Thirteen copies of MODEL through the vehicles entry against the shared-model entry on the same batch (three
    sub-batches, per-instance widths): X, U, T and all twelve stats columns."""
    d = prob[0]
    sc = width_scales(B13)
    left, right = d["left"][None] * sc[:, None], d["right"][None] * sc[:, None]
    shared = ops.mintime_solve_batch(vc.defaults.MODEL, *_args(d, left, right), *_guess(prob, B13), **IT12)
    veh = ops.mintime_solve_vehicles([dict(vc.defaults.MODEL)] * B13, *_args(d, left, right), *_guess(prob, B13), **IT12)
    assert (shared[3][:, 0] == 12.0).all() and np.isfinite(shared[0]).all()
    _equal(veh, shared, "vehicles entry with equal rows")
    # and on shared widths (left / right [N])
    _equal(ops.mintime_solve_vehicles([dict(vc.defaults.MODEL)] * B13, *_args(d), *_guess(prob, B13), **IT12),
           ops.mintime_solve_batch(vc.defaults.MODEL, *_args(d), *_guess(prob, B13), **IT12), "shared widths")


def test_each_instance_is_its_single_call_bit_for_bit(ops, prob, singles12):
    d = prob[0]
    names = _cycled(B13)
    res = ops.mintime_solve_vehicles(vc.models(names), *_args(d), *_guess(prob, B13), **IT12)
    assert (res[3][:, 0] == 12.0).all()
    for b, n in enumerate(names):
        _equal([a[b] for a in res], [a[0] for a in singles12[n]], f"instance {b} ({n})")
    # the vehicles do differ: every modified one has left the base iterate
    for n in vc.NAMES[1:]:
        assert np.abs(singles12[n][0] - singles12["base"][0]).max() > 1e-6, n
    # reordering the rows reorders the results
    perm = np.random.default_rng(7).permutation(B13)
    assert (perm != np.arange(B13)).any()
    res_p = ops.mintime_solve_vehicles(vc.models([names[p] for p in perm]), *_args(d), *_guess(prob, B13), **IT12)
    _equal(res_p, [a[perm] for a in res], "permuted rows")


def test_each_instance_is_its_single_call_with_per_instance_widths(ops, prob):
    d = prob[0]
    names = _cycled(B13)
    sc = width_scales(B13)
    left, right = d["left"][None] * sc[:, None], d["right"][None] * sc[:, None]
    res = ops.mintime_solve_vehicles(vc.models(names), *_args(d, left, right), *_guess(prob, B13), **IT12)
    for b, n in enumerate(names):
        one = ops.mintime_solve_batch(vc.model(n), *_args(d, left[b], right[b]), *_guess(prob, 1), **IT12)
        _equal([a[b] for a in res], [a[0] for a in one], f"instance {b} ({n}, width x {sc[b]:.3f})")


@pytest.mark.parametrize("iters", [1, 3])
def test_vehicles_against_the_twin(ops, prob, iters):
    """The two vehicles whose change reaches the SCALES (mass) and the tyre rows (mu), one and three iterations against the
    twin's same iteration; bound and scaling of test_mintime_solve_vs_twin."""
    d = prob[0]
    names = ["mass x 1.1", "mu x 0.9"]
    X, U, T, st = ops.mintime_solve_vehicles(vc.models(names), *_args(d), *_guess(prob, 2), max_iter=iters, tol=1e-12, **SOLVER)
    for b, n in enumerate(names):
        P, w0 = vc.twin_start(d, vc.model(n))
        w, info = tw.solve(P, w0, max_iter=iters, tol=1e-12)
        Xt, Ut, Tt = P.unpack(w)
        dev = max(np.abs((X[b] - Xt) / P.scale_x).max(), np.abs((U[b] - Ut) / P.scale_u).max(), np.abs(T[b] - Tt).max())
        print(f"{n}, after {iters} iteration(s): max scaled deviation from the twin {dev:.2e}")
        assert dev <= 1e-5, (n, iters, dev)


def test_converged_batch_of_five_vehicles(ops, prob):
    import kkt_certificate as kc
    from test_optimality_gpu import _check_nlp
    d = prob[0]
    X, U, T, st = ops.mintime_solve_vehicles(vc.models(), *_args(d), *_guess(prob, 5), max_iter=200, tol=1e-6, **SOLVER)
    lap = dict(zip(vc.NAMES, st[:, 4]))
    for b, n in enumerate(vc.NAMES):
        print(f"{n}: iterations {st[b, 0]:.0f} (twin {vc.TWIN_ITERATIONS[n]}), lap {st[b, 4]:.6f} s (twin {vc.TWIN_LAP[n]:.6f}), "
              f"difference {st[b, 4] - vc.TWIN_LAP[n]:+.2e} s, status {st[b, 5]:.0f}")
    assert (st[:, 5] == 1.0).all(), st[:, 5]
    for b, n in enumerate(vc.NAMES):
        assert abs(st[b, 4] - vc.TWIN_LAP[n]) <= 1e-6, (n, st[b, 4], vc.TWIN_LAP[n])
    for b, n in enumerate(vc.NAMES):   # every result is a first-order optimum of ITS vehicle's problem, by the pinned functions
        nlp = kc.DoubleTrackNLP(vc.model(n), d["s"], d["kappa"], d["left"], d["right"], d["L"], SOLVER["average_track_width"],
                                SOLVER["speed_cap"])
        _check_nlp(f"vehicles batch row {b} ({n})", nlp, nlp.to_w(X[b], U[b], T[b]), st[b])
    for n in ("mu x 0.9", "Pmax x 0.8", "mass x 1.1"):   # the twin's ordering
        assert lap[n] >= lap["base"], (n, lap)


def test_two_front_kernel_selected_by_the_switch(tmp_path):
    """RL_MT_KKT4=0 (test_four_front_vs_two_front_elimination's switch, read when the context is created: a process of its own)
    at 8 m: the vehicles entry with two different models equals the two single calls after twelve iterations."""
    f = str(tmp_path / "k2.npz")
    subprocess.run([sys.executable, os.path.join(HERE, "mintime_vehicles_run.py"), f, "12", "8.0", "mass x 1.1", "Fd_max x 0.9"],
                   check=True, env=dict(os.environ, RL_MT_KKT4="0"), timeout=300)
    r = np.load(f)
    assert r["X"].shape[1] >= 64 and (r["st"][:, 0] == 12.0).all()
    for b in range(2):
        for k in KEYS:
            np.testing.assert_array_equal(r[k][b], r[f"{k}{b}"], err_msg=f"instance {b} {k}")
    assert np.abs(r["X"][0] - r["X"][1]).max() > 1e-6


def test_short_lap_takes_the_two_front_kernel_by_itself(ops):
    """Fewer than 64 nodes (MGKT at 22 m): k_mt_kkt without any switch, and a node count that leaves tails in every grid."""
    d, X0, U0, T0 = vc.problem(22.0)
    N = len(d["s"])
    assert 8 <= N < 64
    names = ["mu x 0.9", "mass x 1.1"]
    g = lambda B: (vc.rep(X0, B), vc.rep(U0, B), vc.rep(T0, B))  # noqa: E731
    res = ops.mintime_solve_vehicles(vc.models(names), *_args(d), *g(2), **IT12)
    for b, n in enumerate(names):
        _equal([a[b] for a in res], [a[0] for a in ops.mintime_solve_batch(vc.model(n), *_args(d), *g(1), **IT12)], n)


def test_host_entry_equals_the_device_entry_on_a_forked_batch(ops, prob):
    import torch
    d = prob[0]
    names = _cycled(B13)
    sc = width_scales(B13)
    left, right = d["left"][None] * sc[:, None], d["right"][None] * sc[:, None]
    kw = dict(max_iter=200, tol=1e-6, **SOLVER)
    Xh, Uh, Th, sth = ops.mintime_solve_vehicles(vc.models(names), *_args(d, left, right), *_guess(prob, B13), **kw)
    dev = torch.device("cuda", 0)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    X, U, T = (g(a) for a in _guess(prob, B13))
    a = _args(d, left, right)
    st = ops.mintime_solve_vehicles_torch(vc.models(names), g(a[0]), g(a[1]), g(a[2]), g(a[3]), a[4], a[5], X, U, T, **kw)
    torch.cuda.synchronize()
    print("host / device entry: iterations", sth[:, 0], st.cpu().numpy()[:, 0])
    assert (sth[:, 5] == 1.0).all() and sth[:, 0].max() < 200
    _equal((X.cpu().numpy(), U.cpu().numpy(), T.cpu().numpy(), st.cpu().numpy()), (Xh, Uh, Th, sth), "device entry")


def _race_track():
    from mintime_problem import _load
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    est = vc.defaults.ESTIMATES
    veh = Vehicle(VehicleParams(np.array(est["acc_speed_loopup"]), np.array(est["dcc_speed_lookup"]), est["max_lon_acc_mpss"],
                                est["max_lon_dcc_mpss"], est["max_left_acc_mpss"], est["max_right_acc_mpss"],
                                est["max_speed_mps"], est["max_jerk_mpsc"]))
    rt = RaceTrack("MGKT", _load("MGKT_OUT_BOUND_enu.csv"), _load("MGKT_IN_BOUND_enu.csv"), _load("MGKT_CENTER_enu.csv"),
                   s=1.0, interval=8.0)
    return rt, veh


def test_the_chain_with_one_model_per_instance(ops):
    """optimise_track_batch(models=five): the tables' lap time is the solver's (the bound of the existing chain test), every
    X[b] is that of the single-vehicle chain, and B QSS vehicles that are all the shared one change nothing."""
    import torch
    from spline_trajectory_optimization_amd.min_time_optm.min_time_optimizer import optimise_track_batch
    rt, veh = _race_track()
    kw = dict(max_iter=200, tol=1e-6, **SOLVER)
    ms = vc.models()
    res = optimise_track_batch(rt, veh, None, models=ms, **kw)
    trk = res["track"]
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "track"}
    assert out["X"].shape[0] == 5 and (out["stats"][:, 5] == 1.0).all()
    rel = np.abs(out["summary"][:, 0] / out["stats"][:, 4] - 1.0).max()
    print(f"[vehicles chain] lap time of the tables against the solver's: {rel:.2e} relative; laps {out['stats'][:, 4]}")
    assert rel <= 1e-12
    for b, m in enumerate(ms):
        one = optimise_track_batch(rt, veh, m, track=trk, **kw)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out["X"][b], one["X"].cpu().numpy()[0], err_msg=vc.NAMES[b])
    same = optimise_track_batch(rt, None, None, models=ms, vehicles=[veh] * 5, track=trk, **kw)
    torch.cuda.synchronize()
    for k in ("X", "U", "T", "stats", "points", "summary"):
        np.testing.assert_array_equal(same[k].cpu().numpy(), out[k], err_msg=k)
    # vehicles of different widths: each margin folded into the distances the solver sees
    wide = [dict(ms[0]), dict(ms[0], vehicle_width=ms[0]["vehicle_width"] * 1.5)]
    res2 = optimise_track_batch(rt, veh, None, models=wide, track=trk, **kw)
    one = optimise_track_batch(rt, veh, wide[1], track=trk, **kw)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(res2["X"].cpu().numpy()[0], out["X"][0])
    np.testing.assert_array_equal(res2["X"].cpu().numpy()[1], one["X"].cpu().numpy()[0])


def test_a_bad_model_row_is_refused_and_nothing_runs(ops, prob):
    from spline_trajectory_optimization_amd import _lib
    d = prob[0]
    ctx = _lib.Context.get(0)
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    for key, value, what in (("mass", 0.0, "mass"), ("Pmax", float("nan"), "not finite")):
        tab = ops.dt_models_table(vc.models())
        tab[3, ops.DT_PARAMS.index(key)] = value
        X, U, T = (np.ascontiguousarray(a) for a in _guess(prob, 5))
        X_in, st = X.copy(), np.full((5, 12), -7.0)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in _args(d)[:4]]
        rc = ctx.lib.rl_mintime_solve_vehicles(ctx.h, p(tab), 5, len(d["s"]), p(a[0]), p(a[1]), p(a[2]), p(a[3]), 0,
                                               vc.margin(vc.defaults.MODEL), float(d["L"]), SOLVER["average_track_width"],
                                               SOLVER["speed_cap"], p(X), p(U), p(T), 12, 1e-12, p(st))
        msg = ctx.lib.rl_last_error().decode()
        print(f"{key} = {value}: rc {rc}, '{msg}'")
        assert rc == -1                                                          # RL_ERR_ARG
        assert "instance 3" in msg and what in msg
        np.testing.assert_array_equal(X, X_in)
        assert (st == -7.0).all()                                               # nothing ran, nothing came back
        with pytest.raises(ValueError, match="instance 3"):
            ops.mintime_solve_vehicles(tab, *_args(d), *_guess(prob, 5), **IT12)
