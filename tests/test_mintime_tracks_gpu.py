"""rl_mintime_solve_tracks[_dev]: one centre line per instance in the batched min-time solve, on the device.

The tracks are those of tests/mintime_track_cases.py (base, mirrored, scaled by 1.25, an oval; N = 103), the vehicles those of
tests/mintime_vehicle_cases.py.  The <MtProblemT> kernels evaluate the same expressions in the same order as the other two
forms on the same doubles (the host fills every instance's row with the shared entries' function), so wherever a tracks call
is compared with calls of the existing entries the comparison is bit for bit (assert_array_equal) on X, U, T and all twelve
stats columns.  Against the CPU twin the bounds are those of tests/test_mintime.py: 1e-5 scaled deviation after 1 and 3
iterations (the twin's Hessian is a finite difference), 1e-6 s on the converged lap time against the twin's constants of the
case file.

Measured on the MI355X (first run, 11 tests in 9.9 s; profiles/mintime_tracks/test_mintime_tracks_gpu.log): every bit-for-bit
comparison holds; against the twin 7.9e-9 .. 3.0e-8 after one iteration and 4.1e-8 .. 2.3e-6 (the oval) after three; converged laps
within 9.3e-11 s of the twin's constants (iterations 52 / 65 / 52 / 69 / 30 / 33 / 20 / 30, the twin's 53 / 64 / 53 / 67 / 31 / 31 /
21 / 31); certificates: stationarity <= 4.9e-8, complementarity <= 1.9e-7, violation <= 2.0e-7; the base vehicle laps MGKT in
47.62019670555031 s and its mirror image in 47.620196705544984 s; the chain's tables against optimise_track_batch per track: equal."""
import ctypes

import numpy as np
import pytest

import mintime_track_cases as tc
import mintime_vehicle_cases as vc
from mintime_problem import width_scales
from oracle import sqp_twin as tw

pytestmark = pytest.mark.gpu
KEYS = ("X", "U", "T", "st")
B13 = 13   # the smallest batch that forks three sub-batches (4, 4 and 5 instances)
MARGIN = vc.margin(vc.defaults.MODEL)


@pytest.fixture(scope="module")
def ops():
    from spline_trajectory_optimization_amd import _lib, ops
    _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing
    return ops


def _equal(a, b, what=""):
    for k, x, y in zip(KEYS, a, b):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {k}")


class Batch:
    """A mixed batch: instance b = vehicle vehicles[b] on track tracks[track_of[b]] with its width factor; the call's arrays."""

    def __init__(self, tracks, track_of, vehicles, widths=None, n=tc.N):
        self.tracks, self.track_of, self.vehicles, self.n = list(tracks), np.asarray(track_of, dtype=np.int64), list(vehicles), n
        self.B = len(self.track_of)
        self.widths = np.ones(self.B) if widths is None else widths
        self.d = [tc.track(t, n) for t in self.tracks]
        self.s, self.kappa, self.L, self.atw, self.cap = tc.stacked(self.tracks, n)
        of = self.track_of
        self.left = np.stack([self.d[t]["left"] * w for t, w in zip(of, self.widths)])
        self.right = np.stack([self.d[t]["right"] * w for t, w in zip(of, self.widths)])
        g = [tc.guess(d) for d in self.d]
        self.X0, self.U0, self.T0 = (np.stack([g[t][i] for t in of]) for i in range(3))

    def solve(self, ops, track_of="own", order=None, **kw):
        """The one call; order: a permutation of the instances (rows, widths, guesses and track_of together)."""
        o = np.arange(self.B) if order is None else order
        of = self.track_of[o] if isinstance(track_of, str) else track_of
        return ops.mintime_solve_tracks(vc.models([self.vehicles[b] for b in o]), of, self.s, self.kappa, self.left[o], self.right[o],
                                        MARGIN, self.L, self.X0[o], self.U0[o], self.T0[o], self.atw, self.cap, **kw)

    def single(self, ops, b, **kw):
        """Instance b as its own call of the vehicles entry with B = 1 on its track's data."""
        t = self.track_of[b]
        d = self.d[t]
        return ops.mintime_solve_vehicles(vc.models([self.vehicles[b]]), d["s"], d["kappa"], self.left[b], self.right[b], MARGIN, d["L"],
                                          self.X0[b][None], self.U0[b][None], self.T0[b][None], d["atw"], d["cap"], **kw)


IT12 = dict(max_iter=12, tol=1e-12)


def _mixed():
    """4 tracks x 5 vehicles = 20 instances, permuted so that neighbours and the sub-batch boundaries (6 | 7 | 7) mix tracks."""
    perm = np.random.default_rng(3).permutation(20)
    track_of, veh = perm // 5, [vc.NAMES[p % 5] for p in perm]
    assert (np.diff(track_of) != 0).sum() >= 10 and track_of[5] != track_of[6] and track_of[12] != track_of[13]
    return Batch(tc.TRACKS, track_of, veh, width_scales(20))


@pytest.fixture(scope="module")
def mixed12(ops):
    """The mixed batch after twelve iterations, and every instance as its own single call: computed once, read by three tests."""
    bt = _mixed()
    res = bt.solve(ops, **IT12)
    singles = [bt.single(ops, b, **IT12) for b in range(bt.B)]
    for a in res:
        a.setflags(write=False)
    return bt, res, singles


def test_one_track_is_the_shared_model_call_and_the_vehicles_call_bit_for_bit(ops):
    """T = 1, track_of = 0 (B = 13: all three sub-batches, per-instance widths): equal model rows return the bits of
    rl_mintime_solve_batch, one model for all does too, thirteen different rows those of rl_mintime_solve_vehicles."""
    d = tc.track("base")
    sc = width_scales(B13)
    names = [vc.NAMES[b % 5] for b in range(B13)]
    bt = Batch(["base"], np.zeros(B13, dtype=int), ["base"] * B13, sc)
    args = (d["s"], d["kappa"], bt.left, bt.right, MARGIN, d["L"], bt.X0, bt.U0, bt.T0, d["atw"], d["cap"])
    shared = ops.mintime_solve_batch(vc.defaults.MODEL, *args, **IT12)
    assert (shared[3][:, 0] == 12.0).all() and np.isfinite(shared[0]).all()
    _equal(bt.solve(ops, **IT12), shared, "equal rows")
    one = ops.mintime_solve_tracks(vc.defaults.MODEL, bt.track_of, bt.s, bt.kappa, bt.left, bt.right, MARGIN, bt.L, bt.X0, bt.U0, bt.T0,
                                   bt.atw, bt.cap, **IT12)
    _equal(one, shared, "one model row for all")
    bt.vehicles = names
    _equal(bt.solve(ops, **IT12), ops.mintime_solve_vehicles(vc.models(names), *args, **IT12), "thirteen vehicles")


def test_every_instance_of_a_mixed_batch_is_its_own_single_call_bit_for_bit(mixed12):
    bt, res, singles = mixed12
    assert (res[3][:, 0] == 12.0).all() and np.isfinite(res[0]).all()
    for b in range(bt.B):
        _equal([a[b] for a in res], [a[0] for a in singles[b]],
               f"instance {b} ({bt.vehicles[b]} on {bt.tracks[bt.track_of[b]]}, width x {bt.widths[b]:.3f})")
    # the tracks do differ: the same vehicle on two tracks has two iterates
    for t in range(1, 4):
        a = next(b for b in range(bt.B) if bt.track_of[b] == 0 and bt.vehicles[b] == "base")
        c = next(b for b in range(bt.B) if bt.track_of[b] == t and bt.vehicles[b] == "base")
        for i in (0, 1, 2):   # X (its column 0 is s itself), U, T
            assert np.abs(res[i][a] - res[i][c]).max() > 1e-6, (bt.tracks[t], KEYS[i])


def test_a_permutation_of_the_instances_permutes_the_results(ops, mixed12):
    bt, res, _ = mixed12
    perm = np.random.default_rng(7).permutation(bt.B)
    assert (perm != np.arange(bt.B)).any() and (bt.track_of[perm] != bt.track_of).any()
    _equal(bt.solve(ops, order=perm, **IT12), [a[perm] for a in res], "permuted track_of and rows")


def test_null_track_of_is_the_identity(ops):
    names = ["mass x 1.1", "base", "mu x 0.9", "Pmax x 0.8"]
    bt = Batch(tc.TRACKS, np.arange(4), names)
    explicit = bt.solve(ops, **IT12)
    _equal(bt.solve(ops, track_of=None, **IT12), explicit, "track_of = None")
    for b in range(4):
        _equal([a[b] for a in explicit], [a[0] for a in bt.single(ops, b, **IT12)], f"instance {b}")


def _wrap_crossers(d, X):
    """Nodes of the pairs whose abscissa difference the wrap rule folds by one track_length: the closing pair."""
    return int(np.sum(np.abs(np.diff(np.r_[X[:, 0], X[0, 0]])) > d["L"] / 2.0))


@pytest.mark.parametrize("iters", [1, 3])
def test_tracks_against_the_twin(ops, iters):
    """One instance on every track (and a second on the scaled one, whose closing pair crosses the wrap node with ITS
    track_length -- a length taken from another track would show in the last node's defect), after one and three iterations
    against the twin's same iteration, called once per instance with that instance's s, kappa and L."""
    names = ["mu x 0.9", "mass x 1.1", "base", "Pmax x 0.8", "mass x 1.1"]
    bt = Batch(tc.TRACKS, [0, 1, 2, 3, 2], names)
    X, U, T, st = bt.solve(ops, max_iter=iters, tol=1e-12)
    assert _wrap_crossers(bt.d[2], X[2]) == 1 and abs(bt.d[2]["L"] - tc.track("base")["L"]) > 100.0
    for b, n in enumerate(names):
        d = bt.d[bt.track_of[b]]
        P, w0 = tc.twin_start(d, vc.model(n))
        w, info = tw.solve(P, w0, max_iter=iters, tol=1e-12)
        Xt, Ut, Tt = P.unpack(w)
        dev = max(np.abs((X[b] - Xt) / P.scale_x).max(), np.abs((U[b] - Ut) / P.scale_u).max(), np.abs(T[b] - Tt).max())
        last = max(np.abs((X[b, -1] - Xt[-1]) / P.scale_x).max(), abs(T[b, -1] - Tt[-1]))
        print(f"{n} on {bt.tracks[bt.track_of[b]]}, after {iters} iteration(s): max scaled deviation from the twin {dev:.2e} "
              f"(last node, whose pair wraps: {last:.2e})")
        assert dev <= 1e-5, (n, bt.tracks[bt.track_of[b]], iters, dev)


def test_converged_batch_of_the_recorded_pairs(ops):
    import kkt_certificate as kc
    from test_optimality_gpu import _check_nlp
    pairs = list(tc.TWIN)
    bt = Batch(tc.TRACKS, [tc.TRACKS.index(t) for t, _ in pairs], [v for _, v in pairs])
    X, U, T, st = bt.solve(ops, max_iter=200, tol=1e-6)
    for b, p in enumerate(pairs):
        lap, iters = tc.TWIN[p]
        print(f"{p[1]} on {p[0]}: iterations {st[b, 0]:.0f} (twin {iters}), lap {st[b, 4]:.6f} s (twin {lap:.6f}), "
              f"difference {st[b, 4] - lap:+.2e} s, status {st[b, 5]:.0f}")
    lap = {p: st[b, 4] for b, p in enumerate(pairs)}
    print(f"base vehicle: lap on the base track {lap['base', 'base']!r} s, on its mirror image {lap['mirrored', 'base']!r} s, "
          f"difference {lap['mirrored', 'base'] - lap['base', 'base']:+.2e} s")
    assert (st[:, 5] == 1.0).all(), st[:, 5]
    for b, p in enumerate(pairs):
        assert abs(st[b, 4] - tc.TWIN[p][0]) <= 1e-6, (p, st[b, 4], tc.TWIN[p][0])
    for b, p in enumerate(pairs):   # every result is a first-order optimum of ITS track's and vehicle's problem, by the pinned functions
        d = bt.d[bt.track_of[b]]
        nlp = kc.DoubleTrackNLP(vc.model(p[1]), d["s"], d["kappa"], d["left"], d["right"], d["L"], d["atw"], d["cap"])
        _check_nlp(f"tracks batch row {b} ({p[1]} on {p[0]})", nlp, nlp.to_w(X[b], U[b], T[b]), st[b])


def test_host_entry_equals_the_device_entry_on_a_forked_batch(ops):
    import torch
    bt = _mixed()
    kw = dict(max_iter=200, tol=1e-6)
    Xh, Uh, Th, sth = bt.solve(ops, **kw)
    dev = torch.device("cuda", 0)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    X, U, T = g(bt.X0), g(bt.U0), g(bt.T0)
    st = ops.mintime_solve_tracks_torch(vc.models(bt.vehicles), bt.track_of, g(bt.s), g(bt.kappa), g(bt.left), g(bt.right), MARGIN, bt.L,
                                        X, U, T, bt.atw, bt.cap, **kw)
    torch.cuda.synchronize()
    print("host / device entry: iterations", sth[:, 0], st.cpu().numpy()[:, 0], "status", sth[:, 5])
    assert (sth[:, 5] == 1.0).all() and sth[:, 0].max() < 200
    _equal((X.cpu().numpy(), U.cpu().numpy(), T.cpu().numpy(), st.cpu().numpy()), (Xh, Uh, Th, sth), "device entry")


def test_short_lap_takes_the_two_front_kernel(ops):
    """Fewer than 64 nodes on two tracks (base and scaled at N = 37): k_mt_kkt, and a node count that leaves tails in every grid."""
    names = ["mu x 0.9", "mass x 1.1", "base"]
    bt = Batch(["base", "scaled"], [1, 0, 1], names, n=37)
    assert bt.s.shape == (2, 37) and 8 <= bt.n < 64
    res = bt.solve(ops, **IT12)
    assert (res[3][:, 0] == 12.0).all() and np.isfinite(res[0]).all()
    for b in range(3):
        _equal([a[b] for a in res], [a[0] for a in bt.single(ops, b, **IT12)], f"instance {b}")
    assert np.abs(res[0][0] - res[0][2]).max() > 1e-6


def test_a_bad_track_is_refused_and_nothing_runs(ops):
    from spline_trajectory_optimization_amd import _lib
    bt = Batch(tc.TRACKS, [0, 1, 2, 3, 2], vc.NAMES)
    ctx = _lib.Context.get(0)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    tab = ops.dt_models_table(vc.models())
    for what, track_of, L in (("instance 3: track 4 outside", [0, 1, 2, 4, 2], bt.L),
                              ("track 1: track_length", [0, 1, 2, 3, 2], bt.L * np.array([1.0, 0.0, 1.0, 1.0]))):
        X, U, T = bt.X0.copy(), bt.U0.copy(), bt.T0.copy()
        st = np.full((5, 12), -7.0)
        of, L = np.array(track_of, dtype=np.int32), np.ascontiguousarray(L)
        rc = ctx.lib.rl_mintime_solve_tracks(ctx.h, p(tab), 1, 5, tc.N, 4, of.ctypes.data_as(ip), p(bt.s), p(bt.kappa), p(bt.left),
                                             p(bt.right), MARGIN, p(L), p(bt.atw), p(bt.cap), p(X), p(U), p(T), 12, 1e-12, p(st))
        msg = ctx.lib.rl_last_error().decode()
        print(f"rc {rc}, '{msg}'")
        assert rc == -1 and what in msg                                          # RL_ERR_ARG
        np.testing.assert_array_equal(X, bt.X0); np.testing.assert_array_equal(U, bt.U0); np.testing.assert_array_equal(T, bt.T0)
        assert (st == -7.0).all()                                               # nothing ran, nothing came back
        with pytest.raises(ValueError, match=what):
            ops.mintime_solve_tracks(tab, of, bt.s, bt.kappa, bt.left, bt.right, MARGIN, L, bt.X0, bt.U0, bt.T0, bt.atw, bt.cap, **IT12)


def _race_tracks():
    from spline_trajectory_optimization_amd.models.race_track import race_track_with_nodes
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    est = vc.defaults.ESTIMATES
    veh = Vehicle(VehicleParams(np.array(est["acc_speed_loopup"]), np.array(est["dcc_speed_lookup"]), est["max_lon_acc_mpss"],
                                est["max_lon_dcc_mpss"], est["max_left_acc_mpss"], est["max_right_acc_mpss"],
                                est["max_speed_mps"], est["max_jerk_mpsc"]))
    rts = []
    for name in ("base", "scaled"):
        centre, left, right = tc.arrays(name)
        rts.append(race_track_with_nodes(name, left, right, centre, tc.N, s=1.0))
    return rts, veh


def test_the_chain_on_two_tracks_and_two_vehicles(ops):
    """optimise_tracks_batch on the base and the scaled track x two vehicles: byte for byte its steps issued one by one through
    ops, and per track the tables of optimise_track_batch to the 1e-12 relative of test_the_chain_with_one_model_per_instance."""
    import torch
    from spline_trajectory_optimization_amd import _lib, batch
    from spline_trajectory_optimization_amd.min_time_optm.min_time_optimizer import optimise_track_batch, optimise_tracks_batch
    from spline_trajectory_optimization_amd.models.trajectory import _ring_coords
    rts, veh = _race_tracks()
    assert [len(rt.center_d) for rt in rts] == [tc.N, tc.N]
    ms = vc.models(["base", "mass x 1.1"])
    atw, cap = [7.0, 8.75], [30.0, 30.0]
    kw = dict(max_iter=200, tol=1e-6)
    res = optimise_tracks_batch(rts, veh, None, models=ms, average_track_width=atw, speed_cap=cap, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items() if k not in ("tracks", "track_of")}
    np.testing.assert_array_equal(res["track_of"], [0, 0, 1, 1])                 # track-major
    assert out["X"].shape == (4, tc.N, 6) and (out["stats"][:, 5] == 1.0).all()
    rel = np.abs(out["summary"][:, 0] / out["stats"][:, 4] - 1.0).max()
    print(f"[tracks chain] lap time of the tables against the solver's: {rel:.2e} relative; laps {out['stats'][:, 4]}")
    assert rel <= 1e-12
    # the steps one by one
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    s_h = [np.ascontiguousarray(rt.abscissa) for rt in rts]
    X = torch.empty((4, tc.N, 6), dtype=torch.float64, device=dev); U = torch.empty((4, tc.N, 4), dtype=torch.float64, device=dev)
    T = torch.empty((4, tc.N), dtype=torch.float64, device=dev)
    bases = []
    for t, rt in enumerate(rts):
        traj = rt.center_d.copy(); rt.fill_trajectory_boundaries(traj)
        base = up(traj.points)[None].contiguous()
        ops.qss_sim_torch(base, *batch.vehicle_tables(veh))
        bases.append(base[0])
        X[2 * t:2 * t + 2], U[2 * t:2 * t + 2], T[2 * t:2 * t + 2] = batch.min_time_centerline_guess_torch(up(s_h[t]), base[0], 2)
    left = up(np.stack([rts[t].left_intp(s_h[t]) for t in (0, 0, 1, 1)])); right = up(np.stack([rts[t].right_intp(s_h[t]) for t in (0, 0, 1, 1)]))
    st = ops.mintime_solve_tracks_torch(ms * 2, np.array([0, 0, 1, 1]), up(np.stack(s_h)), up(np.stack([rt.curvature_intp(s) for rt, s in zip(rts, s_h)])),
                                        left, right, MARGIN, [float(rt.center_s.get_length()) for rt in rts], X, U, T, atw, cap, **kw)
    pts = []
    for t, rt in enumerate(rts):
        res["tracks"][t].set_rings(_ring_coords(rt.left_r), _ring_coords(rt.right_r))
        pts.append(batch.min_time_tables_torch(rt, res["tracks"][t], X[2 * t:2 * t + 2], T[2 * t:2 * t + 2], _lib.BOUNDS_SHARED_RINGS, None,
                                               base=bases[t]))
    pts = torch.cat(pts)
    summ = ops.table_summary_torch(pts)
    torch.cuda.synchronize()
    for k, v in (("X", X), ("U", U), ("T", T), ("stats", st), ("points", pts), ("summary", summ)):
        assert out[k].tobytes() == v.cpu().numpy().tobytes(), k
    # per track: optimise_track_batch with the two vehicles
    for t, rt in enumerate(rts):
        one = optimise_track_batch(rt, veh, None, models=ms, average_track_width=atw[t], speed_cap=cap[t], track=res["tracks"][t], **kw)
        torch.cuda.synchronize()
        sl = slice(2 * t, 2 * t + 2)
        np.testing.assert_array_equal(out["X"][sl], one["X"].cpu().numpy(), err_msg=f"track {t} X")
        np.testing.assert_array_equal(out["stats"][sl], one["stats"].cpu().numpy(), err_msg=f"track {t} stats")
        p1 = one["points"].cpu().numpy()
        scale = np.maximum(np.abs(p1).max(axis=(0, 1)), 1.0)
        rel = (np.abs(out["points"][sl] - p1) / scale).max()
        print(f"[tracks chain] track {t}: tables against optimise_track_batch {rel:.2e} relative")
        assert rel <= 1e-12
    assert np.abs(out["stats"][0, 4] - out["stats"][2, 4]) > 1.0                  # two circuits, two laps
