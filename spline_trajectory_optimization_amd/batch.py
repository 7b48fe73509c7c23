"""Batched min-curvature solves: workload generators for the BASELINE.json configs and the
rank-sharding helpers (one process per GPU, independent track instances, one gather).

No arithmetic of the hot path lives here: instances are solved by rl_mincurv_solve_batch_* (HIP).
"""
import os

import numpy as np

from . import _lib, ops
from .models.trajectory import BSplineTrajectory

_PKG = os.path.dirname(os.path.abspath(__file__))
MONZA_DIR = os.path.join(_PKG, "examples", "race_track", "monza")


def load_track_csv(path):
    """x,y columns of a track CSV (tests/test_trajectory.py:9-15 reads usecols=(0,1))."""
    return np.loadtxt(path, dtype=np.float64, delimiter=",", skiprows=1, usecols=(0, 1))


def load_track_rows(path):
    """All numeric columns of a track CSV: 3 columns x,y,z or 4 columns x,y,z,bank (README.md:28-35;
    the reference itself only ever reads columns 0-1, race_track.py:23-25)."""
    rows = np.loadtxt(path, dtype=np.float64, delimiter=",", skiprows=1, ndmin=2)
    assert rows.shape[1] in (2, 3, 4), rows.shape
    return rows


def save_track_rows(path, rows):
    rows = np.asarray(rows, dtype=np.float64)
    header = ",".join(["x", "y", "z", "bank"][:rows.shape[1]])
    np.savetxt(path, rows, delimiter=",", header=header, comments="", fmt="%.17g")


def bank_on_samples(raw_xy, raw_bank, points):
    """BASELINE config 4: bank angle [rad] of the raw 4-column track rows carried onto the samples of
    a trajectory table -- for every sample the two nearest consecutive raw points, linear in the
    projection onto their segment.  Returns float64 [N] (what goes into Trajectory.BANK, column 13;
    only the simulator reads it, simulator.py:51-58)."""
    raw_xy = np.asarray(raw_xy, dtype=np.float64); raw_bank = np.asarray(raw_bank, dtype=np.float64)
    p = np.asarray(points)[:, :2]
    d2 = ((p[:, None, :] - raw_xy[None, :, :]) ** 2).sum(axis=2)
    j = d2.argmin(axis=1)
    P = len(raw_xy)
    jn, jp = (j + 1) % P, (j - 1) % P
    use_next = d2[np.arange(len(p)), jn] <= d2[np.arange(len(p)), jp]
    j0 = np.where(use_next, j, jp); j1 = np.where(use_next, jn, j)
    seg = raw_xy[j1] - raw_xy[j0]
    tpar = ((p - raw_xy[j0]) * seg).sum(axis=1) / np.maximum((seg * seg).sum(axis=1), 1e-300)
    tpar = np.clip(tpar, 0.0, 1.0)
    return raw_bank[j0] * (1.0 - tpar) + raw_bank[j1] * tpar


def load_monza():
    return (load_track_csv(os.path.join(MONZA_DIR, "MONZA_UNOPTIMIZED_LINE_enu.csv")),
            load_track_csv(os.path.join(MONZA_DIR, "MONZA_LEFT_BOUNDARY_enu.csv")),
            load_track_csv(os.path.join(MONZA_DIR, "MONZA_RIGHT_BOUNDARY_enu.csv")))


def monza_sectors(n_sectors=8, refine=4):
    """Sector polygons of Monza for region tagging (tools/time_region.py, tests/test_region_gpu.py): the left boundary cut
    into `n_sectors` stretches of equal vertex count, each closed by the reversed stretch of the right boundary between the
    right-boundary vertices nearest to its two ends.  `refine` > 1 inserts refine - 1 points on every boundary segment
    first (same polylines, more vertices).  Returns a list of [n, 2] float64 vertex arrays."""
    _, left, right = load_monza()

    def dense(ring):
        nxt = np.roll(ring, -1, axis=0)
        f = np.arange(refine)[None, :, None] / refine
        return (ring[:, None, :] + f * (nxt - ring)[:, None, :]).reshape(-1, 2)

    left, right = dense(left), dense(right)
    nL, nR = len(left), len(right)
    cuts = [i * nL // n_sectors for i in range(n_sectors)] + [nL]
    near = [int(np.argmin(np.hypot(*(right - left[c % nL]).T))) for c in cuts]
    out = []
    for s_ in range(n_sectors):
        li = np.arange(cuts[s_], cuts[s_ + 1] + 1) % nL
        rj = (near[s_] + np.arange((near[s_ + 1] - near[s_]) % nR + 1)) % nR
        out.append(np.vstack([left[li], right[rj[::-1]]]))
    return out


def monza_centerline(s=100.0, k=5):
    """The centre-line spline of tests/test_optimizer.py:16-17 (host FITPACK fit)."""
    centre, _, _ = load_monza()
    return BSplineTrajectory(centre, s, k)


def half_widths_from_bounds(points):
    """|p - L|, |p - R| per sample from a bounds-filled [N,19] table."""
    wl = np.hypot(points[:, 9] - points[:, 0], points[:, 10] - points[:, 1])
    wr = np.hypot(points[:, 11] - points[:, 0], points[:, 12] - points[:, 1])
    return wl, wr


def width_batch(w_left, w_right, B, seed=1234, eps=0.15, floor=1.5):
    """per-instance widths w[b,i] = w[i] * (1 + e[b]), e ~ U(-eps, eps)
    from numpy.random.default_rng(seed), floored at `floor` metres.  Returns float64 [B,N,2]."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-eps, eps, size=(B, 2))
    w = np.empty((B, len(w_left), 2))
    w[:, :, 0] = np.maximum(w_left[None, :] * (1.0 + e[:, 0:1]), floor)
    w[:, :, 1] = np.maximum(w_right[None, :] * (1.0 + e[:, 1:2]), floor)
    return w


def i_start_range(n, k, driver="sweep"):
    """[lo, hi) of np.random.randint for the start index: optimizer.py:303 (driver "sweep") or the sliding window's,
    optimizer.py:178 (driver "window")."""
    if driver == "window":
        return ops.window_i_start_range(n, k)
    if driver != "sweep":
        raise ValueError(f"driver: expected 'sweep' or 'window', got {driver!r}")
    return k // 2, n - (k - k // 2)


def default_i_start(n, k, max_iter, seed=0, driver="sweep"):
    """A pinned stand-in for the unseeded np.random.randint of optimizer.py:303 (driver "window": of optimizer.py:178)."""
    lo, hi = i_start_range(n, k, driver)
    rng = np.random.RandomState(seed)
    return np.array([rng.randint(lo, hi) for _ in range(max_iter)], dtype=np.int32)


def default_i_start_batch(n, k, max_iter, B, seed=0, driver="sweep"):
    """B draws of the start indices, row b = default_i_start(seed=seed + b): int32 [B,max_iter] for the per-instance
    form of ops.solve_batch_host / _torch ("how much does the line depend on the draw": B draws, one launch)."""
    return np.stack([default_i_start(n, k, max_iter, seed=seed + b, driver=driver) for b in range(B)]).astype(np.int32)


def polish_lines_torch(track, xy, bounds_form, bounds, i_start, u=None, search=_lib.SEARCH_WINDOWED, arith=None,
                       driver="sweep"):
    """Lines that are not the track's -> sweep: fit every instance's points onto the track's knots (ops.spline_fit_torch:
    xy [B,P,2] points or [B,P,19] tables, e.g. the pose tables of a min-time batch), then sweep every instance from its fit
    (ops.solve_batch_torch with ctrl0 = the fit), both enqueued on torch's current stream with no host round trip.  An
    instance whose fit failed (fit_stats[:,0] != 0) starts from the track's control points.  i_start [max_iter] or
    [B,max_iter].  driver: "sweep" or "window" (the sliding-window driver polishes the fit).  Returns the dict of
    solve_batch_torch plus fit_ctrl [B,n,2] and fit_stats [B,4]."""
    fit_ctrl, fit_stats = ops.spline_fit_torch(track, xy, u=u)
    out = ops.solve_batch_torch(track, bounds_form, bounds, i_start, search=search, arith=arith, ctrl0=fit_ctrl, driver=driver)
    out["fit_ctrl"] = fit_ctrl
    out["fit_stats"] = fit_stats
    return out


def make_track(spline: BSplineTrajectory, N: int, device=None):
    t, cx, cy, k = spline._tck()
    return _lib.Track(_lib.Context.get(device), t, cx, cy, k, N)


# ---------------------------------------------------------------- solved batch -> tables -> lap times
def vehicle_tables(vehicle):
    """(acc_x, acc_c, dcc_x, dcc_c, params) of a Vehicle as rl_qss_sim takes them; a 5-tuple is passed through."""
    if isinstance(vehicle, (tuple, list)):
        if len(vehicle) != 5:
            raise ValueError("vehicle: a Vehicle or the 5-tuple (acc_x, acc_c, dcc_x, dcc_c, params)")
        return tuple(vehicle)
    p = vehicle.param
    acc, dcc = vehicle.acc_intp, vehicle.dcc_intp   # scipy CubicSpline (vehicle.py:21-24)
    params = np.array([p.max_lon_acc_mpss, p.max_lon_dcc_mpss, p.max_left_acc_mpss, p.max_right_acc_mpss, p.max_speed_mps,
                       p.max_jerk], dtype=np.float64)
    return (np.ascontiguousarray(acc.x), np.ascontiguousarray(acc.c), np.ascontiguousarray(dcc.x),
            np.ascontiguousarray(dcc.c), params)


def vehicle_tables_batch(vehicles):
    """B vehicles as rl_qss_sim_vehicles_* takes them: a sequence of Vehicles or 5-tuples (vehicle_tables) -> the five stacked
    arrays acc_x [B,m+1], acc_c [B,4,m], dcc_x [B,m'+1], dcc_c [B,4,m'], params [B,6] (numpy float64, C-contiguous).
    Breakpoints and coefficients may differ per vehicle; the piece counts m, m' are common to the batch (the kernels' LDS
    layout depends on them): ValueError naming the first vehicle whose counts differ from vehicle 0's."""
    tabs = [vehicle_tables(v) for v in vehicles]
    if not tabs:
        raise ValueError("vehicles: empty sequence")
    tabs = [tuple(np.asarray(a, dtype=np.float64) for a in t) for t in tabs]
    m0 = (len(tabs[0][0]) - 1, len(tabs[0][2]) - 1)
    for b, t in enumerate(tabs):
        ax, ac, dx, dc, pr = t
        m = (len(ax) - 1, len(dx) - 1)
        if ac.shape != (4, m[0]) or dc.shape != (4, m[1]) or pr.shape != (6,):
            raise ValueError(f"vehicles[{b}]: expected acc_c [4,{m[0]}], dcc_c [4,{m[1]}], params [6]")
        if m != m0:
            raise ValueError(f"vehicles[{b}]: {m[0]} / {m[1]} pieces in the acc / dcc lookup, vehicles[0] has {m0[0]} / {m0[1]}: "
                             "piece counts are common to a batch")
    return tuple(np.ascontiguousarray(np.stack([t[q] for t in tabs])) for q in range(5))


def _one_of(vehicle, vehicles):
    if (vehicle is None) == (vehicles is None):
        raise ValueError("exactly one of vehicle (shared by the batch) and vehicles (one per instance) must be given")


def _vehicles_stacked(vehicles, B, device=None):
    """`vehicles` of lap_times_*: B Vehicles / 5-tuples, or the stacked 5-tuple of vehicle_tables_batch as numpy arrays or cuda
    tensors -> the stacked 5-tuple as cuda tensors on `device`, or as numpy arrays for device None."""
    stacked = isinstance(vehicles, (tuple, list)) and len(vehicles) == 5 and all(hasattr(a, "ndim") for a in vehicles)
    veh = tuple(vehicles) if stacked else vehicle_tables_batch(vehicles)
    if int(veh[4].shape[0]) != B:
        raise ValueError(f"vehicles: {int(veh[4].shape[0])} vehicles for {B} instances")
    if device is None:
        return tuple(a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in veh)
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device) if isinstance(a, np.ndarray) else a
                 for a in veh)


def lap_times_torch(track, ctrl, bounds_form, bounds, length, vehicle=None, bank=None, vehicles=None):
    """Which of these B solved lines is the fastest lap, and what is its table: tables of the batch (ops.tables_torch) ->
    QSS simulation in place (ops.qss_sim_torch) -> per-instance summary (ops.table_summary_torch), all enqueued on torch's
    current stream with no host round trip.  ctrl [B,n,2] (e.g. solve_batch_torch(...)["ctrl"]), bounds / bank as for
    ops.tables_torch, vehicle = a Vehicle or vehicle_tables(...).  vehicles (instead of vehicle) = one vehicle per instance
    (ops.qss_sim_vehicles_torch): B Vehicles / 5-tuples, or the stacked 5-tuple of vehicle_tables_batch as numpy arrays or
    cuda tensors.  Returns dict(points [B,N,19], iters [B] int32, summary [B,8] in the order of ops.SUMMARY_COLUMNS) of cuda
    tensors."""
    _one_of(vehicle, vehicles)
    if vehicles is None:
        veh = vehicle_tables(vehicle)
    else:
        if getattr(ctrl, "ndim", None) != 3:
            raise ValueError(f"ctrl: expected [B,{track.n},2]")
        veh = _vehicles_stacked(vehicles, int(ctrl.shape[0]), ctrl.device)
    points = ops.tables_torch(track, ctrl, bounds_form, bounds, length, bank=bank)
    iters = ops.qss_sim_torch(points, *veh) if vehicles is None else ops.qss_sim_vehicles_torch(points, *veh)
    summary = ops.table_summary_torch(points, iters)
    return {"points": points, "iters": iters, "summary": summary}


def lap_times_grid_torch(track, ctrl, bounds_form, bounds, length, vehicles, bank=None):
    """Every one of L lines under every one of V vehicles: the L tables once (ops.tables_torch), expanded to L V instances on
    the device (instance l V + v = line l, vehicle v), ONE QSS launch with per-instance vehicles (ops.qss_sim_vehicles_torch)
    and the summary, all enqueued on torch's current stream with no host round trip.  ctrl [L,n,2], bounds / bank as for
    ops.tables_torch; vehicles: V Vehicles / 5-tuples or the stacked 5-tuple of vehicle_tables_batch (numpy or cuda).
    Returns dict(summary [L,V,8] in the order of ops.SUMMARY_COLUMNS, iters [L,V] int32, points [L,V,N,19]) of cuda tensors."""
    if getattr(ctrl, "ndim", None) != 3:
        raise ValueError(f"ctrl: expected [L,{track.n},2]")
    L = int(ctrl.shape[0])
    stacked = isinstance(vehicles, (tuple, list)) and len(vehicles) == 5 and all(hasattr(a, "ndim") for a in vehicles)
    V = int(vehicles[4].shape[0]) if stacked else len(vehicles)
    veh = _vehicles_stacked(vehicles, V, ctrl.device)
    lines = ops.tables_torch(track, ctrl, bounds_form, bounds, length, bank=bank)
    N = int(lines.shape[1])
    points = lines[:, None].expand(L, V, N, _lib.NCOL).contiguous().view(L * V, N, _lib.NCOL)
    veh = tuple(a[None].expand((L,) + tuple(a.shape)).contiguous().view((L * V,) + tuple(a.shape[1:])) for a in veh)
    iters = ops.qss_sim_vehicles_torch(points, *veh)
    summary = ops.table_summary_torch(points, iters)
    return {"summary": summary.view(L, V, -1), "iters": iters.view(L, V), "points": points.view(L, V, N, _lib.NCOL)}


def lap_times_host(track, ctrl, bounds_form, bounds, length, vehicle=None, bank=None, vehicles=None):
    """lap_times_torch for numpy input (float64, C-contiguous): copies in, runs the same chain on the track's device, copies
    out.  Returns dict(points, iters, summary) of numpy arrays."""
    import torch
    _one_of(vehicle, vehicles)
    veh = vehicle_tables(vehicle) if vehicles is None else None
    B = ops.check_tables_host(track, ctrl, bounds_form, bounds, bank)
    dev = torch.device("cuda", track.ctx.device)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    if vehicles is not None:
        vehicles = _vehicles_stacked(vehicles, B, dev)
    out = lap_times_torch(track, up(ctrl), bounds_form, up(bounds), length, veh, bank=up(bank), vehicles=vehicles)
    return {k_: v.cpu().numpy() for k_, v in out.items()}


SPEED_COLUMN = 4   # Trajectory.SPEED


def vehicle_lines_torch(track, widths, length, vehicles, rounds=2, margin=0.0, n_outer=6, bank=None):
    """One racing line per vehicle: the speed-weighted global min-curvature QP iterated with the QSS simulator, all enqueued
    on torch's current stream with no host round trip.  Round 0 is the unweighted global QP (ops.global_batch_torch); each of
    the `rounds` further rounds simulates every vehicle on its current line (lap_times_torch(..., vehicles=vehicles)), takes
    w = 1 / SPEED of its table with a torch op on the device, and solves the QP again under those weights
    (ops.global_batch_torch(weights=w)): the line spends the track's width where THAT vehicle is slow.  Every QP starts from
    the track's own line.  widths [1,N,2] (one track for every vehicle) or [B,N,2], float64 cuda; vehicles: B Vehicles /
    5-tuples or the stacked 5-tuple of vehicle_tables_batch (numpy or cuda); B is the number of vehicles; bank as for
    ops.tables_torch.  A failed simulation whose speed is zero gives an infinite weight: the kernel refuses that instance (it
    comes back as the track's line) and reports it in stats[r, b, 6].
    Returns dict(ctrl [B,n,2], summary [rounds+1,B,8] (ops.SUMMARY_COLUMNS of every round's lines), stats [rounds+1,B,8] (the
    QP's), weights [B,N] (those of the last round; ones for rounds=0), points [B,N,19] (the simulated tables of ctrl))."""
    import torch
    if getattr(widths, "ndim", None) != 3 or tuple(widths.shape[1:]) != (track.N, 2):
        raise ValueError(f"widths: expected [1,{track.N},2] or [B,{track.N},2]")
    if int(rounds) < 0:
        raise ValueError("rounds: must be >= 0")
    stacked = isinstance(vehicles, (tuple, list)) and len(vehicles) == 5 and all(hasattr(a, "ndim") for a in vehicles)
    B = int(vehicles[4].shape[0]) if stacked else len(vehicles)
    if int(widths.shape[0]) not in (1, B):
        raise ValueError(f"widths: {int(widths.shape[0])} instances for {B} vehicles")
    ops._check_torch(widths, "widths", tuple(widths.shape))
    veh = _vehicles_stacked(vehicles, B, widths.device)
    widths = widths.expand(B, track.N, 2).contiguous()
    weights = torch.ones((B, track.N), dtype=torch.float64, device=widths.device)
    summary, stats = [], []
    for r in range(int(rounds) + 1):
        sol = ops.global_batch_torch(track, widths, margin, n_outer, weights=None if r == 0 else weights)
        lap = lap_times_torch(track, sol["ctrl"], _lib.BOUNDS_WIDTHS, widths, length, bank=bank, vehicles=veh)
        summary.append(lap["summary"]); stats.append(sol["stats"])
        if r < int(rounds):
            weights = (1.0 / lap["points"][:, :, SPEED_COLUMN]).contiguous()
    return {"ctrl": sol["ctrl"], "summary": torch.stack(summary), "stats": torch.stack(stats), "weights": weights,
            "points": lap["points"]}


def vehicle_lines_host(track, widths, length, vehicles, rounds=2, margin=0.0, n_outer=6, bank=None):
    """vehicle_lines_torch for numpy input (float64, C-contiguous): copies in, runs the same chain on the track's device,
    copies out.  Returns the same dict of numpy arrays."""
    import torch
    if not isinstance(widths, np.ndarray) or widths.ndim != 3:
        raise ValueError(f"widths: expected a numpy array [1,{track.N},2] or [B,{track.N},2]")
    ops._check_np(widths, "widths", (widths.shape[0], track.N, 2))
    if bank is not None:
        ops._check_np(bank, "bank", tuple(bank.shape))
    dev = torch.device("cuda", track.ctx.device)
    out = vehicle_lines_torch(track, torch.from_numpy(widths).to(dev), length, vehicles, rounds, margin, n_outer,
                              bank=None if bank is None else torch.from_numpy(bank).to(dev))
    return {k_: v.cpu().numpy() for k_, v in out.items()}


def min_time_tables_torch(race_track, track, X, T, bounds_form, bounds, base=None, pieces=None):
    """Tables of a batch the min-time solve returned (ops.mintime_solve_torch): X [B,N,6] in race_track's curvilinear frame, T
    [B,N] -> points [B,N,19] with X, Y, YAW, SPEED, the bounds, the distances and TIME filled (ops.pose_tables_torch, form
    POSE_FRENET), every other column from `base` ([N,19] or [B,N,19], e.g. the QSS table the solve started from).
    bounds_form / bounds as for ops.pose_tables_torch (rings of track.N vertices in the widths / points forms).  pieces:
    race_track.centerline_pieces() as cuda tensors on X's device; None uploads them with this call (three small copies), so a
    caller that makes many calls passes its own.  Enqueues on torch's current stream, no sync.  Returns the cuda tensor."""
    import torch
    if pieces is None:
        pieces = tuple(torch.from_numpy(a).to(X.device) for a in race_track.centerline_pieces())
    return ops.pose_tables_torch(track, _lib.POSE_FRENET, X, pieces, bounds_form, bounds, base=base, T=T)


def min_time_tables_host(race_track, track, X, T, bounds_form, bounds, base=None):
    """min_time_tables_torch for numpy input (float64, C-contiguous): rl_pose_tables_batch_host.  Returns points [B,N,19]."""
    return ops.pose_tables_host(track, _lib.POSE_FRENET, X, race_track.centerline_pieces(), bounds_form, bounds, base=base, T=T)


# ---------------------------------------------------------------- min-time NLP plumbing (config 5)
def min_time_initial_guess(points):
    """The initial guess the reference hands to its min-time NLP when no previous solution is given
    (min_time_optimizer.py:146-151): the QSS-simulated table's abscissa, speed and segment times, zero
    lateral offset / relative yaw / yaw rate / slip, controls (1, -1, 0.001, 0) in physical units.
    `points` = [N,19] after Simulator.run_simulation (rl_qss_sim).  Returns (s [N], X [N,6], U [N,4], T [N])
    ready for ops.dt_eval_nodes / ops.dt_eval_jac."""
    pts = np.asarray(points, dtype=np.float64)
    N = len(pts)
    s = pts[:, 6].copy()                      # DIST_TO_SF_BWD: race_track.abscissa (race_track.py:56)
    X = np.zeros((N, 6)); X[:, 0] = s; X[:, 5] = pts[:, 4]
    U = np.tile(np.array([1.0, -1.0, 0.001, 0.0]), (N, 1))
    T = pts[:, 16].copy()
    return s, X, U, T


MIN_TIME_U0 = (1.0, -1.0, 0.001, 0.0)   # the reference's constant controls of an initial guess (min_time_optimizer.py:146-151)


def min_time_centerline_guess_torch(s_nodes, base, B):
    """The guess optimise_track_batch hands the NLP without start lines: on the centre line with the QSS table's speeds and
    times.  s_nodes [N], base [N,19] (simulated centre-line table) or [B,N,19] (one per instance: vehicle sweeps), cuda
    tensors.  Returns (X0 [B,N,6], U0 [B,N,4], T0 [B,N])."""
    import torch
    N = int(s_nodes.shape[0])
    if base.ndim == 3 and int(base.shape[0]) != B:
        raise ValueError(f"base: {int(base.shape[0])} tables for {B} instances")
    X = torch.zeros((B, N, 6), dtype=torch.float64, device=s_nodes.device)
    X[:, :, 0] = s_nodes
    X[:, :, 5] = base[..., 4]
    U = torch.tensor(MIN_TIME_U0, dtype=torch.float64, device=s_nodes.device).repeat(B, N, 1).contiguous()
    T = base[:, :, 16].contiguous() if base.ndim == 3 else base[:, 16].repeat(B, 1).contiguous()
    return X, U, T


def min_time_guess_from_lines_torch(race_track, points, s_nodes, kappa_nodes, base, pieces=None):
    """Initial guesses of the min-time NLP from B lines in global coordinates, e.g. the simulated tables of a min-curvature
    batch (lap_times_torch(...)["points"]): project every line onto race_track's centre line (ops.frenet_torch), take its
    lateral offset, relative heading and SPEED at the NLP's nodes (ops.frenet_resample_torch), and from them
        X0[b,j] = (s_j, n_j, xi_j, 0, 0, v_j),  U0 = MIN_TIME_U0,  T0[b,j] = (s_{j+1} - s_j) (1 - n_j kappa_j) / (v_j cos xi_j)
    (the last step closes with the track length; the model's s_dot at zero slip).  points [B,P,19], s_nodes [N], kappa_nodes
    [N], base [N,19] (the simulated centre-line table): float64 cuda tensors; pieces: race_track.centerline_pieces() as cuda
    tensors (None uploads them).  An instance whose line cannot be used -- a point that did not project, an abscissa that
    is not cyclically increasing, a step time that is not positive and finite -- gets the centre-line guess of
    min_time_centerline_guess_torch instead (torch.where: no host round trip).  Enqueues on torch's current stream, no sync.
    Returns (X0 [B,N,6], U0 [B,N,4], T0 [B,N], status int32 [B]: 0 = from the line, 1 = projection / abscissa, 2 = step time)."""
    import torch
    dev = points.device
    if pieces is None:
        pieces = tuple(torch.from_numpy(a).to(dev) for a in race_track.centerline_pieces())
    if getattr(points, "ndim", None) != 3 or points.shape[2] != _lib.NCOL:
        raise ValueError("points: expected [B,P,19]")
    B, N = int(points.shape[0]), int(s_nodes.shape[0])
    ops._check_torch(kappa_nodes, "kappa_nodes", (N,))
    ops._check_torch(base, "base", (N, _lib.NCOL))
    length = float(race_track.center_s.get_length())
    fr, _, fstats = ops.frenet_torch(pieces, points)
    res, rstatus = ops.frenet_resample_torch(fr, points[:, :, 4:5].contiguous(), s_nodes, length)
    n, xi, v = res[:, :, 0], res[:, :, 1], res[:, :, 2]
    ds = torch.cat([s_nodes[1:], s_nodes.new_full((1,), length)]) - s_nodes
    T = ds[None, :] * (1.0 - n * kappa_nodes[None, :]) / (v * torch.cos(xi))
    bad_line = (rstatus != 0) | (fstats[:, 0] != 0)
    bad_time = ~(torch.isfinite(T) & (T > 0)).all(dim=1)
    status = torch.where(bad_line, 1, torch.where(bad_time, 2, 0)).to(torch.int32)
    Xc, U, Tc = min_time_centerline_guess_torch(s_nodes, base, B)
    X = torch.zeros_like(Xc)
    X[:, :, 0] = s_nodes
    X[:, :, 1], X[:, :, 2], X[:, :, 5] = n, xi, v
    use = (status != 0)
    X = torch.where(use[:, None, None], Xc, X).contiguous()
    T = torch.where(use[:, None], Tc, T).contiguous()
    return X, U, T, status


def _unwrap_torch(p):
    """numpy.unwrap along the last axis (period 2 pi) with torch ops."""
    import torch
    dd = p[..., 1:] - p[..., :-1]
    ddmod = torch.remainder(dd + np.pi, 2.0 * np.pi) - np.pi
    ddmod = torch.where((ddmod == -np.pi) & (dd > 0), torch.full_like(ddmod, np.pi), ddmod)
    corr = torch.where(dd.abs() < np.pi, torch.zeros_like(dd), ddmod - dd)
    out = p.clone()
    out[..., 1:] = p[..., 1:] + corr.cumsum(dim=-1)
    return out


def bicycle_inputs_from_tables_torch(points):
    """What the bicycle NLP reads of B tables, with torch ops on the tables' device: points [B,N,19] (float64 cuda tensor, e.g.
    lap_times_torch(...)["points"]) -> dict(P0 [B,N,2], yaw [B,N], dl [B,N] >= 0, dr [B,N] <= 0, X0 [B,N,5], U0 [B,N,2], T0 [B,N],
    usable [B] bool): the line, its headings, the distances to its bounds and the centre-line guess, with BicycleProblem's
    expressions (SPEED where it is filled, else 10 m/s).  The distances are norms, as in the reference: a table whose bound
    point IS the line's point -- what rl_tables_batch_* writes where the normal ray finds no crossing, i.e. where the line lies
    on or outside that bound (models/trajectory.py:127) -- gives dl == 0 or dr == 0 there.  The solver needs dr < dl at every
    node, which holds while only one side is 0; usable[b] says that instance b has it, with every value finite.  Lines meant
    for this chain should keep a margin to the bounds in the solve that made them.  No host round trip."""
    import torch
    from .models.trajectory import Trajectory as Tr
    if getattr(points, "ndim", None) != 3 or points.shape[2] != _lib.NCOL:
        raise ValueError("points: expected [B,N,19]")
    ops._check_torch(points, "points", points.shape)
    B, N = int(points.shape[0]), int(points.shape[1])
    P0 = points[:, :, Tr.X:Tr.Y + 1].contiguous()
    yaw = points[:, :, Tr.YAW].contiguous()
    dl = torch.linalg.norm(points[:, :, Tr.LEFT_BOUND_X:Tr.LEFT_BOUND_Y + 1] - P0, dim=2).contiguous()
    dr = (-torch.linalg.norm(points[:, :, Tr.RIGHT_BOUND_X:Tr.RIGHT_BOUND_Y + 1] - P0, dim=2)).contiguous()
    v = points[:, :, Tr.SPEED]
    v = torch.where(torch.isfinite(v) & (v > 0.0), v, torch.full_like(v, 10.0))
    X0 = torch.zeros((B, N, 5), dtype=torch.float64, device=points.device)
    X0[:, :, 0:2] = P0
    X0[:, :, 2] = _unwrap_torch(yaw)
    X0[:, :, 4] = v
    U0 = torch.zeros((B, N, 2), dtype=torch.float64, device=points.device)
    T0 = (torch.linalg.norm(torch.roll(P0, -1, dims=1) - P0, dim=2) / v).contiguous()
    finite = torch.isfinite(P0).all(dim=2) & torch.isfinite(yaw) & torch.isfinite(dl) & torch.isfinite(dr) & torch.isfinite(T0)
    usable = (finite & (dr < dl)).all(dim=1)
    return {"P0": P0, "yaw": yaw, "dl": dl, "dr": dr, "X0": X0, "U0": U0, "T0": T0, "usable": usable}


def bicycle_on_tables_torch(points, models, max_iter=200, tol=1e-6, check=False):
    """The time-optimal bicycle trajectory along each of B lines, as one chain on torch's current stream: points [B,N,19]
    (cuda tensor: B lines with their bounds, e.g. lap_times_torch(...)["points"] of a solved min-curvature batch) -> the
    solver's inputs and the centre-line guess (bicycle_inputs_from_tables_torch) -> ops.bicycle_solve_lines_torch.  models:
    one model dict or B of them -- the only host data of the call.  Returns dict(X [B,N,5], U [B,N,2], T [B,N], stats
    [B,12], lap [B] = T.sum(1), P0, yaw, dl, dr, usable [B] bool) of cuda tensors; a table of the result is
    ops.pose_tables_torch(track, POSE_GLOBAL, X, None, ...).
    An instance whose table is not usable (bicycle_inputs_from_tables_torch: a node with dr >= dl -- the line on or outside
    BOTH bounds there -- or a value that is not finite) is not a problem the solver can be given: it runs on a stand-in (a
    straight line with bounds of +-1 m, so that the device-pointer entry's "caller guarantees dr < dl" holds for the whole
    batch), and its X, U, T, lap come back NaN with stats[b, 5] = 2 (failed).  check=True reads `usable` on the host first (one
    synchronisation) and raises a ValueError naming the first such instance instead."""
    import torch
    inp = bicycle_inputs_from_tables_torch(points)
    ok = inp["usable"]
    if check and not bool(ok.all()):
        bad = torch.nonzero(~ok).flatten()
        raise ValueError(f"points: instance {int(bad[0])} (and {len(bad) - 1} more): a node with dr >= dl or a value that is not "
                         "finite; the lines need a margin to their bounds")
    B, N = int(points.shape[0]), int(points.shape[1])
    ramp = torch.arange(N, dtype=torch.float64, device=points.device)
    sP0 = torch.stack([ramp, torch.zeros_like(ramp)], dim=1)                       # stand-in: 1 m steps along x
    sel = lambda a, stand_in: torch.where(ok.reshape((B,) + (1,) * (a.dim() - 1)), a, stand_in).contiguous()  # noqa: E731
    P0, yaw = sel(inp["P0"], sP0[None]), sel(inp["yaw"], torch.zeros_like(ramp)[None])
    dl, dr = sel(inp["dl"], torch.ones_like(ramp)[None]), sel(inp["dr"], -torch.ones_like(ramp)[None])
    sX = torch.zeros((N, 5), dtype=torch.float64, device=points.device); sX[:, 0] = ramp; sX[:, 4] = 10.0
    X, U, T = sel(inp["X0"], sX[None]), inp["U0"], sel(inp["T0"], torch.full_like(ramp, 0.1)[None])
    stats = ops.bicycle_solve_lines_torch(models, P0, yaw, dl, dr, X, U, T, max_iter=max_iter, tol=tol)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=points.device)
    X, U, T = (torch.where(ok.reshape((B,) + (1,) * (a.dim() - 1)), a, nan) for a in (X, U, T))
    stats[:, 5] = torch.where(ok, stats[:, 5], torch.full_like(stats[:, 5], 2.0))
    return {"X": X, "U": U, "T": T, "stats": stats, "lap": T.sum(1), "P0": inp["P0"], "yaw": inp["yaw"], "dl": inp["dl"],
            "dr": inp["dr"], "usable": ok}


def signed_curvature(points):
    """Centre-line curvature with sign at the samples of a sampled table (the turn radius of column 5 is
    unsigned): heading change per arc length, central differences over the closed line."""
    pts = np.asarray(points, dtype=np.float64)
    yaw = np.unwrap(pts[:, 3])
    dyaw = np.roll(yaw, -1) - np.roll(yaw, 1)
    dyaw[0] += 2 * np.pi * round((yaw[-1] - yaw[0]) / (2 * np.pi)); dyaw[-1] += 2 * np.pi * round((yaw[-1] - yaw[0]) / (2 * np.pi))
    L = pts[0, 7] if pts[0, 7] > 0 else pts[-1, 6]
    ds = np.roll(pts[:, 6], -1) - np.roll(pts[:, 6], 1)
    ds[0] += L; ds[-1] += L
    return dyaw / ds


# ---------------------------------------------------------------- rank sharding
def shard_range(B, rank, world):
    """Contiguous block partition: rank r takes instances [lo, hi)."""
    base, rem = divmod(B, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class _Works:
    """wait() on every work handle of a grouped send / receive (what dist.gather's single handle offers)."""

    def __init__(self, works):
        self.works = list(works or [])

    def wait(self):
        for w in self.works:
            w.wait()
        return True


_gather_fallback = {"p2p": os.environ.get("RL_GATHER", "") == "p2p"}   # RL_GATHER=p2p forces the grouped send / receive


def _gather_p2p(pad, bufs, rank, world, dist, async_op):
    """The same collective as grouped point-to-point transfers ("ncclGather-equivalent via grouped
    ncclSend / ncclRecv"): rank 0 posts one receive per peer, every other rank one send, in ONE batch
    (dist.batch_isend_irecv = ncclGroupStart ... ncclGroupEnd on RCCL); rank 0's own shard is a local copy."""
    if rank == 0:
        bufs[0].copy_(pad)
        ops_ = [dist.P2POp(dist.irecv, bufs[r], r) for r in range(1, world)]
    else:
        ops_ = [dist.P2POp(dist.isend, pad, 0)]
    works = _Works(dist.batch_isend_irecv(ops_) if ops_ else [])
    if async_op:
        return works
    works.wait()
    return None


def gather_to_root(tensor, rank, world, dist, total=None, out=None, async_op=False, method="auto"):
    """The single collective of the path: every rank's result shard to rank 0 (RCCL `gather` over
    xGMI; gloo in the CPU tests).  `total` = global instance count when the shards come from
    shard_range(total, r, world) (they may then differ by one instance and are padded to the
    largest); None = every rank holds the same number of instances (weak scaling).
    `out` (rank 0, equal shards only): preallocated [world * B, ...] tensor the shards land in directly,
    no concatenation.  `async_op=True` returns the collective's work handle instead of the result: the
    gather then runs on the process group's own stream, ordered after what is already enqueued on the
    current stream, and overlaps with whatever the caller enqueues next (bench.py: the next launch).
    `method`: "gather" = dist.gather; "p2p" = the same transfer as one batch of grouped isend / irecv; "auto" =
    dist.gather, and from the first time the backend REFUSES it (NotImplementedError / "not supported": every rank is
    refused alike, before anything is sent) the grouped form for the rest of the process; any other exception is re-raised.
    RL_GATHER=p2p decides for the grouped form up front."""
    import torch
    if world == 1:
        return None if async_op else tensor
    if total is None:
        counts = [tensor.shape[0]] * world
    else:
        counts = [shard_range(total, r, world)[1] - shard_range(total, r, world)[0] for r in range(world)]
    mx = max(counts)
    pad = tensor
    if tensor.shape[0] < mx:
        pad = torch.cat([tensor, tensor.new_zeros((mx - tensor.shape[0],) + tuple(tensor.shape[1:]))])
    pad = pad.contiguous()
    bufs = None
    if rank == 0:
        if out is not None:
            assert total is None and out.shape[0] == world * mx and out.is_contiguous()
            bufs = list(out.view((world, mx) + tuple(tensor.shape[1:])).unbind(0))
        else:
            bufs = [torch.empty_like(pad) for _ in range(world)]
    use_p2p = method == "p2p" or (method == "auto" and _gather_fallback["p2p"])
    work = None
    if not use_p2p:
        try:
            work = dist.gather(pad, bufs, dst=0, async_op=async_op)
        except (RuntimeError, NotImplementedError) as e:
            # only a REFUSED collective switches forms: a backend that does not implement gather says so on every rank alike,
            # before anything is sent.  Any other failure (a shape error on one rank, out of memory, a communicator error)
            # is that rank's alone -- falling back there would leave it in send / receive while the others sit in gather.
            refused = isinstance(e, NotImplementedError) or any(
                w in str(e).lower() for w in ("not support", "unsupported", "not implemented", "no backend type"))
            if method != "auto" or not refused:
                raise
            print(f"gather_to_root: dist.gather raised on backend '{dist.get_backend()}' ({type(e).__name__}: {e}); "
                  f"using grouped isend / irecv from here on", flush=True)
            _gather_fallback["p2p"] = True
            use_p2p = True
    if use_p2p:
        work = _gather_p2p(pad, bufs, rank, world, dist, async_op)
    if async_op:
        return work
    if rank != 0:
        return None
    if out is not None:
        return out
    return torch.cat([b[:c] for b, c in zip(bufs, counts)])


# ---------------------------------------------------------------- synthetic oval (BASELINE config 3)
def oval_points(spacing=10.0, heading0=np.deg2rad(17.0)):
    """Centre line and half-widths of the synthetic Indy-style oval of SURVEY.md 8(d) config 3 (the
    reference ships no Indy data): two 1006 m straights, two 201 m short chutes, four 402 m
    quarter-turns (4023 m in all); half-width 7.6 m on the straights, 9.1 m in the turns.
    The front straight heads `heading0` off the x axis: the reference's constraints are axis-aligned
    boxes between the two bound points (optimizer.py:243-248), which collapse to zero width on an
    exactly axis-parallel straight and leave every QP there feasible or not by rounding noise.
    Returns (xy [P,2], half_width [P]) sampled every ~`spacing` metres, counter-clockwise."""
    R = 402.0 / (np.pi / 2.0)
    segs = [("s", 1006.0), ("t", 402.0), ("s", 201.0), ("t", 402.0),
            ("s", 1006.0), ("t", 402.0), ("s", 201.0), ("t", 402.0)]
    pos = np.array([0.0, 0.0]); heading = float(heading0)
    pts, hw = [], []
    for kind, length in segs:
        m = max(2, int(round(length / spacing)))
        for j in range(m):
            s = length * j / m
            if kind == "s":
                p = pos + s * np.array([np.cos(heading), np.sin(heading)])
                w = 7.6
            else:
                ang = s / R
                c = pos + R * np.array([-np.sin(heading), np.cos(heading)])      # centre of the left turn
                p = c + R * np.array([np.sin(heading + ang), -np.cos(heading + ang)])
                w = 9.1
            pts.append(p); hw.append(w)
        if kind == "s":
            pos = pos + length * np.array([np.cos(heading), np.sin(heading)])
        else:
            c = pos + R * np.array([-np.sin(heading), np.cos(heading)])
            heading += np.pi / 2.0
            pos = c + R * np.array([np.sin(heading), -np.cos(heading)])
    return np.array(pts), np.array(hw)


def oval_track_rows(bank_turn_deg=9.2, spacing=10.0):
    """The oval as 4-column track rows x,y,z,bank (BASELINE config 4): turns banked `bank_turn_deg`
    (Indianapolis: 9.2 degrees), straights flat, z = 0."""
    xy, hw = oval_points(spacing)
    bank = np.where(hw > 8.0, np.deg2rad(bank_turn_deg), 0.0)
    return np.column_stack([xy, np.zeros(len(xy)), bank])


def oval_centerline(s=100.0, k=5):
    xy, _ = oval_points()
    return BSplineTrajectory(xy, s, k)


def oval_half_widths(N):
    """Half-widths of the oval resampled on N uniform-in-parameter samples (nearest raw point)."""
    xy, hw = oval_points()
    idx = np.minimum((np.arange(N) * (len(hw) / N)).astype(int), len(hw) - 1)
    return hw[idx].copy(), hw[idx].copy()


def solve_grouped(groups, i_starts, search=_lib.SEARCH_WINDOWED):
    """Mixed batches (BASELINE config 3): instances are grouped by track so that every workgroup of
    one launch sees one knot layout.  groups = [(Track, widths [B_g,N,2]), ...], i_starts = one pinned
    start-index array per group (control-point counts differ between tracks).
    Returns a list of (ctrl, xy, n_success, status) per group, in order."""
    out = []
    for (trk, widths), ist in zip(groups, i_starts):
        ctrl, xy, ns, status, _ = ops.solve_batch_host(trk, _lib.BOUNDS_WIDTHS, widths, ist, search=search)
        out.append((ctrl, xy, ns, status))
    return out
