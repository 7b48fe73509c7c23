"""Host-side mirror of `spline_traj_optm.min_time_optm.min_time_optimizer`: `set_up_bicycle_problem` (:14-90, over
`BicycleProblem` and rl_bicycle_solve_batch; see that class) and `set_up_double_track_problem`
(min_time_optm/min_time_optimizer.py:93-163) and of the solve the reference's CLI performs on it
(entrypoints/traj_opt_double_track.py:24-86), with the GPU solver behind it.

The reference builds a casadi.Opti object and calls IPOPT.  `set_up_double_track_problem(params)` here takes the same
`params` dictionary (N, model, race_track, traj_d, average_track_width, speed_cap, max_iter, tol, verbose, optional
x0 / u0 / t0) and returns what the reference returns (:163):

    (X, U, T), (scale_x, scale_u, scale_t), opti

`X`, `U`, `T` are handles of the decision-variable blocks (N x 6, N x 4, N) in the reference's SCALED variables,
`scale_*` the scalings of :109-113, and `opti` a facade with the slice of casadi.Opti's surface the reference's
callers use (entrypoints/traj_opt_double_track.py:58-69, tests/test_min_time_optm.py): `solve()` (raises when the
solver does not reach its tolerance, like casadi), `value(v)`, `debug.value(v)` (the last iterate, also after a
failed solve), `set_initial(v, values)`, `solver(...)`, `stats()`.  So the CLI's

    x = opti.debug.value(X) * scale_x + np.hstack([race_track.abscissa[:, np.newaxis], np.zeros((N, 5))])
    u = opti.debug.value(U) * scale_u;   t = opti.debug.value(T) * scale_t

give the physical solution.  Underneath sits `DoubleTrackProblem` (`opti.problem`), whose `solve()` /
`solve_batch()` run rl_mintime_solve_batch (include/rl_mincurv.h) in physical units -- the batched entry the
reference has no counterpart for.

Deviations from the reference, all in one place:
  * solver: IPOPT is not part of the reference tree nor of this image; the solve is the build's own interior-point
    SQP-type method on the GPU (DESIGN_HISTORY.md 3d).  Its `tol` is an ABSOLUTE bound on the KKT residuals in the reference's
    scaling, whereas IPOPT's `tol` (yaml :8, 0.1) bounds its SCALED NLP error (residuals divided by multiplier-dependent
    factors s_d, s_c >= 1, and only reached after the barrier parameter has come down with it) -- handing 0.1 straight
    through stopped seconds of lap time short of the optimum while reporting success (round-3 advisor finding).  The
    facade therefore maps IPOPT-style tolerances onto the solver's scale: `effective_tol = min(tol, IPOPT_TOL_CAP)`
    (1e-4: measured on the example, the lap is then within 1e-3 s of the 1e-6 lap), warns when it does so, and reports
    `requested_tol`, `effective_tol` and the IPOPT options it has no counterpart for in `stats()`.
    `DoubleTrackProblem.solve(tol=...)` takes the solver's own tolerance unchanged (default 1e-6).
  * interpolants: `race_track.left_intp / right_intp / curvature_intp` are periodic cubic splines through the same
    samples (models/race_track.py), not CasADi's not-a-knot `bspline` interpolants on the padded table: the NLP's
    data agree with the reference's to interpolation accuracy, not bit for bit.
  * initial guess: `params["initial_guess"]` = "reference" (default) is :146-151 as written -- speed of the QSS
    table unfloored, controls (1, -1, 0.001, 0) in physical units, `T[i] = TIME[i]` unshifted; "clipped" is the
    build's variant (speed floored at 1.5 m/s so that v >= 1 holds strictly, the unused brake control at its
    optimum 0, TIME rolled by one sample because fill_time stores a segment's time on its END point, floor 1e-3 s).
    `u[1]` enters only the objective (its optimum is 0) and is eliminated by the solver either way.
"""
import warnings

import numpy as np

from .. import ops
from ..models.trajectory import Trajectory


def vehicle_margins(models, default=None):
    """margin_b = vehicle_width / 2 + safety_margin (:134) of B model dicts -> float64 [B].  Rows of an array carry no
    such keys: `default` (the margin of the problem's own model) for every instance then."""
    if len(models) > 0 and isinstance(models[0], dict):
        return np.array([m["vehicle_width"] / 2.0 + m["safety_margin"] for m in models], dtype=np.float64)
    if default is None:
        raise ValueError("models: an array has no vehicle_width / safety_margin; pass dicts or a margin")
    return np.full(len(models), float(default))


def fold_margins(left, right, margins):
    """The solver takes ONE margin per call; vehicles of different widths get theirs folded into their boundary distances:
    (left - m_b, right + m_b) [B,N], to be passed with margin = 0.  These are the sums the kernels form themselves
    (left - margin, right + margin), so the folded call sees the same doubles.  left / right [N] or [B,N], numpy arrays
    or torch tensors; margins [B] (numpy)."""
    m = np.asarray(margins, dtype=np.float64)
    if isinstance(left, np.ndarray):
        col = m[:, None]
    else:
        import torch
        col = torch.from_numpy(m).to(left.device)[:, None]
    if left.ndim == 1:
        left, right = left[None], right[None]
    if left.shape[0] not in (1, len(m)):
        raise ValueError(f"left / right: {left.shape[0]} instances for {len(m)} vehicles")
    return left - col, right + col


def _solver_margin(models, B, left, right, default):
    """(table [B,28], left, right, margin) of a vehicles call: one shared margin when all vehicles have the same, folded
    margins and 0 otherwise."""
    table = ops.dt_models_table(models, B)
    m = vehicle_margins(models, default)
    if np.all(m == m[0]):
        return table, left, right, float(m[0])
    left, right = fold_margins(left, right, m)
    return table, left, right, 0.0


class DoubleTrackProblem:
    def __init__(self, params):
        self.params = params
        self.model = dict(params["model"])
        rt = params["race_track"]
        traj_d = params["traj_d"]
        self.N = int(params.get("N", len(traj_d)))
        assert self.N == len(traj_d) == len(rt.abscissa)
        self.s = np.ascontiguousarray(rt.abscissa, dtype=np.float64)                       # S0, :105
        self.left = np.asarray(rt.left_intp(self.s), dtype=np.float64)                      # BoundL, :110
        self.right = np.asarray(rt.right_intp(self.s), dtype=np.float64)                    # BoundR, :111
        self.kappa = np.asarray(rt.curvature_intp(self.s), dtype=np.float64)                # :139
        self.track_length = float(rt.center_s.get_length())
        self.margin = self.model["vehicle_width"] / 2.0 + self.model["safety_margin"]        # :134
        bad = np.where(~(self.right + self.margin < self.left - self.margin))[0]
        assert len(bad) == 0, f"Track width must be wider than vehicle width plus 2 * safety margin at point {bad[0]}."
        self.average_track_width = float(params["average_track_width"])
        self.speed_cap = float(params["speed_cap"])
        pts = traj_d.points if isinstance(traj_d, Trajectory) else np.asarray(traj_d)
        if "x0" in params:                                                                  # :152-155
            self.X0 = np.array(params["x0"], dtype=np.float64).reshape(self.N, 6)
            self.U0 = np.array(params["u0"], dtype=np.float64).reshape(self.N, 4)
            self.T0 = np.array(params["t0"], dtype=np.float64).reshape(self.N)
        else:
            mode = params.get("initial_guess", "reference")
            assert mode in ("reference", "clipped"), mode
            self.X0 = np.zeros((self.N, 6)); self.X0[:, 0] = self.s
            if mode == "reference":                                                         # :146-151 as written
                self.X0[:, 5] = pts[:, Trajectory.SPEED]
                self.U0 = np.tile(np.array([1.0, -1.0, 0.001, 0.0]), (self.N, 1))
                self.T0 = pts[:, Trajectory.TIME].copy()
            else:
                self.X0[:, 5] = np.maximum(pts[:, Trajectory.SPEED], 1.5)                   # strictly inside v >= 1 (:188 of double_track.py)
                self.U0 = np.tile(np.array([1.0, 0.0, 0.001, 0.0]), (self.N, 1))            # u[1] is unused; its cost optimum is 0
                # TIME sits on the END point of each segment (Trajectory.fill_time); T[j] is the interval that STARTS at node j
                self.T0 = np.maximum(np.roll(pts[:, Trajectory.TIME], -1), 1e-3)
        # the reference's variable scaling (:109-113)
        self.scale_x = np.array([[1.0, self.average_track_width, 1.0, 1.0, 0.5, self.speed_cap]])
        self.scale_u = np.array([[self.model["Fd_max"], abs(self.model["Fb_max"]), self.model["delta_max"],
                                  self.model["mass"] * 50.0]])
        self.scale_t = 1.0
        self.x_offset = np.zeros((self.N, 6)); self.x_offset[:, 0] = self.s                 # X_OFFSET, :106

    def solve(self, max_iter=None, tol=None):
        """-> (X [N,6], U [N,4], T [N], stats [12]); stats as include/rl_mincurv.h: rl_mintime_solve_batch."""
        X, U, T, st = self.solve_batch(self.left[None], self.right[None], max_iter=max_iter, tol=tol)
        return X[0], U[0], T[0], st[0]

    def solve_batch(self, left, right, X0=None, U0=None, T0=None, max_iter=None, tol=None, models=None, tracks=None,
                    track_of=None):
        """B instances that differ in their boundary distances left/right [B,N] (and optionally in their initial
        guesses).  The reference's IPOPT tolerance `tol` (yaml :8) is a loose 0.1; the default here is 1e-6.
        models: None, or B model dicts (or an array [B, len(ops.DT_PARAMS)]): instance b is then solved for vehicle b
        (ops.mintime_solve_vehicles) instead of for the problem's own model; vehicles of different vehicle_width /
        safety_margin get their margins folded into left / right (fold_margins).  The initial guesses stay the problem's.
        tracks: None, or T centre lines of equal node count (ops.mintime_solve_tracks): DoubleTrackProblems, or dicts with
        "s", "kappa", "track_length" (or "L") and optionally "average_track_width", "speed_cap" (else this problem's);
        instance b runs on tracks[track_of[b]] (track_of None: T == B, instance b on track b).  left / right [B,N] are the
        distances from each instance's OWN centre line.  A guess that is not given is the instance's track's own, which
        only a DoubleTrackProblem has.  This problem supplies the model (unless models=) and the defaults of the scales."""
        left = np.ascontiguousarray(left, dtype=np.float64); right = np.ascontiguousarray(right, dtype=np.float64)
        B = left.shape[0]
        if tracks is None and track_of is not None:
            raise ValueError("track_of goes with tracks=")
        if tracks is not None:
            return self._solve_tracks(tracks, track_of, left, right, X0, U0, T0, max_iter, tol, models)
        rep = lambda a: np.repeat(np.asarray(a)[None], B, axis=0)  # noqa: E731
        X0 = rep(self.X0) if X0 is None else X0
        U0 = rep(self.U0) if U0 is None else U0
        T0 = rep(self.T0) if T0 is None else T0
        if models is not None:
            table, left, right, margin = _solver_margin(models, B, left, right, self.margin)
            return ops.mintime_solve_vehicles(table, self.s, self.kappa, np.ascontiguousarray(left), np.ascontiguousarray(right),
                                              margin, self.track_length, X0, U0, T0, self.average_track_width, self.speed_cap,
                                              max_iter=int(max_iter or self.params.get("max_iter", 200)),
                                              tol=float(tol if tol is not None else 1e-6))
        return ops.mintime_solve_batch(self.model, self.s, self.kappa, left, right, self.margin, self.track_length,
                                       X0, U0, T0, self.average_track_width, self.speed_cap,
                                       max_iter=int(max_iter or self.params.get("max_iter", 200)),
                                       tol=float(tol if tol is not None else 1e-6))


    def _solve_tracks(self, tracks, track_of, left, right, X0, U0, T0, max_iter, tol, models):
        B, nt = left.shape[0], len(tracks)
        get = lambda tr, key, alt=None: getattr(tr, key) if isinstance(tr, DoubleTrackProblem) else tr.get(key, alt)  # noqa: E731
        s = [np.asarray(get(tr, "s"), dtype=np.float64) for tr in tracks]
        counts = [len(a) for a in s]
        if len(set(counts)) != 1:
            raise ValueError(f"tracks: node counts differ: {counts}")
        length = [get(tr, "track_length", None if isinstance(tr, DoubleTrackProblem) else tr.get("L")) for tr in tracks]
        if any(v is None for v in length):
            raise ValueError(f"tracks: track {[v is None for v in length].index(True)}: no \"track_length\" (or \"L\")")
        atw = [get(tr, "average_track_width", self.average_track_width) for tr in tracks]
        cap = [get(tr, "speed_cap", self.speed_cap) for tr in tracks]
        track_of, length, atw, cap = ops.mintime_track_arrays(B, nt, track_of, length, atw, cap)
        of = np.arange(B) if track_of is None else track_of
        guess = []
        for name, given in (("X0", X0), ("U0", U0), ("T0", T0)):
            if given is None:
                if not all(isinstance(tracks[t], DoubleTrackProblem) for t in of):
                    raise ValueError(f"{name}: a track given as a dict has no initial guess of its own, pass {name}")
                given = np.stack([getattr(tracks[t], name) for t in of])
            guess.append(given)
        if models is None:
            table, margin = self.model, self.margin
        else:
            table, left, right, margin = _solver_margin(models, B, left, right, self.margin)
        return ops.mintime_solve_tracks(table, track_of, np.stack(s), np.stack([np.asarray(get(tr, "kappa"), dtype=np.float64) for tr in tracks]),
                                        np.ascontiguousarray(left), np.ascontiguousarray(right), margin, length, *guess, atw, cap,
                                        max_iter=int(max_iter or self.params.get("max_iter", 200)),
                                        tol=float(tol if tol is not None else 1e-6))


class OptiVariable:
    """Handle of one block of decision variables -- what `opti.variable(...)` returns in the reference (:101-103)."""

    def __init__(self, name, shape):
        self.name, self.shape = name, tuple(shape)

    def __repr__(self):
        return f"OptiVariable({self.name}, {self.shape})"


class OptiSolution:
    """What `opti.solve()` returns: `.value(v)` of the converged point, `.stats()`."""

    def __init__(self, values, stats):
        self._values, self._stats = values, stats

    def value(self, var):
        return self._values[var.name].copy()

    def stats(self):
        return dict(self._stats)


IPOPT_TOL_CAP = 1e-4   # the loosest absolute KKT tolerance an IPOPT-style `tol` is mapped to (module docstring)


class OptiFacade:
    """The slice of casadi.Opti the reference's callers of set_up_double_track_problem touch, over the GPU solve.
    All values are in the reference's SCALED variables (X * scale_x + X_OFFSET, U * scale_u, T * scale_t are physical)."""

    def __init__(self, problem, X, U, T):
        self.problem, self._vars = problem, {"X": X, "U": U, "T": T}
        p = problem
        self._values = {"X": (p.X0 - p.x_offset) / p.scale_x, "U": p.U0 / p.scale_u, "T": p.T0 / p.scale_t}
        self._stats = {"iter_count": 0, "return_status": "not solved", "success": False}
        self._max_iter = int(p.params.get("max_iter", 500))                                  # yaml :7; s_opts of :160
        self._tol = float(p.params.get("tol", 1e-6))
        self._ignored_opts = {}
        self.debug = self          # casadi: opti.debug.value(v) = the latest iterate, solved or not

    def effective_tol(self):
        """The absolute KKT tolerance handed to the GPU solver for the IPOPT-style tolerance set on this object."""
        return min(self._tol, IPOPT_TOL_CAP)

    def solver(self, name="ipopt", p_opts=None, s_opts=None):
        """casadi signature (:161); the plugin name is accepted and ignored -- the solver is the library's."""
        s_opts = s_opts or {}
        self._max_iter = int(s_opts.get("max_iter", self._max_iter))
        self._tol = float(s_opts.get("tol", self._tol))
        # IPOPT options without a counterpart in the library's solver (e.g. constr_viol_tol, the reference passes none
        # besides max_iter / tol, :158-160): kept and reported, never silently dropped
        self._ignored_opts = {k_: v for k_, v in s_opts.items() if k_ not in ("max_iter", "tol", "print_level")}

    def set_initial(self, var, value):
        v = np.asarray(value, dtype=np.float64)
        self._values[var.name] = np.broadcast_to(v.reshape(var.shape) if v.size == int(np.prod(var.shape)) else v,
                                                 var.shape).copy()

    def value(self, var):
        return self._values[var.name].copy()

    def stats(self):
        return dict(self._stats)

    def solve(self):
        p = self.problem
        X0 = self._values["X"] * p.scale_x + p.x_offset
        U0 = self._values["U"] * p.scale_u
        T0 = self._values["T"] * p.scale_t
        tol_eff = self.effective_tol()
        if tol_eff < self._tol:
            warnings.warn(f"IPOPT-style tol {self._tol:g} mapped to the GPU solver's absolute KKT tolerance {tol_eff:g} "
                          f"(min_time_optimizer.IPOPT_TOL_CAP); see stats()['effective_tol']", RuntimeWarning, stacklevel=2)
        if self._ignored_opts:
            warnings.warn(f"solver options without a counterpart in the GPU solver are ignored: {sorted(self._ignored_opts)}",
                          RuntimeWarning, stacklevel=2)
        X, U, T, st = p.solve_batch(p.left[None], p.right[None], X0[None], U0[None], T0[None],
                                    max_iter=self._max_iter, tol=tol_eff)
        self._values = {"X": (X[0] - p.x_offset) / p.scale_x, "U": U[0] / p.scale_u, "T": T[0] / p.scale_t}
        ok = st[0, 5] == 1.0
        self._stats = {"iter_count": int(st[0, 0]), "success": bool(ok),
                       "return_status": "Solve_Succeeded" if ok else
                       ("Maximum_Iterations_Exceeded" if st[0, 5] == 0.0 else "Solver_Failed"),
                       "dual_inf": float(st[0, 1]), "constr_viol": float(st[0, 2]), "compl": float(st[0, 3]),
                       "lap_time": float(st[0, 4]), "requested_tol": self._tol, "effective_tol": tol_eff,
                       "ignored_options": dict(self._ignored_opts), "raw": st[0].copy()}
        if not ok:   # casadi raises on anything but success; the iterate stays readable through opti.debug.value
            raise RuntimeError(f"Error in Opti::solve: solver returned '{self._stats['return_status']}' "
                               f"after {self._stats['iter_count']} iterations")
        return OptiSolution({k_: v.copy() for k_, v in self._values.items()}, self._stats)


def set_up_double_track_problem(params):
    """-> (X, U, T), (scale_x, scale_u, scale_t), opti   (min_time_optimizer.py:93-163, return at :163)."""
    prob = DoubleTrackProblem(params)
    X = OptiVariable("X", (prob.N, 6)); U = OptiVariable("U", (prob.N, 4)); T = OptiVariable("T", (prob.N,))
    opti = OptiFacade(prob, X, U, T)
    return (X, U, T), (prob.scale_x, prob.scale_u, prob.scale_t), opti


class BicycleProblem:
    """The NLP of the reference's set_up_bicycle_problem (min_time_optimizer.py:14-90) for the GPU solve
    (include/rl_mincurv.h: rl_bicycle_solve_batch), in physical units.  `params` is the reference's dictionary
    (N, traj_d, nu, nx, model, dynamics, x_l, x_u, u_l, u_u, verbose, max_iter, tol) plus the optional
    `initial_guess`: "reference" (default, :80-83 as written: the affine `set_initial` on x_i puts every node at the
    global origin with theta = yaw, v = 1, u = 0, T = 1) or "centerline" (on P0, theta = yaw, delta = 0, v = SPEED
    where filled else 10 m/s, T = segment length / v).  `dynamics` must be the bicycle model; its bound callables
    are called on the host and must describe what the kernels implement (x, y, theta free; symmetric steering and
    steering-rate bounds; v in [0, v_max])."""

    def __init__(self, params):
        from ..models import dynamic_bicycle as dyn
        self.params = params
        dynamics = params.get("dynamics", dyn.dynamics)
        if dynamics is not dyn.dynamics and getattr(dynamics, "__module__", "").split(".")[-1] != "dynamic_bicycle":
            raise ValueError("set_up_bicycle_problem: params['dynamics'] must be the bicycle model "
                             "(spline_traj_optm.models.dynamic_bicycle.dynamics); the GPU solver implements no other")
        model = dict(params["model"])
        lo_x = np.asarray(params.get("x_l", dyn.x_l)(model), dtype=np.float64).reshape(5)
        hi_x = np.asarray(params.get("x_u", dyn.x_u)(model), dtype=np.float64).reshape(5)
        lo_u = np.asarray(params.get("u_l", dyn.u_l)(model), dtype=np.float64).reshape(2)
        hi_u = np.asarray(params.get("u_u", dyn.u_u)(model), dtype=np.float64).reshape(2)
        if not (np.all(np.isneginf(lo_x[:3])) and np.all(np.isposinf(hi_x[:3])) and lo_x[3] == -hi_x[3] and lo_x[4] == 0.0
                and lo_u[1] == -hi_u[1] and np.all(np.isfinite([hi_x[3], hi_x[4], lo_u[0], hi_u[0], hi_u[1]]))):
            raise ValueError("set_up_bicycle_problem: the bound callables must leave x, y, theta free, bound delta and "
                             "delta_dot symmetrically and v to [0, v_max] (what rl_bicycle_solve_batch implements)")
        # the bounds the callables give take the place of the model's own keys
        self.model = dict(model, delta_max=float(hi_x[3]), v_max=float(hi_x[4]), a_lon_min=float(lo_u[0]),
                          a_lon_max=float(hi_u[0]), delta_dot_max=float(hi_u[1]))
        pts = params["traj_d"].points if isinstance(params["traj_d"], Trajectory) else np.asarray(params["traj_d"])
        self.N = int(params.get("N", len(pts)))
        assert self.N == len(pts)
        self.P0, self.yaw, self.left, self.right = self.table_data(pts)
        self.scale_x = np.array([[10.0, 10.0, 3.14, 0.1, 80.0]])                                              # :33-35
        self.scale_u = np.array([[20.0, 1.0]])
        self.scale_t = 1.0
        self.x_offset = np.zeros((self.N, 5)); self.x_offset[:, 0:2] = self.P0                                # X_OFFSET, :27
        mode = params.get("initial_guess", "reference")
        if mode not in ("reference", "centerline"):
            raise ValueError(f"initial_guess must be 'reference' or 'centerline', not {mode!r}")
        if mode == "reference":                                                                               # :80-83
            self.X0 = np.zeros((self.N, 5)); self.U0 = np.zeros((self.N, 2))
            self.X0[:, 2] = self.yaw
            self.X0[:, 4] = 1.0
            self.T0 = np.ones(self.N)
        else:
            self.X0, self.U0, self.T0 = self.centerline_guess(pts, self.P0, self.yaw)

    @staticmethod
    def table_data(pts):
        """(P0 [N,2], yaw [N], dl [N] > 0, dr [N] < 0) of one table [N,19]: the line and the distances to its bounds."""
        P0 = np.ascontiguousarray(pts[:, Trajectory.X:Trajectory.Y + 1], dtype=np.float64)                   # :26
        yaw = np.ascontiguousarray(pts[:, Trajectory.YAW], dtype=np.float64)                                  # :28
        bl = pts[:, Trajectory.LEFT_BOUND_X:Trajectory.LEFT_BOUND_Y + 1]                                      # :29-32
        br = pts[:, Trajectory.RIGHT_BOUND_X:Trajectory.RIGHT_BOUND_Y + 1]
        left = np.ascontiguousarray(np.linalg.norm(bl - P0, axis=1))                                          # dl, :66
        right = np.ascontiguousarray(-np.linalg.norm(br - P0, axis=1))                                        # dr, :67
        return P0, yaw, left, right

    @staticmethod
    def centerline_guess(pts, P0, yaw):
        """The "centerline" guess (X0 [N,5], U0 [N,2], T0 [N]) on one table's line."""
        N = len(pts)
        X0 = np.zeros((N, 5)); U0 = np.zeros((N, 2))
        v = pts[:, Trajectory.SPEED]
        v = np.where(np.isfinite(v) & (v > 0.0), v, 10.0)
        X0[:, 0:2] = P0
        X0[:, 2] = np.unwrap(yaw)
        X0[:, 4] = v
        T0 = np.linalg.norm(np.roll(P0, -1, axis=0) - P0, axis=1) / v
        return X0, U0, T0

    def solve(self, max_iter=None, tol=None):
        """-> (X [N,5], U [N,2], T [N], stats [12]); stats as include/rl_mincurv.h: rl_bicycle_solve_batch."""
        X, U, T, st = self.solve_batch(self.left[None], self.right[None], max_iter=max_iter, tol=tol)
        return X[0], U[0], T[0], st[0]

    def solve_batch(self, left, right, X0=None, U0=None, T0=None, max_iter=None, tol=None):
        """B instances that differ in their boundary distances left (dl > 0) / right (dr < 0) [B,N] (and optionally
        in their initial guesses).  Default tol 1e-6 (absolute, the solver's own scale)."""
        left = np.ascontiguousarray(left, dtype=np.float64); right = np.ascontiguousarray(right, dtype=np.float64)
        B = left.shape[0]
        rep = lambda a: np.repeat(np.asarray(a)[None], B, axis=0)  # noqa: E731
        X0 = rep(self.X0) if X0 is None else X0
        U0 = rep(self.U0) if U0 is None else U0
        T0 = rep(self.T0) if T0 is None else T0
        return ops.bicycle_solve_batch(self.model, self.P0, self.yaw, left, right, X0, U0, T0,
                                       max_iter=int(max_iter or self.params.get("max_iter", 200)),
                                       tol=float(tol if tol is not None else 1e-6))

    def tables_data(self, tables):
        """What solve_tables hands the solver for `tables` [B,N,19]: (P0 [B,N,2], yaw [B,N], dl [B,N], dr [B,N], X0 [B,N,5],
        U0 [B,N,2], T0 [B,N]), every row derived as a BicycleProblem built on that table derives its own."""
        tables = np.asarray(tables, dtype=np.float64)
        if tables.ndim != 3 or tables.shape[1] != self.N or tables.shape[2] != 19:
            raise ValueError(f"tables: expected [B,{self.N},19], got {tables.shape}")
        rows = [self.table_data(pts) for pts in tables]
        guess = [self.centerline_guess(pts, r[0], r[1]) for pts, r in zip(tables, rows)]
        return tuple(np.stack(a) for a in zip(*rows)) + tuple(np.stack(a) for a in zip(*guess))

    def solve_tables(self, tables, models=None, X0=None, U0=None, T0=None, max_iter=None, tol=None):
        """One line per instance (ops.bicycle_solve_lines): `tables` [B,N,19] are B lines with their bounds, e.g. the
        tables of a solved min-curvature batch; instance b is the problem a BicycleProblem built on tables[b] would solve,
        from its "centerline" guess unless X0 [B,N,5], U0 [B,N,2], T0 [B,N] are given.  models: None (this problem's model for
        all), one model dict, or B of them.  -> (X [B,N,5], U [B,N,2], T [B,N], stats [B,12])."""
        P0, yaw, dl, dr, Xc, Uc, Tc = self.tables_data(tables)
        return ops.bicycle_solve_lines(self.model if models is None else models, P0, yaw, dl, dr,
                                       Xc if X0 is None else X0, Uc if U0 is None else U0, Tc if T0 is None else T0,
                                       max_iter=int(max_iter or self.params.get("max_iter", 200)),
                                       tol=float(tol if tol is not None else 1e-6))


def set_up_bicycle_problem(params):
    """-> X, U, T, opti   (min_time_optimizer.py:14-90, return at :90).  X (N x 5), U (N x 2), T (N) are handles in
    the reference's SCALED variables: X * scale_x + X_OFFSET, U * scale_u and T are physical (scale_x = (10, 10, 3.14,
    0.1, 80), scale_u = (20, 1), X_OFFSET = (traj_d[:, X:Y+1], 0, 0, 0)).  `opti` is the same facade as
    set_up_double_track_problem's, over BicycleProblem (`opti.problem`)."""
    prob = BicycleProblem(params)
    X = OptiVariable("X", (prob.N, 5)); U = OptiVariable("U", (prob.N, 2)); T = OptiVariable("T", (prob.N,))
    opti = OptiFacade(prob, X, U, T)
    return X, U, T, opti


def optimise_track(race_track, vehicle, model, average_track_width=7.0, speed_cap=30.0, max_iter=200, tol=1e-6):
    """The reference CLI's pipeline (entrypoints/traj_opt_double_track.py:24-86) as a function: centre-line table
    with bounds -> QSS warm start (Simulator, k_qss_sim) -> NLP solve (k_mt_*) -> optimised Trajectory table with
    X, Y, YAW, SPEED, bounds and distances filled, ready for save_ttl.  Returns (Trajectory, X, U, T, stats)."""
    from ..simulator.simulator import Simulator
    traj_d = race_track.center_d.copy()
    race_track.fill_trajectory_boundaries(traj_d)
    traj_d = Simulator(vehicle).run_simulation(traj_d, False).trajectory                    # :35-49
    prob = DoubleTrackProblem({"N": len(traj_d), "model": model, "race_track": race_track, "traj_d": traj_d,
                               "average_track_width": average_track_width, "speed_cap": speed_cap, "max_iter": max_iter})
    X, U, T, st = prob.solve(tol=tol)
    return pose_table(race_track, traj_d, X), X, U, T, st


def pose_table(race_track, traj_d, X):
    """The CLI's last step (entrypoints/traj_opt_double_track.py:75-82) for one solution X [N,6] on the host: a copy of
    `traj_d` with the global poses, the speed, the bounds and the distances of the optimised line."""
    out = traj_d.copy()
    pose = race_track.frenet_to_global(X[:, 0], X[:, 1], X[:, 2])                           # :76
    out[:, 0:2] = pose[:, 0:2]
    out[:, Trajectory.YAW] = pose[:, 2]
    out[:, Trajectory.SPEED] = X[:, 5]
    race_track.fill_trajectory_boundaries(out)
    out.fill_distance()                                                                     # :81
    return out


def optimise_track_batch(race_track, vehicle, model, left=None, right=None, average_track_width=7.0, speed_cap=30.0,
                         max_iter=200, tol=1e-6, device=None, track=None, start_points=None, models=None, vehicles=None):
    """optimise_track for B instances of one track that differ in their boundary distances, as ONE chain on torch's current
    stream with device tensors throughout: QSS warm start (k_qss_sim) -> initial guess -> NLP solve (k_mt_*) -> tables of
    the batch (k_pose_tables) -> their summary (k_table_summary).  No result travels to the host in between; the host set-up is
    the interpolants' values at the nodes (scipy, as in DoubleTrackProblem) and the rl_track of the centre line.
    left / right [B,N] (numpy or cuda tensors): the distances from the centre line to the left (> 0) and right (< 0) edge at
    the nodes, as DoubleTrackProblem.solve_batch takes them; an instance's rings are then the polygons through those edge
    points on the centre line's normals (BOUNDS_POINTS).  None: one instance with the track's own distances, bounded by
    race_track's own rings -- optimise_track's result.
    track: the _lib.Track of race_track.center_s with len(race_track.center_d) samples (batch.make_track) that the tables
    step runs on; None builds one (device allocations and table kernels: set-up, not part of the chain).  A track that is
    destroyed frees device memory, which waits for the device: the one used is therefore returned under "track", and the
    chain stays asynchronous for as long as the caller holds the result; pass it back in for the next call.
    start_points: None, or [B,P,19] simulated tables of B lines in global coordinates (numpy or cuda tensors), e.g.
    batch.lap_times_torch(...)["points"] of a min-curvature batch on the same track: instance b then starts from line b
    projected onto the centre line (batch.min_time_guess_from_lines_torch) instead of from the centre line, and the result
    gains "start_status" (int32 [B]: 0 = started from its line, otherwise from the centre line, see that function).
    models: None, or B model dicts: instance b is solved for vehicle b (ops.mintime_solve_vehicles_torch) and `model` is not
    read.  B must agree with left / right when those are given; otherwise the track's own distances are repeated B times.
    Vehicles of different vehicle_width / safety_margin get their margins folded into the distances the solver sees
    (fold_margins); the tables keep the distances as given.
    vehicles: None, or B QSS vehicles (Vehicles or 5-tuples, batch.vehicle_tables_batch), with `models` only: the warm start is
    then one QSS run per instance (ops.qss_sim_vehicles_torch), `base` is [B,N,19] and `vehicle` is not read.
    Returns dict(points [B,N,19], X [B,N,6], U [B,N,4], T [B,N], stats [B,12], summary [B,8]) of cuda tensors plus "track":
    stats as include/rl_mincurv.h: rl_mintime_solve_batch, summary in the order of ops.SUMMARY_COLUMNS (summary[:, 0] is the
    lap time)."""
    import torch
    from .. import _lib, batch
    from ..models.trajectory import _ring_coords
    if vehicles is not None and models is None:
        raise ValueError("vehicles: one QSS vehicle per instance goes with models=, one NLP model per instance")
    if vehicles is not None and start_points is not None:
        raise ValueError("start_points with vehicles=: the guess from lines takes one centre-line table, not one per instance")
    if models is not None:
        ops.dt_models_table(models)   # a bad row is refused before anything is set up
    dev = torch.device("cuda", _lib.Context.get(device).device)
    up = lambda a: a.to(dev).contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    if (left is None) != (right is None):
        raise ValueError("left and right: both or neither")
    traj_d = race_track.center_d.copy()
    race_track.fill_trajectory_boundaries(traj_d)
    N = len(traj_d)
    s = np.ascontiguousarray(race_track.abscissa, dtype=np.float64)
    if left is None:
        left_d, right_d = up(np.asarray(race_track.left_intp(s))[None]), up(np.asarray(race_track.right_intp(s))[None])
        if models is not None:
            left_d, right_d = left_d.repeat(len(models), 1), right_d.repeat(len(models), 1)
    else:
        left_d, right_d = up(left), up(right)
    B = int(left_d.shape[0])
    if tuple(left_d.shape) != (B, N) or tuple(right_d.shape) != (B, N):
        raise ValueError(f"left / right: expected [B,{N}]")
    if models is None:
        margin = model["vehicle_width"] / 2.0 + model["safety_margin"]
    else:
        if len(models) != B:
            raise ValueError(f"models: {len(models)} vehicles for {B} instances of left / right")
        table, left_s, right_s, margin = _solver_margin(models, B, left_d, right_d, None)
        left_s, right_s = left_s.contiguous(), right_s.contiguous()
    if vehicles is None:
        # QSS warm start: the simulated centre-line table is the same for every instance
        base = up(traj_d.points)[None].contiguous()
        ops.qss_sim_torch(base, *batch.vehicle_tables(vehicle))
        base = base[0]
    else:
        veh = batch._vehicles_stacked(vehicles, B, dev)
        base = up(traj_d.points)[None].repeat(B, 1, 1).contiguous()
        ops.qss_sim_vehicles_torch(base, *veh)
    # initial guess (min_time_optimizer.py:146-151 as written; DoubleTrackProblem's "reference" mode)
    s_d = up(s)
    kappa_d = up(race_track.curvature_intp(s))
    pieces = tuple(up(a) for a in race_track.centerline_pieces())
    start_status = None
    if start_points is None:
        X, U, T = batch.min_time_centerline_guess_torch(s_d, base, B)
    else:
        start_d = up(start_points)
        if start_d.ndim != 3 or int(start_d.shape[0]) != B or int(start_d.shape[2]) != 19:
            raise ValueError(f"start_points: expected [{B},P,19]")
        X, U, T, start_status = batch.min_time_guess_from_lines_torch(race_track, start_d, s_d, kappa_d, base, pieces=pieces)
    if models is None:
        stats = ops.mintime_solve_torch(dict(model), s_d, kappa_d, left_d, right_d, margin,
                                        float(race_track.center_s.get_length()), X, U, T, float(average_track_width),
                                        float(speed_cap), max_iter=int(max_iter), tol=float(tol))
    else:
        stats = ops.mintime_solve_vehicles_torch(table, s_d, kappa_d, left_s, right_s, margin,
                                                 float(race_track.center_s.get_length()), X, U, T, float(average_track_width),
                                                 float(speed_cap), max_iter=int(max_iter), tol=float(tol))
    if track is None:
        track = batch.make_track(race_track.center_s, N, device=dev.index)
    elif track.N != N:
        raise ValueError(f"track: {track.N} samples, the race track has {N} nodes")
    if left is None:
        track.set_rings(_ring_coords(race_track.left_r), _ring_coords(race_track.right_r))
        form, bounds = _lib.BOUNDS_SHARED_RINGS, None
    else:
        yaw0 = up(race_track.yaw_intp(s))
        cx, cy, nx, ny = up(race_track.x_intp(s)), up(race_track.y_intp(s)), -torch.sin(yaw0), torch.cos(yaw0)
        bounds = torch.stack([cx + nx * left_d, cy + ny * left_d, cx + nx * right_d, cy + ny * right_d], dim=2).contiguous()
        form = _lib.BOUNDS_POINTS
    points = batch.min_time_tables_torch(race_track, track, X, T, form, bounds, base=base, pieces=pieces)
    summary = ops.table_summary_torch(points)
    out = {"points": points, "X": X, "U": U, "T": T, "stats": stats, "summary": summary, "track": track}
    if start_status is not None:
        out["start_status"] = start_status
    return out


def optimise_tracks_batch(race_tracks, vehicle, model, models=None, vehicles=None, track_of=None, average_track_width=7.0,
                          speed_cap=30.0, max_iter=200, tol=1e-6, device=None, tracks=None, start_points=None):
    """optimise_track_batch for T race tracks of EQUAL node count in one chain on torch's current stream: per track the QSS
    warm start and the initial guess, then ONE solve for all instances (ops.mintime_solve_tracks_torch), then per track the
    tables of its instances (ops.pose_tables_batch_*, on the track's contiguous slice) and the summary of all.
    Instances are ordered TRACK-MAJOR.  models / vehicles None: one instance per track with `model` / `vehicle`.  models: V
    model dicts -> T x V instances, instance t V + v = vehicle v on track t (vehicles: V QSS vehicles for the warm starts, as
    in optimise_track_batch).  track_of: None, or B non-decreasing track indices, with models (and vehicles) of length B:
    instance b = models[b] on race_tracks[track_of[b]], every track at least once.  The distances are each track's own;
    vehicles of different vehicle_width / safety_margin get their margins folded in (fold_margins).  average_track_width,
    speed_cap: one value, or T of them.  tracks: None, or the T _lib.Tracks of an earlier call's result.
    Returns the dict of optimise_track_batch with "track_of" (int32 [B], numpy) and "tracks" (list of T) in place of "track"."""
    import torch
    from .. import _lib, batch
    from ..models.trajectory import _ring_coords
    if start_points is not None:
        raise ValueError("start_points with several tracks: the guess from lines takes one centre-line table, not one per track")
    if vehicles is not None and models is None:
        raise ValueError("vehicles: one QSS vehicle per instance goes with models=, one NLP model per instance")
    nt = len(race_tracks)
    if nt == 0:
        raise ValueError("race_tracks: at least one track")
    counts = [len(rt.center_d) for rt in race_tracks]
    if len(set(counts)) != 1:
        raise ValueError(f"race_tracks: node counts differ: {counts} (models.race_track.race_track_with_nodes builds a track with a given count)")
    N = counts[0]
    if models is not None:
        ops.dt_models_table(models)   # a bad row is refused before anything is set up
    if track_of is None:
        nv = 1 if models is None else len(models)
        track_of = np.repeat(np.arange(nt, dtype=np.int32), nv)
        inst_models = None if models is None else [models[b % nv] for b in range(nt * nv)]
        inst_vehicles = None if vehicles is None else [vehicles[b % nv] for b in range(nt * nv)]
        if vehicles is not None and len(vehicles) != nv:
            raise ValueError(f"vehicles: {len(vehicles)} QSS vehicles for {nv} models")
    else:
        if models is None:
            raise ValueError("track_of: goes with models=, one per instance")
        track_of = np.asarray(track_of)
        if track_of.shape != (len(models),) or (vehicles is not None and len(vehicles) != len(models)):
            raise ValueError(f"track_of: {track_of.shape} for {len(models)} models")
        if np.any(np.diff(track_of) < 0) or sorted(set(track_of.tolist())) != list(range(nt)):
            raise ValueError("track_of: track-major order, non-decreasing, every track at least once")
        track_of = track_of.astype(np.int32)
        inst_models, inst_vehicles = models, vehicles
    B = len(track_of)
    lengths = [float(rt.center_s.get_length()) for rt in race_tracks]
    track_of, lengths, atw, cap = ops.mintime_track_arrays(B, nt, track_of, lengths, average_track_width, speed_cap)
    dev = torch.device("cuda", _lib.Context.get(device).device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    slices = [slice(int(np.searchsorted(track_of, t, "left")), int(np.searchsorted(track_of, t, "right"))) for t in range(nt)]
    s_h = [np.ascontiguousarray(rt.abscissa, dtype=np.float64) for rt in race_tracks]
    s_d = up(np.stack(s_h))
    kappa_d = up(np.stack([rt.curvature_intp(s) for rt, s in zip(race_tracks, s_h)]))
    left_d = up(np.stack([np.asarray(race_tracks[t].left_intp(s_h[t])) for t in track_of]))
    right_d = up(np.stack([np.asarray(race_tracks[t].right_intp(s_h[t])) for t in track_of]))
    if inst_models is None:
        table, left_s, right_s, margin = dict(model), left_d, right_d, model["vehicle_width"] / 2.0 + model["safety_margin"]
    else:
        table, left_s, right_s, margin = _solver_margin(inst_models, B, left_d, right_d, None)
        left_s, right_s = left_s.contiguous(), right_s.contiguous()
    X = torch.empty((B, N, 6), dtype=torch.float64, device=dev)
    U = torch.empty((B, N, 4), dtype=torch.float64, device=dev)
    T = torch.empty((B, N), dtype=torch.float64, device=dev)
    bases, pieces = [], []
    for t, rt in enumerate(race_tracks):
        sl = slices[t]
        nb = sl.stop - sl.start
        traj_d = rt.center_d.copy()
        rt.fill_trajectory_boundaries(traj_d)
        if inst_vehicles is None:
            base = up(traj_d.points)[None].contiguous()
            ops.qss_sim_torch(base, *batch.vehicle_tables(vehicle))
            base = base[0]
        else:
            base = up(traj_d.points)[None].repeat(nb, 1, 1).contiguous()
            ops.qss_sim_vehicles_torch(base, *batch._vehicles_stacked(inst_vehicles[sl], nb, dev))
        X[sl], U[sl], T[sl] = batch.min_time_centerline_guess_torch(s_d[t], base, nb)
        bases.append(base)
        pieces.append(tuple(up(a) for a in rt.centerline_pieces()))
    stats = ops.mintime_solve_tracks_torch(table, track_of, s_d, kappa_d, left_s, right_s, margin, lengths, X, U, T, atw, cap,
                                           max_iter=int(max_iter), tol=float(tol))
    if tracks is None:
        tracks = [batch.make_track(rt.center_s, N, device=dev.index) for rt in race_tracks]
    elif len(tracks) != nt or any(trk.N != N for trk in tracks):
        raise ValueError(f"tracks: expected {nt} tracks of {N} samples")
    points = torch.empty((B, N, 19), dtype=torch.float64, device=dev)
    for t, rt in enumerate(race_tracks):
        sl = slices[t]
        tracks[t].set_rings(_ring_coords(rt.left_r), _ring_coords(rt.right_r))
        points[sl] = batch.min_time_tables_torch(rt, tracks[t], X[sl], T[sl], _lib.BOUNDS_SHARED_RINGS, None, base=bases[t],
                                                 pieces=pieces[t])
    summary = ops.table_summary_torch(points)
    return {"points": points, "X": X, "U": U, "T": T, "stats": stats, "summary": summary, "tracks": tracks, "track_of": track_of}
