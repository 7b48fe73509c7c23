"""traj_opt_double_track: the minimum-lap-time problem of the double-track model, driven by `traj_opt_double_track.yaml` in
the working directory (entrypoints/traj_opt_double_track.py of the reference; min_time_optm/defaults.py holds the values of the
reference's example file).

Steps: RaceTrack from the three CSVs of the YAML (paths relative to the working directory) -> boundaries of the centre line ->
initial guess (the QSS simulator's speed profile from `estimates`, or the CasADi txt files named by `x0`, `u0`, `t0`) ->
set_up_double_track_problem and `opti.solve()` on the GPU.  A failed solve is reported and its last iterate used.  Writes the
TTL named by `output` and, in the working directory, ttl_input.txt, x_optm.txt, u_optm.txt, t_optm.txt and ttl_optm.txt.
The reference's plots are drawn only when matplotlib has an interactive backend, so a headless run never blocks."""
import os
import sys

import numpy as np
import yaml

from ..min_time_optm import min_time_optimizer as optm
from ..models.race_track import RaceTrack
from ..models.trajectory import Trajectory, save_ttl
from ..models.vehicle import Vehicle, VehicleParams
from ..simulator.simulator import Simulator
from ..utils.casadi_txt import read_txt, write_txt

PARAM_FILE = "traj_opt_double_track.yaml"
_NON_INTERACTIVE = {"agg", "cairo", "pdf", "pgf", "ps", "svg", "template"}


def _load_xy(path):
    return np.loadtxt(path, dtype=np.float64, delimiter=",", skiprows=1, usecols=(0, 1))


def _interactive_matplotlib():
    """pyplot, when it would open windows; else None."""
    if sys.platform.startswith("linux") and not (os.environ.get("DISPLAY") or os.environ.get("WAYLAND_DISPLAY")):
        return None
    try:
        import matplotlib
        backend = matplotlib.get_backend().lower()
    except Exception:
        return None
    if backend in _NON_INTERACTIVE or "inline" in backend:
        return None
    import matplotlib.pyplot as plt
    return plt


def _plot(plt, traj_d, opt_traj_d, x, u, t):
    plt.figure()
    plt.plot(opt_traj_d[:, 0], opt_traj_d[:, 1], "-o")
    plt.plot(traj_d[:, Trajectory.LEFT_BOUND_X], traj_d[:, Trajectory.LEFT_BOUND_Y])
    plt.plot(traj_d[:, Trajectory.RIGHT_BOUND_X], traj_d[:, Trajectory.RIGHT_BOUND_Y])
    plt.gca().set_aspect("equal")
    plt.show()
    for values, label in ((opt_traj_d[:, Trajectory.YAW], "Yaw"), (x[:, 5], "Velocity"), (t, "Time"),
                          (u[:, 0], "Drive Force"), (u[:, 1], "Brake Force"), (u[:, 2], "Steering Angle"),
                          (u[:, 3], "Load Transfer")):
        plt.figure()
        plt.plot(values, "-o" if label == "Yaw" else "-", label=label)
        plt.legend()
        plt.show()


def main():
    if not os.path.exists(PARAM_FILE):
        raise FileNotFoundError(f"{PARAM_FILE} does not exist.")
    with open(PARAM_FILE, "r") as f:
        params = yaml.safe_load(f)

    race_track = RaceTrack("Test track", _load_xy(params["left_boundary"]), _load_xy(params["right_boundary"]),
                           _load_xy(params["centerline"]), s=1.0, interval=params["interval"])
    traj_d = race_track.center_d.copy()
    race_track.fill_trajectory_boundaries(traj_d)

    if "x0" not in params:
        est = params["estimates"]
        vp = VehicleParams(np.array(est["acc_speed_loopup"]), np.array(est["dcc_speed_lookup"]), est["max_lon_acc_mpss"],
                           est["max_lon_dcc_mpss"], est["max_left_acc_mpss"], est["max_right_acc_mpss"],
                           est["max_speed_mps"], est["max_jerk_mpsc"])
        traj_d = Simulator(Vehicle(vp)).run_simulation(traj_d, False).trajectory
    else:
        for key in ("x0", "u0", "t0"):
            params[key] = read_txt(params[key])

    N = len(traj_d)
    params["N"] = N
    params["traj_d"] = traj_d
    params["race_track"] = race_track

    (X, U, T), (scale_x, scale_u, scale_t), opti = optm.set_up_double_track_problem(params)
    try:
        opti.solve()
    except Exception as e:
        print(e)
    st = opti.stats()
    print(f"[Solver: {st['return_status']} after {st['iter_count']} iterations]")

    x = opti.debug.value(X) * scale_x + np.hstack([race_track.abscissa[:, np.newaxis], np.zeros((N, 5))])
    u = opti.debug.value(U) * scale_u
    t = opti.debug.value(T) * scale_t

    print(f"[Optimal lap time: {float(np.sum(t)) * scale_t}]")

    write_txt("ttl_input.txt", traj_d.points[:, :Trajectory.TIME + 1])

    opt_traj_d = traj_d.copy()
    pose = np.asarray(race_track.frenet_to_global(x[:, 0], x[:, 1], x[:, 2]))
    opt_traj_d[:, 0:2] = pose[:, 0:2]
    opt_traj_d[:, Trajectory.YAW] = pose[:, 2]
    opt_traj_d[:, Trajectory.SPEED] = x[:, 5]
    race_track.fill_trajectory_boundaries(opt_traj_d)
    opt_traj_d.fill_distance()
    save_ttl(params["output"], opt_traj_d)
    write_txt("x_optm.txt", x)
    write_txt("u_optm.txt", u)
    write_txt("t_optm.txt", t)
    write_txt("ttl_optm.txt", opt_traj_d.points[:, :Trajectory.TIME + 1])

    plt = _interactive_matplotlib()
    if plt is not None:
        _plot(plt, traj_d, opt_traj_d, x, u, t)


if __name__ == "__main__":
    main()
