#!/usr/bin/env python3
"""Timing of the batched global -> Frenet projection (include/rl_mincurv.h: rl_frenet_batch_dev, kernel k_frenet) and of the
resample behind it, and what a warm start from min-curvature lines does to the min-time solve.  ONE run on one MI355X:
  * the 1024 x 2000 points of the benchmarked sweep batch (bench.py's headline: width-perturbed Monza instances, N = 2000,
    max_iter = 5) projected onto the centre line of RaceTrack("Monza", interval 5 m) (M = 1158 pieces): device time from events,
    the median of --repeats single launches, for both searches ("frenet_search" 1 and 0), and whether their results are
    identical; min g and max |n| over the batch;
  * k_frenet_resample of the projected batch (SPEED channel) at the track's own nodes;
  * the route it replaces: the vectorised numpy twin (tests/frenet_twin.py) on the host for the same points, wall time of
    --baseline-instances instances scaled to B, and the largest difference between the two results on those instances;
  * a small Monza batch (--nlp-interval, B = 2) through optimise_track_batch from the centre line and from the simulated tables
    of the sweep's lines (start_points): interior-point iterations and lap times of both.
The kernels' registers and scratch come from profiles/frenet/kernel_resources_before_after.json.  Prints one JSON line and
writes it to --out.

    python tools/time_frenet.py [--out profiles/frenet/time_frenet.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def launch_ms(fn, repeats, warmup=3):
    """(median, min, max) of single launches, device time in ms."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frenet", "time_frenet.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--max-iter", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--baseline-instances", type=int, default=2)
    ap.add_argument("--nlp-interval", type=float, default=10.0)
    ap.add_argument("--skip-nlp", action="store_true")
    a = ap.parse_args()
    import torch
    import frenet_twin as ft
    from spline_trajectory_optimization_amd import _lib, batch, ops
    from spline_trajectory_optimization_amd.min_time_optm import defaults
    from spline_trajectory_optimization_amd.min_time_optm.min_time_optimizer import optimise_track_batch
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    centre, left, right = batch.load_monza()
    line = batch.monza_centerline(100.0, 5)
    t, cx, cy, k = line._tck()
    N, B = a.N, a.B
    rt = RaceTrack("Monza", left, right, centre, s=10.0, interval=5.0)
    traj = line.sample_along(ts=np.linspace(0.0, 1.0, N, endpoint=False))
    rt.fill_trajectory_boundaries(traj)
    wl, wr = batch.half_widths_from_bounds(traj.points)
    widths = np.ascontiguousarray(batch.width_batch(wl, wr, B, seed=1234))
    trk = batch.make_track(line, N)
    dev = torch.device("cuda", 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    widths_d = up(widths)
    solved = ops.solve_batch_torch(trk, _lib.BOUNDS_WIDTHS, widths_d, batch.default_i_start(len(cx), k, a.max_iter, seed=0))
    xy = solved["xy"]
    pieces_h = rt.centerline_pieces()
    pieces = tuple(up(v) for v in pieces_h)
    M, L = len(pieces_h[0]) - 1, float(pieces_h[0][-1])
    ctx = _lib.Context.get(0)
    res = {"B": B, "P": N, "M": M, "track_length_m": L, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "points": f"xy of the benchmarked batch (Monza, N = {N}, max_iter = {a.max_iter}, widths seed 1234) onto the centre "
                     f"line of RaceTrack('Monza', s=10, interval=5)",
           "dynamic_lds_bytes": 3 * ((M * 8 + 15) & ~15) + 6144}
    outs = {}
    for search in (1, 0):
        ctx.set_option("frenet_search", search)
        out = ops.frenet_torch(pieces, xy)
        res[f"frenet_search_{search}_ms"] = launch_ms(lambda: ops.frenet_torch(pieces, xy, out=out), a.repeats)
        outs[search] = tuple(v.clone() for v in out)
    ctx.set_option("frenet_search", 1)
    res["searches_identical"] = all(bool(torch.equal(p, q) or torch.equal(torch.nan_to_num(p), torch.nan_to_num(q)))
                                    for p, q in zip(outs[0], outs[1]))
    fr, status, stats = (v.cpu().numpy() for v in outs[1])
    res["status_counts"] = {str(int(s_)): int((status == s_).sum()) for s_ in np.unique(status)}
    res["min_g"], res["max_abs_n_m"], res["max_evaluations"] = float(stats[:, 1].min()), float(stats[:, 2].max()), int(stats[:, 3].max())
    res["bytes_moved_min"] = int(B * N * (2 + 4 + 0.5) * 8)
    nodes = up(rt.abscissa)
    speed = torch.full((B, N, 1), 10.0, dtype=torch.float64, device=dev)
    rout = ops.frenet_resample_torch(outs[1][0], speed, nodes, L)
    res["resample_ms"] = launch_ms(lambda: ops.frenet_resample_torch(outs[1][0], speed, nodes, L, out=rout), a.repeats)
    res["resample_status_counts"] = {str(int(s_)): int((rout[1] == s_).sum()) for s_ in torch.unique(rout[1]).cpu().numpy()}
    # the host route: the numpy twin on the same points
    xy_h = xy[:a.baseline_instances].cpu().numpy()
    t0 = time.perf_counter()
    ref, gap = ft.project_batch(pieces_h, xy_h)
    wall = (time.perf_counter() - t0) / len(xy_h) * 1e3
    nb = len(xy_h)
    res["baseline_numpy_twin_host"] = {
        "instances_timed": nb, "wall_ms_per_instance": wall, "wall_ms_scaled_to_B": wall * B,
        "max_abs_difference": {"s_m": float(ft.cyclic(fr[:nb, :, 0], ref[..., 0], L).max()),
                               "n_m": float(np.abs(fr[:nb, :, 1] - ref[..., 1]).max()),
                               "g": float(np.abs(fr[:nb, :, 3] - ref[..., 3]).max())},
        "min_gap_best_to_second_best_m": float(gap.min())}
    res["speedup_vs_host_twin"] = wall * B / res["frenet_search_1_ms"]["median"]
    kr = os.path.join(ROOT, "profiles", "frenet", "kernel_resources_before_after.json")
    if os.path.exists(kr):
        after = json.load(open(kr))["after"]
        res["kernels"] = {q: after[q] for q in after if "k_frenet" in q}
    if not a.skip_nlp:
        est = defaults.ESTIMATES
        veh = Vehicle(VehicleParams(np.array(est["acc_speed_loopup"]), np.array(est["dcc_speed_lookup"]), est["max_lon_acc_mpss"],
                                    est["max_lon_dcc_mpss"], est["max_left_acc_mpss"], est["max_right_acc_mpss"],
                                    est["max_speed_mps"], est["max_jerk_mpsc"]))
        Bn = 2
        laps = batch.lap_times_torch(trk, solved["ctrl"][:Bn].contiguous(), _lib.BOUNDS_WIDTHS, widths_d[:Bn].contiguous(),
                                     line.get_length(), veh)
        rt2 = RaceTrack("Monza", left, right, centre, s=10.0, interval=a.nlp_interval)
        s2 = rt2.abscissa
        sc = np.array([1.0, 0.95])
        lft = np.ascontiguousarray(rt2.left_intp(s2)[None] * sc[:, None]); rgt = np.ascontiguousarray(rt2.right_intp(s2)[None] * sc[:, None])
        kw = dict(average_track_width=10.0, speed_cap=defaults.SOLVER["speed_cap"], max_iter=400, tol=1e-6)
        cold = optimise_track_batch(rt2, veh, defaults.MODEL, lft, rgt, **kw)
        warm = optimise_track_batch(rt2, veh, defaults.MODEL, lft, rgt, track=cold["track"], start_points=laps["points"], **kw)
        torch.cuda.synchronize()
        cs, ws = cold["stats"].cpu().numpy(), warm["stats"].cpu().numpy()
        res["warm_start"] = {
            "track": f"Monza, nodes every {a.nlp_interval} m (N = {len(s2)}), B = {Bn}, boundary distances x {sc.tolist()}",
            "start_lines": "the first two lines of the sweep batch above, simulated (batch.lap_times_torch)",
            "sweep_lap_times_s": laps["summary"][:, 0].cpu().numpy().tolist(),
            "start_status": warm["start_status"].cpu().numpy().tolist(),
            "from_centre_line": {"iterations": cs[:, 0].tolist(), "solver_status": cs[:, 5].tolist(), "lap_times_s": cs[:, 4].tolist()},
            "from_lines": {"iterations": ws[:, 0].tolist(), "solver_status": ws[:, 5].tolist(), "lap_times_s": ws[:, 4].tolist()},
            "iterations_saved": (cs[:, 0] - ws[:, 0]).tolist()}
    line_ = json.dumps(res)
    print(line_)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
