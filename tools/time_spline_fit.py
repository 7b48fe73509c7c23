#!/usr/bin/env python3
"""Timing of the batched periodic spline fit (include/rl_mincurv.h: rl_spline_fit_batch_dev, kernel k_spline_fit<5>): the
P = 2000 samples of every line the benchmarked batch returns (bench.py's headline: 1024 width-perturbed Monza instances,
N = 2000, max_iter = 5) fitted back onto the centre line's knots (61 unknowns per coordinate), parameters u_p = p / P.
ONE run on one MI355X, warm-up first:
  * rl_spline_fit_batch_dev, device time from events: the median of --repeats single launches, and --repeats launches back to
    back between one pair of events;
  * the same with chord-length parameters computed in the kernel (u = NULL);
  * the route it replaces: scipy.interpolate.splprep(task=-1, per=True) on the same knots, one host call per instance, wall
    time of --baseline-instances, scaled to B; and the largest distance between the two results on those instances.
The kernel's registers and scratch come from profiles/start_lines/kernel_resources_before_after.json, its LDS from the carve
of csrc/rl_spline_fit.hpp (fit_lds_layout).  Prints one JSON line and writes it to --out.

    python tools/time_spline_fit.py [--out profiles/start_lines/time_spline_fit.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def launch_ms(fn, repeats, warmup=3):
    """(median, min, max of single launches, per launch of `repeats` launches back to back), device time in ms."""
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)),
            "back_to_back_per_launch": float(e0.elapsed_time(e1) / repeats)}


def fit_lds_bytes(k, m, P):
    """csrc/rl_spline_fit.hpp: fit_lds_layout(k, m, P).total_bytes."""
    Pp = (P + 3) & ~3
    nacc = (k + 1) * (k + 2) // 2 + 2 * (k + 1)
    doubles = Pp + m * nacc + m * (k + 1) + 2 * m + m * (k + 1) + m * (k + 2) + (25 + 10 + 2) + 2 * m + 2 * 256
    return (doubles * 8 + 2 * Pp * 2 + (m + 4) * 4 + 15) & ~15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "start_lines", "time_spline_fit.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--max-iter", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--baseline-instances", type=int, default=16)
    a = ap.parse_args()
    import torch
    from scipy import interpolate
    from spline_trajectory_optimization_amd import _lib, batch, ops
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack
    centre, left, right = batch.load_monza()
    line = batch.monza_centerline(100.0, 5)
    t, cx, cy, k = line._tck()
    N, B = a.N, a.B
    traj = line.sample_along(ts=np.linspace(0.0, 1.0, N, endpoint=False))
    RaceTrack("Monza", left, right, centre).fill_trajectory_boundaries(traj)
    wl, wr = batch.half_widths_from_bounds(traj.points)
    widths = np.ascontiguousarray(batch.width_batch(wl, wr, B, seed=1234))
    trk = batch.make_track(line, N)
    dev = torch.device("cuda", 0)
    solved = ops.solve_batch_torch(trk, _lib.BOUNDS_WIDTHS, torch.from_numpy(widths).to(dev),
                                   batch.default_i_start(len(cx), k, a.max_iter, seed=0))
    xy = solved["xy"]
    u = torch.arange(N, dtype=torch.float64, device=dev) / N
    out = (torch.empty((B, len(cx), 2), dtype=torch.float64, device=dev), torch.empty((B, 4), dtype=torch.float64, device=dev))
    res = {"B": B, "P": N, "unknowns_per_coordinate": len(cx) - k, "degree": k, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0),
           "points": f"xy of the benchmarked batch (Monza, N = {N}, max_iter = {a.max_iter}, widths seed 1234), u_p = p / P"}
    res["fit_given_u_ms"] = launch_ms(lambda: ops.spline_fit_torch(trk, xy, u, out=out), a.repeats)
    ctrl, stats = (v.cpu().numpy() for v in out)
    res["status_counts"] = {str(int(s)): int((stats[:, 0] == s).sum()) for s in np.unique(stats[:, 0])}
    res["rms_residual_m_max"] = float(np.nanmax(stats[:, 1]))
    res["pivot_ratio_min"] = float(stats[:, 3].min())
    res["distance_from_the_solved_control_points_m_max"] = float(np.abs(ctrl - solved["ctrl"].cpu().numpy()).max())
    res["fit_chord_length_ms"] = launch_ms(lambda: ops.spline_fit_torch(trk, xy, None, out=out), a.repeats)
    res["bytes_moved_min"] = int(B * (N * 2 + N + len(cx) * 2 + 4) * 8)
    # the host route: FITPACK on the same knots, one call per instance
    xy_h = xy[:a.baseline_instances].cpu().numpy()
    uu = np.concatenate([np.arange(N) / N, [1.0]])
    t0 = time.perf_counter()
    worst = 0.0
    for b in range(len(xy_h)):
        loop = np.vstack([xy_h[b], xy_h[b, :1]])
        (_, c, _), _ = interpolate.splprep([loop[:, 0], loop[:, 1]], u=uu, t=t, task=-1, per=True, k=k, quiet=1)
        worst = max(worst, float(np.abs(np.column_stack(c) - ctrl[b]).max()))
    wall = (time.perf_counter() - t0) / len(xy_h) * 1e3
    res["baseline_splprep_host"] = {"instances_timed": len(xy_h), "wall_ms_per_instance": wall, "wall_ms_scaled_to_B": wall * B,
                                    "max_abs_difference_of_control_points_m": worst}
    res["speedup_vs_host_loop"] = wall * B / res["fit_given_u_ms"]["median"]
    kr = os.path.join(ROOT, "profiles", "start_lines", "kernel_resources_before_after.json")
    if os.path.exists(kr):
        after = json.load(open(kr))["after"]
        name = [q for q in after if f"k_spline_fit<{k}>" in q]
        if name:
            res["kernel"] = dict(after[name[0]], name=f"k_spline_fit<{k}>", threads=256,
                                 dynamic_lds_bytes=fit_lds_bytes(k, len(cx) - k, N))
    line_ = json.dumps(res)
    print(line_)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
