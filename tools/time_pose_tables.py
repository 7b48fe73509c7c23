#!/usr/bin/env python3
"""Timing of the tables of a batch of min-time solutions (include/rl_mincurv.h: rl_pose_tables_batch_dev, kernel
k_pose_tables): 1024 Monza instances at nodes every 5 m (N = 1158) in the FRENET form, rings from per-instance widths.
The poses are synthetic (n = 0.3 m sin, xi = 0.05 rad cos, phase and wave number per instance): the kernel's work does not
depend on where the poses come from, and 1024 NLP solves are not what is timed.  ONE run on one MI355X, warm-up first:
  * rl_pose_tables_batch_dev, device time from events: the median of --repeats single launches, and --repeats launches back to
    back between one pair of events (the per-launch figure free of the event overhead);
  * the same with the culled and the brute-force ring search, and bit identity of the three;
  * the route it replaces: the tail of optimise_track per instance on the host (min_time_optimizer.pose_table: scipy
    interpolants, two synchronous fill_bounds calls, fill_distance in numpy), wall time of --baseline-instances, scaled to B.
Prints one JSON line and writes it to --out.

    python tools/time_pose_tables.py [--out profiles/pose_tables/time_pose_tables.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_tables", "time_pose_tables.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--interval", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--baseline-instances", type=int, default=16)
    a = ap.parse_args()
    import torch
    from spline_trajectory_optimization_amd import _lib, batch, ops
    from spline_trajectory_optimization_amd.min_time_optm.min_time_optimizer import pose_table
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack
    centre, left, right = batch.load_monza()
    rt = RaceTrack("Monza", left, right, centre, s=10.0, interval=a.interval)
    traj_d = rt.center_d.copy()
    N, B = len(traj_d), a.B
    L = rt.center_s.get_length()
    wl, wr = batch.half_widths_from_bounds(traj_d.points)
    widths = np.ascontiguousarray(batch.width_batch(wl, wr, B, seed=1234))
    trk = batch.make_track(rt.center_s, N)
    rng = np.random.default_rng(0)
    i = np.arange(N)
    ph = rng.uniform(0, 2 * np.pi, size=(B, 1))
    wn = rng.integers(2, 12, size=(B, 1))
    X = np.zeros((B, N, 6))
    X[:, :, 0] = rt.abscissa
    X[:, :, 1] = 0.3 * np.sin(2 * np.pi * wn * i / N + ph)
    X[:, :, 2] = 0.05 * np.cos(2 * np.pi * (wn + 1) * i / N + ph)
    X[:, :, 5] = 40.0
    T = np.full((B, N), L / N / 40.0)
    dev = torch.device("cuda", 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    X_d, T_d, w_d, base_d = up(X), up(T), up(widths), up(traj_d.points)
    pieces = tuple(up(p) for p in rt.centerline_pieces())
    out = torch.empty((B, N, 19), dtype=torch.float64, device=dev)
    ctx = trk.ctx
    res = {"B": B, "N": N, "ring_vertices": N, "pieces": int(pieces[0].shape[0]) - 1, "repeats": a.repeats,
           "form": "FRENET, width rings, base [N,19], T given", "device": torch.cuda.get_device_name(0)}
    ref = None
    for name, mode in (("windowed", _lib.SEARCH_WINDOWED), ("culled", _lib.SEARCH_CULLED), ("brute", _lib.SEARCH_BRUTE)):
        ctx.set_option("tables_search", mode)
        res[f"pose_tables_{name}_ms"] = launch_ms(
            lambda: ops.pose_tables_torch(trk, _lib.POSE_FRENET, X_d, pieces, _lib.BOUNDS_WIDTHS, w_d, base=base_d, T=T_d, out=out),
            a.repeats if mode != _lib.SEARCH_BRUTE else max(3, a.repeats // 4), warmup=2)
        cur = out.cpu().numpy()
        ref = cur if ref is None else ref
        res[f"pose_tables_{name}_bit_identical_to_windowed"] = bool(np.array_equal(cur, ref))
    ctx.set_option("tables_search", _lib.SEARCH_WINDOWED)
    res["bytes_moved_min"] = int(B * N * 8 * (19 + 6 + 1 + 2) + N * 19 * 8)   # rows out, X, T, widths in, base once
    res["summary_lap_time_s"] = float(ops.table_summary_torch(out)[0, 0].item())
    # the route it replaces: optimise_track's tail per instance (against race_track's own rings: the host route has no other)
    nb = min(a.baseline_instances, B)
    pose_table(rt, traj_d, X[0])
    t0 = time.perf_counter()
    for b in range(nb):
        pose_table(rt, traj_d, X[b])
    dt = time.perf_counter() - t0
    res["baseline_optimise_track_tail_host"] = {"instances_timed": nb, "wall_ms_per_instance": 1e3 * dt / nb,
                                                "wall_ms_scaled_to_B": 1e3 * dt / nb * B}
    res["k_tables_reference_ms"] = {"value": 2.00, "workload": "B = 1024, N = 2000, 21 spline evaluations per sample more",
                                    "source": "profiles/tables/time_tables.json"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
