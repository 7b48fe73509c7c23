#!/usr/bin/env python3
"""Timing of the batched sliding-window driver (include/rl_mincurv.h: rl_mincurv_solve_batch_joint_dev, kernels
k_sweep<SweepConfigWindowFrom<...>>) on the benchmarked batch: Monza, N = 2000, B = 1024 width-perturbed instances (bench.py's
headline batch, widths seed 1234), max_iter = 3 outer iterations of 56 windows, reference-order arithmetic.  ONE run on one
MI355X, warm-up first:
  * rl_mincurv_solve_batch_joint_dev, device time from events: the median of --repeats single launches (and the same launches
    back to back), in the residency the plan picks, and with the other one forced where the forcing takes effect;
  * the route that existed before: rl_mincurv_sweep_joint, one synchronous host call per instance against the track's shared
    rings -- the instance's width rings set with rl_track_set_rings first.  --baseline-instances (8) instances are timed and the
    wall time is SCALED to B: nobody waits for 1024 of them here.
  * --bench-parent DIR (a checkout of the parent commit, built): the headline of bench.py (--gpus 1 --steps 5 --warmup 1), parent
    and this tree alternating, --bench-runs each; the spread of the parent's own runs is the yardstick for "did not move".
The measurement runs in a child process under a time limit of its own (--timeout seconds), every bench.py run likewise.
Prints one JSON line per file and writes --out / --bench-out.

    python tools/time_window_batch.py [--out profiles/window_batch/time_window_batch.json] [--bench-parent DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def launch_ms(fn, repeats, warmup=2):
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


def measure(a):
    import torch
    from scipy import interpolate
    from spline_trajectory_optimization_amd import _lib, batch, ops
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack
    centre, left, right = batch.load_monza()
    line = batch.monza_centerline(100.0, 5)
    t, cx, cy, k = line._tck()
    N, B, n = a.N, a.B, len(cx)
    traj = line.sample_along(ts=np.linspace(0.0, 1.0, N, endpoint=False))
    RaceTrack("Monza", left, right, centre).fill_trajectory_boundaries(traj)
    wl, wr = batch.half_widths_from_bounds(traj.points)
    widths = np.ascontiguousarray(batch.width_batch(wl, wr, B, seed=1234))
    i_start = batch.default_i_start(n, k, a.max_iter, seed=0, driver="window")
    trk = batch.make_track(line, N)
    dev = torch.device("cuda", 0)
    dw = torch.from_numpy(widths).to(dev)
    W, REF = _lib.BOUNDS_WIDTHS, _lib.ARITH_REFERENCE
    out = {"ctrl": torch.empty((B, n, 2), dtype=torch.float64, device=dev), "xy": torch.empty((B, N, 2), dtype=torch.float64, device=dev),
           "n_success": torch.empty((B, a.max_iter), dtype=torch.int32, device=dev), "status": torch.empty((B,), dtype=torch.int32, device=dev)}
    res = {"B": B, "N": N, "max_iter": a.max_iter, "windows_per_iteration": int(np.diff(batch.i_start_range(n, k, "window"))[0]),
           "arithmetic": "reference-order", "i_start": i_start.tolist(), "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "batch": f"bench.py's headline batch (Monza, N = {N}, {B} width instances, widths seed 1234), window driver from the track's line"}
    stats = {}

    def run():
        stats["st"] = ops.solve_batch_torch(trk, W, dw, i_start, out=out, arith=REF, driver="window")["stats"]

    # the residency the plan picks, then the OTHER one forced -- timed only if the forcing takes effect (a state that does not fit
    # LDS runs all-global whatever is asked: timing it again would be the same kernel under another name)
    os.environ.pop("RL_FORCE_RESIDENCY", None)
    blk = launch_ms(run, a.repeats)
    planned = int(stats["st"].rings_in_lds)
    blk["rings_in_lds"] = planned; blk["lds_bytes_per_workgroup"] = int(stats["st"].lds_bytes)
    res["batch_joint_dev_ms_plan"] = blk
    other = "all_lds" if planned == 0 else "all_global"
    os.environ["RL_FORCE_RESIDENCY"] = "1" if planned == 0 else "0"
    run(); torch.cuda.synchronize()
    if int(stats["st"].rings_in_lds) != planned:
        blk = launch_ms(run, a.repeats)
        blk["rings_in_lds"] = int(stats["st"].rings_in_lds); blk["lds_bytes_per_workgroup"] = int(stats["st"].lds_bytes)
        res[f"batch_joint_dev_ms_forced_{other}"] = blk
    else:
        res["other_residency"] = f"{other} was asked for (RL_FORCE_RESIDENCY) and did not take effect: the plan's residency is the only one at this size"
    os.environ.pop("RL_FORCE_RESIDENCY", None)
    run(); torch.cuda.synchronize()
    ns, status = out["n_success"].cpu().numpy(), out["status"].cpu().numpy()
    res["windows_updated_share"] = float(ns.sum() / (ns.size * res["windows_per_iteration"]))
    res["instances_that_updated_a_window"] = int((ns.sum(axis=1) > 0).sum())
    ms = res["batch_joint_dev_ms_plan"]["median"]
    res["instances_per_s"] = B / ms * 1e3
    res["ms_per_instance_in_the_batch"] = ms / B

    # the route of the parent commit: one synchronous rl_mincurv_sweep_joint per instance on the instance's own rings
    u = np.arange(N) / N
    sx, sy = interpolate.BSpline(t, cx, k), interpolate.BSpline(t, cy, k)
    px, py, dx, dy = sx(u), sy(u), sx.derivative()(u), sy.derivative()(u)
    nrm = np.hypot(dx, dy)
    nx, ny = -dy / nrm, dx / nrm                           # left normal
    trk1 = batch.make_track(line, N)
    nb = a.baseline_instances

    def single(b):
        w = widths[b]
        trk1.set_rings(np.column_stack([px + w[:, 0] * nx, py + w[:, 0] * ny]), np.column_stack([px - w[:, 1] * nx, py - w[:, 1] * ny]))
        return ops.mincurv_sweep_joint(trk1, cx, cy, i_start, want_points=False, arith=REF)

    single(0)                                              # warm-up: tables of the reference-order arithmetic, first launch
    walls, kernels, updated = [], [], []
    for b in range(nb):
        t0 = time.perf_counter()
        r = single(b)
        walls.append((time.perf_counter() - t0) * 1e3); kernels.append(float(r[4].kernel_ms)); updated.append(int(r[3].sum()))
    res["baseline_sweep_joint_per_instance"] = {
        "instances_timed": nb, "wall_ms_per_instance_median": float(np.median(walls)), "wall_ms_per_instance": walls,
        "kernel_ms_per_instance_median": float(np.median(kernels)), "kernel_ms_per_instance": kernels, "windows_updated": updated,
        "wall_ms_scaled_to_B": float(np.mean(walls) * B), "kernel_ms_scaled_to_B": float(np.mean(kernels) * B),
        "note": f"{nb} instances timed, scaled to B = {B} by the mean; rings are the width rings about the centre line (scipy's "
                "evaluation: the timing does not depend on their last bits)"}
    res["speedup_vs_per_instance_calls_wall"] = res["baseline_sweep_joint_per_instance"]["wall_ms_scaled_to_B"] / ms
    res["speedup_vs_per_instance_calls_kernel_time"] = res["baseline_sweep_joint_per_instance"]["kernel_ms_scaled_to_B"] / ms
    kr = os.path.join(ROOT, "profiles", "window_batch", "kernel_resources_before_after.json")
    if os.path.exists(kr):
        res["kernels"] = json.load(open(kr)).get("new_kernels_resources")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def bench_headline(root, timeout):
    """One run of bench.py's headline in `root`, in a process of its own: (solves/s, kernel ms per step)."""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], cwd=root, capture_output=True,
                       text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py in {root}: exit {p.returncode}: {p.stderr[-400:]}")
    line = [q for q in p.stdout.splitlines() if q.startswith("{")][-1]
    r = json.loads(line)
    return float(r["value"]), float(r["roofline"]["kernel_ms"])


def bench_compare(a):
    runs = {"parent": [], "pr": []}
    for i in range(a.bench_runs):
        for who, root in (("parent", os.path.abspath(a.bench_parent)), ("pr", ROOT)):
            v, ms = bench_headline(root, a.bench_timeout)
            runs[who].append({"solves_per_s": v, "kernel_ms": ms})
            print(f"bench {who} run {i}: {v:.1f} solves/s, {ms:.3f} ms", flush=True)
    val = {w: np.array([r["solves_per_s"] for r in runs[w]]) for w in runs}
    spread = float(val["parent"].max() - val["parent"].min())
    res = {"what": "bench.py --gpus 1 --steps 5 --warmup 1 (headline: min-curvature QP solves/s, N = 2000, 1024 width instances, "
                   "reference-order arithmetic), the parent commit's tree and this one alternating, one process per run",
           "runs": runs, "parent_median": float(np.median(val["parent"])), "pr_median": float(np.median(val["pr"])),
           "parent_run_to_run_spread": spread, "parent_min": float(val["parent"].min()), "parent_max": float(val["parent"].max()),
           "pr_minus_parent_median": float(np.median(val["pr"]) - np.median(val["parent"])),
           "pr_median_within_parent_spread": bool(abs(np.median(val["pr"]) - np.median(val["parent"])) <= spread),
           "note": "the sweep kernels are the parent's (profiles/window_batch/kernel_resources_before_after.json)"}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.bench_out), exist_ok=True)
    with open(a.bench_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_batch", "time_window_batch.json"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "window_batch", "bench_parent_vs_pr.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--max-iter", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--baseline-instances", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--bench-parent", default=None, help="built checkout of the parent commit: also compare bench.py's headline")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=150, help="seconds one bench.py run may take")
    ap.add_argument("--skip-timing", action="store_true", help="only the bench.py comparison")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        measure(a)
        return
    if not a.skip_timing:   # this process never opens the GPU: the measurement is a child under a time limit
        args = [q for q in sys.argv[1:]]
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, timeout=a.timeout)
        if p.returncode != 0:
            sys.exit(p.returncode)
    if a.bench_parent:
        bench_compare(a)


if __name__ == "__main__":
    main()
