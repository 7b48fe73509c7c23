#!/usr/bin/env python3
"""Timing of the min-time solve with one vehicle per instance (include/rl_mincurv.h: rl_mintime_solve_vehicles) on the README's
batch: MGKT at 1 m (N = 828), B = 1024 width-perturbed tracks.  ONE run on one MI355X; host calls timed on the wall clock
(copies of the guess and of the solution included, as tools/bench_mintime.py times them), one warm-up at the full batch size
first, --repeats timed calls per leg, their median / min / max:
  * equal rows against the shared entry: B copies of MODEL through the vehicles entry, and the shared-model entry, on the
    same batch (both must return the same bits);
  * the grid: B = 32 grip (mu x 0.7 .. 1.1) x 32 power (Pmax x 0.6 .. 1.2) vehicles on the unperturbed track in one call,
    against the per-vehicle loop of single calls it replaces (--baseline-vehicles of the B, scaled);
  * --compare-lib OTHER.so: the shared-model leg on this build and on another build of the library (the parent commit's) in
    child processes that alternate, --rounds each: the medians of every round of both, and whether this build's median lies
    within the range the other build's rounds show by themselves.
Prints one JSON line and writes it to --out.

    python tools/time_mintime_vehicles.py [--out profiles/mintime_vehicles/time_mintime_vehicles.json] [--compare-lib PARENT.so]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MAX_ITER, TOL = 300, 1e-6


def load_package(lib_path):
    """The package on the library at lib_path (None: its own); entry points that library lacks are left unbound."""
    if lib_path:
        os.environ["RL_LIB_PATH"] = os.path.abspath(lib_path)
    from spline_trajectory_optimization_amd import _lib
    if lib_path:
        import torch  # noqa: F401  (first, as _lib.load does: the library then shares torch's HIP runtime)
        probe = ctypes.CDLL(os.path.abspath(lib_path))
        for name in [n for n in _lib._SIGNATURES if not hasattr(probe, n)]:
            del _lib._SIGNATURES[name]
    return _lib


def timed(fn, repeats):
    fn()                                        # warm-up at the timed batch size (arena, staging pool)
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "calls": len(ts)}, out


def report(st):
    return {"converged": int((st[:, 5] == 1).sum()), "of": int(len(st)), "iterations_mean": float(st[:, 0].mean()),
            "iterations_max": float(st[:, 0].max()), "lap_s_min_max": [float(st[:, 4].min()), float(st[:, 4].max())]}


def grid_models(model, n_grip=32, n_power=32):
    g, p = np.meshgrid(np.linspace(0.7, 1.1, n_grip), np.linspace(0.6, 1.2, n_power), indexing="ij")
    return [dict(model, mu=model["mu"] * a, Pmax=model["Pmax"] * b) for a, b in zip(g.ravel(), p.ravel())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mintime_vehicles", "time_mintime_vehicles.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-vehicles", type=int, default=8)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="child mode: the shared-model leg on this library, JSON on stdout")
    ap.add_argument("--shared-only", action="store_true")
    a = ap.parse_args()
    _lib = load_package(a.lib)
    import torch
    from spline_trajectory_optimization_amd.min_time_optm import example
    prob = example.mgkt_problem()
    B = a.B
    left, right = example.perturbed_widths(prob, B)
    kw = dict(max_iter=MAX_ITER, tol=TOL)
    prob.solve_batch(left[:2], right[:2], max_iter=8)          # module load, kernels resident
    shared_t, shared = timed(lambda: prob.solve_batch(left, right, **kw), a.repeats)
    if a.shared_only:
        print("SHARED " + json.dumps(shared_t))
        return
    res = {"B": B, "N": int(prob.N), "repeats": a.repeats, "max_iter": MAX_ITER, "tol": TOL, "device": torch.cuda.get_device_name(0),
           "timed": "host calls on the wall clock, host<->device copies of guess and solution included; one warm-up per leg first"}
    copies_t, copies = timed(lambda: prob.solve_batch(left, right, models=[prob.model] * B, **kw), a.repeats)
    res["equal_rows_against_the_shared_entry"] = {
        "batch": "B width-perturbed MGKT tracks (example.perturbed_widths), every row = MODEL",
        "shared_entry": shared_t, "vehicles_entry": copies_t,
        "vehicles_over_shared_median": copies_t["median_s"] / shared_t["median_s"],
        "bit_identical": bool(all(np.array_equal(x, y) for x, y in zip(shared, copies))), "result": report(shared[3])}
    # the grid: one call against the per-vehicle loop
    ms = grid_models(prob.model)[:B]
    Bg = len(ms)
    l1, r1 = np.repeat(prob.left[None], Bg, axis=0), np.repeat(prob.right[None], Bg, axis=0)
    grid_t, grid = timed(lambda: prob.solve_batch(l1, r1, models=ms, **kw), a.repeats)
    nb = min(a.baseline_vehicles, Bg)
    pick = np.linspace(0, Bg - 1, nb).astype(int)
    from spline_trajectory_optimization_amd import ops
    single = lambda b: ops.mintime_solve_batch(ms[b], prob.s, prob.kappa, prob.left, prob.right, prob.margin, prob.track_length,  # noqa: E731
                                               prob.X0[None], prob.U0[None], prob.T0[None], prob.average_track_width,
                                               prob.speed_cap, **kw)
    same = all(all(np.array_equal(x[0], y[b]) for x, y in zip(single(b), grid)) for b in pick)     # (also the warm-up)
    t0 = time.perf_counter()
    for b in pick:
        single(b)
    dt = time.perf_counter() - t0
    res["grid"] = {"vehicles": "32 grip levels mu x 0.7 .. 1.1 by 32 power levels Pmax x 0.6 .. 1.2 of MODEL, the unperturbed track",
                   "B": Bg, "one_call": grid_t, "result": report(grid[3]),
                   "per_vehicle_single_calls": {"vehicles_timed": nb, "wall_s_per_vehicle": dt / nb, "wall_s_scaled_to_B": dt / nb * Bg,
                                                "bit_identical_to_the_one_call": bool(same)},
                   "one_call_speedup_over_the_loop": dt / nb * Bg / grid_t["median_s"],
                   "solves_per_s": Bg / grid_t["median_s"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:      # (kept if a child of the comparison fails)
        json.dump(res, f, indent=1)
        f.write("\n")
    if a.compare_lib:
        rounds = {"this": [], "other": []}
        for r in range(a.rounds):
            for who, lib in (("other", a.compare_lib), ("this", _lib.LIB_PATH)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--shared-only", "--B", str(B),
                                      "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    raise RuntimeError(f"child on {lib} failed ({out.returncode}): {out.stderr[-800:]}")
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("SHARED ")][-1]
                rounds[who].append(json.loads(line[len("SHARED "):]))
                print(f"round {r} {who}: {rounds[who][-1]}", file=sys.stderr, flush=True)
        mine = [r["median_s"] for r in rounds["this"]]; theirs = [r["median_s"] for r in rounds["other"]]
        res["shared_entry_this_build_vs_other"] = {
            "rounds": a.rounds, "order": "other, this, other, this, ...", "this": rounds["this"], "other": rounds["other"],
            "this_median_of_rounds_s": float(np.median(mine)), "other_median_of_rounds_s": float(np.median(theirs)),
            "other_min_s": float(min(theirs)), "other_max_s": float(max(theirs)),
            "this_within_other_range": bool(np.median(mine) <= max(theirs))}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
