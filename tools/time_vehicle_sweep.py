#!/usr/bin/env python3
"""Timing of a vehicle sweep (include/rl_mincurv.h: rl_qss_sim_vehicles_dev) on the Monza centre-line table at N = 2000.
ONE run on one MI355X, device times from events, warm-up first, median of --repeats launches:
  * B = 1024 vehicles (32 grip levels 0.6 .. 1.2 x 32 power levels 0.5 .. 1.3 of the two-piece lookups) in ONE launch with
    per-instance vehicles, device tensors throughout;
  * the shared-vehicle launch of the same B (rl_qss_sim_dev);
  * the route it replaces: rl_qss_sim once per vehicle (wall time, synchronous host calls; --baseline-vehicles of the B, scaled).
--compare-lib OTHER.so adds the shared-vehicle legs B = 1 / 256 / 1024 on this build and on another build of the library (the
parent commit's), in child processes that alternate, --rounds each: the medians of every round of both, and whether this
build's median lies within the spread the other build's rounds show by themselves.  (A library that lacks the vehicle entry
points can only run the shared legs.)  Prints one JSON line and writes it to --out.

    python tools/time_vehicle_sweep.py [--out profiles/vehicle_sweep/time_vehicle_sweep.json] [--compare-lib PARENT.so]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHARED_LEGS = (1, 256, 1024)


def median_ms(fn, repeats, warmup=2):
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


def sweep_vehicles(n_grip=32, n_power=32):
    """The stacked 5-tuple of n_grip x n_power vehicles.  The breakpoints are shared, so CubicSpline takes all value columns in
    one call."""
    from scipy.interpolate import CubicSpline
    g, p = np.meshgrid(np.linspace(0.6, 1.2, n_grip), np.linspace(0.5, 1.3, n_power), indexing="ij")
    g, p = g.ravel(), p.ravel()
    x = np.array([0.0, 50.0, 100.0])
    acc = CubicSpline(x, np.array([10.0, 7.0, 0.5])[:, None] * p[None, :])
    dcc = CubicSpline(x, np.array([-13.0, -15.0, -20.0])[:, None] * g[None, :])
    B = len(g)
    params = np.column_stack([10.0 * g, -20.0 * g, 15.0 * g, -15.0 * g, np.full(B, 100.0), np.full(B, 30.0)])
    tile = lambda a: np.ascontiguousarray(np.repeat(a[None], B, axis=0))  # noqa: E731
    return (tile(acc.x), np.ascontiguousarray(acc.c.transpose(2, 0, 1)), tile(dcc.x), np.ascontiguousarray(dcc.c.transpose(2, 0, 1)),
            np.ascontiguousarray(params))


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
    from spline_trajectory_optimization_amd import ops
    return _lib, ops


def monza_table(ops, N):
    g = np.load(os.path.join(ROOT, "tests", "golden", "G1_spline_fits.npz"))
    t, cx, cy, k, length = g["c100_t"], g["c100_cx"], g["c100_cy"], int(g["c100_k"]), float(g["c100_length"])
    return ops.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))


def shared_legs(ops, pts, veh, repeats):
    import torch
    dev = torch.device("cuda", 0)
    out = {}
    for B in SHARED_LEGS:
        P = torch.from_numpy(np.ascontiguousarray(np.repeat(pts[None], B, axis=0))).to(dev)
        out[str(B)] = median_ms(lambda: ops.qss_sim_torch(P, *veh), repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vehicle_sweep", "time_vehicle_sweep.json"))
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--baseline-vehicles", type=int, default=8)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="child mode: the shared legs on this library, JSON on stdout")
    ap.add_argument("--shared-only", action="store_true")
    a = ap.parse_args()
    _lib, ops = load_package(a.lib)
    import time
    import torch
    pts = monza_table(ops, a.N)
    st = sweep_vehicles()
    B = len(st[4])
    one = tuple(np.ascontiguousarray(x[B // 2 + 16]) for x in st)          # a vehicle from the middle of the grid
    if a.shared_only:
        print("SHARED " + json.dumps(shared_legs(ops, pts, one, a.repeats)))
        return
    dev = torch.device("cuda", 0)
    res = {"B": B, "N": a.N, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "vehicles": "32 grip levels 0.6 .. 1.2 x 32 power levels 0.5 .. 1.3, two-piece lookups, vmax 100, jerk 30"}
    P = torch.from_numpy(np.ascontiguousarray(np.repeat(pts[None], B, axis=0))).to(dev)
    dst = tuple(torch.from_numpy(x).to(dev) for x in st)
    res["vehicles_one_launch_ms"] = median_ms(lambda: ops.qss_sim_vehicles_torch(P, *dst), a.repeats)
    it = ops.qss_sim_vehicles_torch(P, *dst)
    lap = ops.table_summary_torch(P, it)[:, 0].cpu().numpy()
    itc = it.cpu().numpy()
    res["lap_time_s"] = {"min": float(np.nanmin(lap)), "max": float(np.nanmax(lap)), "raised": int((itc < 0).sum()),
                         "iterations_min": int(itc[itc >= 0].min()), "iterations_max": int(itc.max())}
    # how many of them the dataflow kernel gives back to the list-order kernel behind it (test hook qss_df_redo = 0 shows them)
    ctx = _lib.Context.get(0)
    Q = P.clone()
    ctx.set_option("qss_df_redo", 0)
    try:
        itq = ops.qss_sim_vehicles_torch(Q, *dst).cpu().numpy()
    finally:
        ctx.set_option("qss_df_redo", 1)
    res["handed_back_to_the_list_order_kernel"] = {"instances": int((itq <= -100).sum()),
                                                   "reasons": sorted({int(-100 - v) for v in itq[itq <= -100]})}
    # the same B through both entry points with ONE vehicle (B copies of it): what the per-instance path itself costs
    cst = tuple(x[B // 2 + 16:B // 2 + 17].expand((B,) + tuple(x.shape[1:])).contiguous() for x in dst)
    res["copies_of_one_vehicle_one_launch_ms"] = median_ms(lambda: ops.qss_sim_vehicles_torch(Q, *cst), a.repeats)
    res["shared_vehicle_one_launch_ms"] = median_ms(lambda: ops.qss_sim_torch(Q, *one), a.repeats)
    # the route it replaces: one synchronous host call per vehicle
    nb = min(a.baseline_vehicles, B)
    pick = np.linspace(0, B - 1, nb).astype(int)
    same = True
    for b in pick:      # (the warm-up, and the check that both routes compute the same; a raised instance's columns are undefined)
        out, it1 = ops.qss_sim(pts, *[x[b] for x in st])
        same = same and int(it1[0]) == int(itc[b]) and (itc[b] < 0 or out.tobytes() == P[b].cpu().numpy().tobytes())
    t0 = time.perf_counter()
    for b in pick:
        ops.qss_sim(pts, *[x[b] for x in st])
    dt = time.perf_counter() - t0
    res["per_vehicle_host_calls"] = {"vehicles_timed": nb, "wall_ms_per_vehicle": 1e3 * dt / nb,
                                     "wall_ms_scaled_to_B": 1e3 * dt / nb * B, "bit_identical_to_the_one_launch": bool(same)}
    res["one_launch_speedup_over_per_vehicle_calls"] = res["per_vehicle_host_calls"]["wall_ms_scaled_to_B"] / \
        res["vehicles_one_launch_ms"]["median"]
    res["vehicles_over_shared"] = res["vehicles_one_launch_ms"]["median"] / res["shared_vehicle_one_launch_ms"]["median"]
    res["copies_over_shared"] = res["copies_of_one_vehicle_one_launch_ms"]["median"] / res["shared_vehicle_one_launch_ms"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:      # (kept if a child of the comparison fails)
        json.dump(res, f, indent=1)
        f.write("\n")
    if a.compare_lib:
        # this process lets go of nothing it needs later: the children run one after the other, each with the GPU to itself
        rounds = {"this": [], "other": []}
        for r in range(a.rounds):
            for who, lib in (("other", a.compare_lib), ("this", _lib.LIB_PATH)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--shared-only", "--N", str(a.N),
                                      "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise RuntimeError(f"child on {lib} failed ({out.returncode}): {out.stderr[-800:]}")
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("SHARED ")][-1]
                rounds[who].append(json.loads(line[len("SHARED "):]))
        cmp_ = {"rounds": a.rounds, "order": "other, this, other, this, ...", "legs_B": list(SHARED_LEGS), "this": rounds["this"],
                "other": rounds["other"], "summary": {}}
        for Bs in map(str, SHARED_LEGS):
            mine = [r[Bs]["median"] for r in rounds["this"]]; theirs = [r[Bs]["median"] for r in rounds["other"]]
            cmp_["summary"][Bs] = {"this_median_of_rounds_ms": float(np.median(mine)), "other_median_of_rounds_ms": float(np.median(theirs)),
                                   "other_min_ms": float(min(theirs)), "other_max_ms": float(max(theirs)),
                                   "this_within_other_spread": bool(np.median(mine) <= max(theirs))}
        res["shared_legs_this_build_vs_other"] = cmp_
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
