#!/usr/bin/env python3
"""Timing of the speed-weighted global min-curvature QP (include/rl_mincurv.h: rl_mincurv_global_weighted_batch_dev) on the Monza
table, N = 2000, B = 1024 width-perturbed instances, 6 linearisations.  ONE run on one MI355X, device times from events, one
warm-up and three timed calls per leg:
  1. the unweighted entry on this build and -- with --compare-lib PARENT.so -- on another build of the library (the parent
     commit's), in child processes that alternate, --rounds each: whether this build's median lies within the spread the other
     build's own timings show in the same session; the children time the weighted entry too (w = 1 / linspace(20, 80, N)),
     judged the same way;
  2. the weighted entry with w = 1;
  3. the weighted entry with w = 1 / SPEED of every instance's simulated table;
  4. batch.vehicle_lines_torch(rounds=2) for the 32 x 32 grip x power grid of tools/time_vehicle_sweep.py on the nominal widths:
     time of the whole chain, per further round, and every vehicle's lap time on the unweighted line and on its own.
Prints one JSON line and writes it to --out.

    python tools/time_weighted_global.py [--out profiles/weighted_global/time_weighted_global.json] [--compare-lib PARENT.so]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from time_vehicle_sweep import load_package, sweep_vehicles  # noqa: E402

MARGIN, N_OUTER = 0.25, 6


def timed_ms(fn, repeats=3, warmup=1):
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
    return {"calls_ms": [float(x) for x in ts], "median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def monza(_lib, ops, N):
    """(track, nominal half-widths [N,2], length) of the Monza fixture spline with its real boundary rings."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "G1_spline_fits.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "G1_rings.npz"))
    t, cx, cy, k, length = g["c100_t"], g["c100_cx"], g["c100_cy"], int(g["c100_k"]), float(g["c100_length"])
    pts = ops.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    pts = ops.fill_bounds(pts, r["ringL"], r["ringR"])
    wl = np.hypot(pts[:, 9] - pts[:, 0], pts[:, 10] - pts[:, 1]); wr = np.hypot(pts[:, 11] - pts[:, 0], pts[:, 12] - pts[:, 1])
    return _lib.Track(_lib.Context.get(0), t, cx, cy, k, N), np.stack([wl, wr], 1), length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_global", "time_weighted_global.json"))
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="child mode: the library to time")
    ap.add_argument("--child", action="store_true", help="the unweighted and the weighted entry only, JSON on stdout")
    a = ap.parse_args()
    _lib, ops = load_package(a.lib)
    import torch
    from spline_trajectory_optimization_amd import batch
    dev = torch.device("cuda", 0)
    trk, w_nom, length = monza(_lib, ops, a.N)
    W = torch.from_numpy(batch.width_batch(w_nom[:, 0], w_nom[:, 1], a.B, seed=1234)).to(dev)
    out = ops.global_batch_torch(trk, W, MARGIN, N_OUTER)
    unweighted = timed_ms(lambda: ops.global_batch_torch(trk, W, MARGIN, N_OUTER, out=out))
    if a.child:   # and the weighted entry, with synthetic weights that need no simulated table
        syn = torch.from_numpy(np.ascontiguousarray(np.tile(1.0 / np.linspace(20.0, 80.0, a.N), (a.B, 1)))).to(dev)
        weighted = timed_ms(lambda: ops.global_batch_torch(trk, W, MARGIN, N_OUTER, out=out, weights=syn))
        print("CHILD " + json.dumps({"unweighted": unweighted, "weighted": weighted}))
        return
    res = {"B": a.B, "N": a.N, "n_outer": N_OUTER, "margin_m": MARGIN, "device": torch.cuda.get_device_name(0),
           "timing": "device events, one warm-up and three timed calls per leg",
           "block_threads": int(out["rl_stats"].block_threads), "lds_bytes": int(out["rl_stats"].lds_bytes)}
    res["unweighted_ms"] = unweighted
    plain = {k_: out[k_].clone() for k_ in ("ctrl", "xy", "a", "stats")}
    # 2. w = 1: the unweighted bits through the weighted kernel
    ones = torch.ones((a.B, a.N), dtype=torch.float64, device=dev)
    res["weighted_unit_weights_ms"] = timed_ms(lambda: ops.global_batch_torch(trk, W, MARGIN, N_OUTER, out=out, weights=ones))
    torch.cuda.synchronize()
    res["unit_weights_bit_identical_to_unweighted"] = bool(all(torch.equal(out[k_], plain[k_]) for k_ in plain))
    # 3. w = 1 / SPEED of every instance's own simulated table (one vehicle from the middle of the grid)
    st = sweep_vehicles()
    V = len(st[4])
    one = tuple(np.ascontiguousarray(x[V // 2 + 16]) for x in st)
    lap = batch.lap_times_torch(trk, plain["ctrl"], _lib.BOUNDS_WIDTHS, W, length, one)
    wts = (1.0 / lap["points"][:, :, batch.SPEED_COLUMN]).contiguous()
    res["weighted_speed_weights_ms"] = timed_ms(lambda: ops.global_batch_torch(trk, W, MARGIN, N_OUTER, out=out, weights=wts))
    torch.cuda.synchronize()
    stw = out["stats"].cpu().numpy()
    res["speed_weights"] = {"refused_instances": int((stw[:, 6] != 0).sum()), "ipm_iterations_mean": float(stw[:, 0].mean()),
                            "ipm_iterations_mean_unweighted": float(plain["stats"][:, 0].mean().item()),
                            "max_bound_violation_m": float(stw[:, 3].max()),
                            "max_line_distance_to_unweighted_m": float((out["xy"] - plain["xy"]).norm(dim=2).max().item())}
    res["weighted_over_unweighted"] = {"unit_weights": res["weighted_unit_weights_ms"]["median"] / unweighted["median"],
                                       "speed_weights": res["weighted_speed_weights_ms"]["median"] / unweighted["median"]}
    # 4. the chain: one line per vehicle of the 32 x 32 grid on the nominal widths
    w1 = torch.from_numpy(np.ascontiguousarray(w_nom[None])).to(dev)
    dst = tuple(torch.from_numpy(x).to(dev) for x in st)
    chain = {}
    for rounds in (0, 2):
        chain[f"rounds_{rounds}_ms"] = timed_ms(lambda: batch.vehicle_lines_torch(trk, w1, length, dst, rounds=rounds, margin=MARGIN,
                                                                                  n_outer=N_OUTER))
    vl = batch.vehicle_lines_torch(trk, w1, length, dst, rounds=2, margin=MARGIN, n_outer=N_OUTER)
    torch.cuda.synchronize()
    summ, vst = vl["summary"].cpu().numpy(), vl["stats"].cpu().numpy()
    before, after = summ[0, :, 0], summ[2, :, 0]
    ok = np.isfinite(before) & np.isfinite(after) & (vst[:, :, 6] == 0).all(axis=0)
    chain["vehicles"] = V
    chain["ms_per_further_round"] = (chain["rounds_2_ms"]["median"] - chain["rounds_0_ms"]["median"]) / 2.0
    chain["refused_instances_per_round"] = [int((vst[r, :, 6] != 0).sum()) for r in range(3)]
    chain["lap_time_s"] = {
        "unweighted_line": {"min": float(before[ok].min()), "mean": float(before[ok].mean()), "max": float(before[ok].max())},
        "own_line_after_2_rounds": {"min": float(after[ok].min()), "mean": float(after[ok].mean()), "max": float(after[ok].max())},
        "vehicles_compared": int(ok.sum()), "vehicles_faster_on_their_own_line": int((after[ok] < before[ok]).sum()),
        "gain_s": {"min": float((before - after)[ok].min()), "mean": float((before - after)[ok].mean()),
                   "max": float((before - after)[ok].max())},
        "per_vehicle_unweighted_line": [round(float(x), 4) for x in before],
        "per_vehicle_own_line": [round(float(x), 4) for x in after]}
    chain["max_distance_between_two_vehicles_lines_m"] = float((vl["ctrl"] - vl["ctrl"][V // 2 + 16]).norm(dim=2).max().item())
    res["vehicle_lines"] = chain

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    write()      # (kept if a child of the comparison fails)
    if a.compare_lib:
        # the children run one after the other, each with the GPU to itself
        rounds = {"this": [], "other": []}
        for _ in range(a.rounds):
            for who, lib in (("other", a.compare_lib), ("this", _lib.LIB_PATH)):
                o = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--child", "--N", str(a.N),
                                    "--B", str(a.B)], capture_output=True, text=True, timeout=600)
                if o.returncode != 0:
                    raise RuntimeError(f"child on {lib} failed ({o.returncode}): {o.stderr[-800:]}")
                line = [ln for ln in o.stdout.splitlines() if ln.startswith("CHILD ")][-1]
                rounds[who].append(json.loads(line[len("CHILD "):]))
        for leg in ("unweighted", "weighted"):   # weighted: w = 1 / linspace(20, 80, N) for every instance
            this, other = [r[leg] for r in rounds["this"]], [r[leg] for r in rounds["other"]]
            mine = [r["median"] for r in this]
            theirs = [x for r in other for x in r["calls_ms"]]
            res[f"{leg}_this_build_vs_other"] = {
                "rounds": a.rounds, "order": "other, this, other, this, ...", "this": this, "other": other,
                "this_median_of_rounds_ms": float(np.median(mine)),
                "other_median_of_rounds_ms": float(np.median([r["median"] for r in other])),
                "other_min_ms": float(min(theirs)), "other_max_ms": float(max(theirs)),
                "this_within_other_spread": bool(np.median(mine) <= max(theirs))}
        write()
    print(json.dumps({k_: v for k_, v in res.items() if k_ != "vehicle_lines"} |
                     {"vehicle_lines": {k_: v for k_, v in res["vehicle_lines"].items() if k_ != "lap_time_s"}}))


if __name__ == "__main__":
    main()
