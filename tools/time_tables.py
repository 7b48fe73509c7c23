#!/usr/bin/env python3
"""Timing of the tables of a solved batch (include/rl_mincurv.h: rl_tables_batch_dev, kernel k_tables) on bench.py's
workload: 1024 Monza width instances at N = 2000, solved by the sweep.  ONE run on one MI355X, device times from events,
warm-up first, median of --repeats launches:
  * rl_tables_batch_dev with the windowed, the culled and the brute-force ring search;
  * the route it replaces, the only one there was: per instance ops.sample_along + ops.fill_bounds on hand-built rings
    (wall time, synchronous host calls; --baseline-instances of the 1024, scaled);
  * the chain batch.lap_times_torch (tables + QSS simulation + summary), and the sweep itself for scale.
--parity adds profiles/tables/parity.json: on the first 16 instances, the curvature column of the kernel against the
strict oracle, beside the spread of the oracle's strict and FMA-contracted builds (tests/test_tables_gpu.py's rule).
--resources FILE.s adds the registers / spills / LDS of the new kernels from a gfx950 assembly listing
(tools/kernel_resources.py's fields).  Prints one JSON line and writes it to --out.

    python tools/time_tables.py [--out profiles/tables/time_tables.json] [--parity] [--resources rl_mincurv-hip-amdgcn-amd-amdhsa-gfx950.s]"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def kernel_resources(path, names=("k_tables", "k_table_summary")):
    txt = open(path).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        f = dict(re.findall(r"\.(\w+):\s+([^\n]+)", ".agpr_count:" + blk))
        if any(n in f.get("name", "") for n in names):
            out[f["name"]] = {k: int(f[k]) for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                     "private_segment_fixed_size", "group_segment_fixed_size") if k in f}
    return out


def median_ms(fn, repeats, warmup=3):
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables", "time_tables.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--baseline-instances", type=int, default=64)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    import torch
    from scipy.interpolate import CubicSpline
    from spline_trajectory_optimization_amd import _lib, batch, ops
    g = np.load(os.path.join(ROOT, "tests", "golden", "G1_spline_fits.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "G1_rings.npz"))
    g6 = np.load(os.path.join(ROOT, "tests", "golden", "G6_simulator.npz"))
    t, cx, cy, k, length = g["c100_t"], g["c100_cx"], g["c100_cy"], int(g["c100_k"]), float(g["c100_length"])
    B, N = a.B, a.N
    ctx = _lib.Context.get(0)
    u = np.linspace(0.0, 1.0, N, endpoint=False)
    base = ops.fill_bounds(ops.sample_along(t, cx, cy, k, length, u), r["ringL"], r["ringR"])
    wl, wr = batch.half_widths_from_bounds(base)
    widths = batch.width_batch(wl, wr, B, seed=1234)
    trk = _lib.Track(ctx, t, cx, cy, k, N)
    i_start = batch.default_i_start(len(cx), k, 5, seed=0)
    dev = torch.device("cuda", 0)
    w_d = torch.from_numpy(widths).to(dev)
    sol = ops.solve_batch_torch(trk, _lib.BOUNDS_WIDTHS, w_d, i_start)
    torch.cuda.synchronize()
    ctrl_d = sol["ctrl"]
    out = torch.empty((B, N, 19), dtype=torch.float64, device=dev)
    res = {"B": B, "N": N, "n": len(cx), "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    res["sweep_ms"] = median_ms(lambda: ops.solve_batch_torch(trk, _lib.BOUNDS_WIDTHS, w_d, i_start, out=sol), a.repeats)[0]
    ref = None
    for name, mode in (("windowed", _lib.SEARCH_WINDOWED), ("culled", _lib.SEARCH_CULLED), ("brute", _lib.SEARCH_BRUTE)):
        ctx.set_option("tables_search", mode)
        med, lo, hi = median_ms(lambda: ops.tables_torch(trk, ctrl_d, _lib.BOUNDS_WIDTHS, w_d, length, out=out),
                                a.repeats if mode != _lib.SEARCH_BRUTE else max(3, a.repeats // 4), warmup=2)
        res[f"tables_{name}_ms"] = {"median": med, "min": lo, "max": hi}
        cur = out.cpu().numpy()
        if ref is None:
            ref = cur
        res[f"tables_{name}_bit_identical_to_windowed"] = bool(np.array_equal(cur, ref))
    ctx.set_option("tables_search", _lib.SEARCH_WINDOWED)
    acc = CubicSpline(g6["acc_lookup"][:, 0], g6["acc_lookup"][:, 1]); dcc = CubicSpline(g6["dcc_lookup"][:, 0], g6["dcc_lookup"][:, 1])
    veh = (acc.x, acc.c, dcc.x, dcc.c, g6["params"])
    res["lap_times_chain_ms"] = median_ms(lambda: batch.lap_times_torch(trk, ctrl_d, _lib.BOUNDS_WIDTHS, w_d, length, veh),
                                          max(5, a.repeats // 4), warmup=1)[0]
    chain = batch.lap_times_torch(trk, ctrl_d, _lib.BOUNDS_WIDTHS, w_d, length, veh)
    lap = chain["summary"][:, 0].cpu().numpy()
    res["lap_time_s"] = {"min": float(np.nanmin(lap)), "max": float(np.nanmax(lap)), "argmin": int(np.nanargmin(lap)),
                         "raised": int((chain["iters"] < 0).sum().item())}
    # the route it replaces: two synchronous host calls per instance, rings built by hand on the host
    ctrl = ctrl_d.cpu().numpy()
    nb = min(a.baseline_instances, B)
    nrm = np.stack([base[:, 0], base[:, 1], np.cos(base[:, 3] + np.pi / 2), np.sin(base[:, 3] + np.pi / 2)], 1)
    t0 = time.perf_counter()
    worst = 0.0
    for b in range(nb):
        p = ops.sample_along(t, ctrl[b, :, 0].copy(), ctrl[b, :, 1].copy(), k, length, u)
        rl_ = nrm[:, :2] + widths[b, :, 0:1] * nrm[:, 2:]
        rr_ = nrm[:, :2] - widths[b, :, 1:2] * nrm[:, 2:]
        ops.fill_bounds(p, rl_, rr_)
        worst = max(worst, float(np.abs(p[:, [0, 1, 9, 10, 11, 12]] - ref[b][:, [0, 1, 9, 10, 11, 12]]).max()))
    dt = time.perf_counter() - t0
    res["baseline_per_instance_host_calls"] = {"instances_timed": nb, "wall_ms_per_instance": 1e3 * dt / nb,
                                               "wall_ms_scaled_to_B": 1e3 * dt / nb * B,
                                               "max_abs_diff_xy_bounds_vs_batched_m": worst}
    res["tables_windowed_over_sweep"] = res["tables_windowed_ms"]["median"] / res["sweep_ms"]
    if a.resources:
        res["kernel_resources"] = kernel_resources(a.resources)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if a.parity:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import tables_twin as tw
        from oracle import oracle as orc
        nb = 16
        rings = [tw.width_rings(t, cx, cy, k, N, widths[b]) for b in range(nb)]
        strict = tw.tables(t, k, N, ctrl[:nb], rings, length)
        with orc.fma_variant():
            fma = tw.tables(t, k, N, ctrl[:nb], [tw.width_rings(t, cx, cy, k, N, widths[b]) for b in range(nb)], length)
        spread = float(np.abs(1 / strict[..., 5] - 1 / fma[..., 5]).max())
        devk = float(np.abs(1 / ref[:nb, :, 5] - 1 / strict[..., 5]).max())
        floor = 1.14e-15
        par = {"instances": nb, "N": N, "kappa_spread_strict_vs_fma": spread, "kappa_floor": floor,
               "kappa_tolerance": 100 * max(spread, floor), "kappa_kernel_vs_strict": devk,
               "kernel_over_spread": devk / max(spread, floor), "needs_more_than_10x_spread": bool(devk > 10 * max(spread, floor)),
               "radius_rel_kernel_vs_strict": float(np.abs(ref[:nb, :, 5] / strict[..., 5] - 1).max()),
               "xy_m": float(np.abs(ref[:nb, :, :2] - strict[..., :2]).max()),
               "bounds_m": float(np.abs(ref[:nb, :, 9:13] - strict[..., 9:13]).max()),
               "dist_m": float(np.abs(ref[:nb, :, 6:8] - strict[..., 6:8]).max())}
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "parity.json"), "w") as f:
            json.dump(par, f, indent=1)
        print(json.dumps(par))


if __name__ == "__main__":
    main()
