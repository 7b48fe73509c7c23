#!/usr/bin/env python3
"""What a change to the exit rule of the global QPs' last linearisation (csrc/rl_device.hpp: kIpmTolLast), or to the kernels
around it (the test hook "global_last_as_mid"), costs: the three global
legs -- one offset per control point, the same with per-sample weights, both coordinates free -- on Monza N = 2000, B = 1024
width-perturbed instances, 6 linearisations, on this build and on another build of the library (the parent commit's), in child
processes that alternate, --rounds each.  Device times from events, one warm-up and three timed calls per leg and child; per leg
the median of the children's medians, the spread of all timed calls, the mean and range of stats[0] (interior-point iterations),
the non-finite outputs, and whether the two builds return the same bits (SHA-256 of out_ctrl and out_stats).  Writes one JSON
file and prints it.

    python tools/time_global_exit.py --compare-lib PARENT.so [--out profiles/global_exit/time_global_exit.json]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from time_vehicle_sweep import load_package  # noqa: E402
from time_weighted_global import MARGIN, N_OUTER, monza, timed_ms  # noqa: E402

LON = 1.0


def child(a):
    _lib, ops = load_package(a.lib)
    import torch
    from spline_trajectory_optimization_amd import batch
    dev = torch.device("cuda", 0)
    trk, w_nom, _ = monza(_lib, ops, a.N)
    W = torch.from_numpy(batch.width_batch(w_nom[:, 0], w_nom[:, 1], a.B, seed=1234)).to(dev)
    wts = torch.from_numpy(1.0 / np.linspace(20.0, 80.0, a.N)).to(dev)
    res = {}
    for leg, kw in (("one_offset", {}), ("weighted", {"weights": wts}), ("xy", {"dof": 2, "lon": LON})):
        out = ops.global_batch_torch(trk, W, MARGIN, N_OUTER, **kw)
        res[leg] = timed_ms(lambda: ops.global_batch_torch(trk, W, MARGIN, N_OUTER, out=out, **kw))
        torch.cuda.synchronize()
        st = out["stats"].cpu().numpy()
        third = out["z" if leg == "xy" else "a"].cpu().numpy()
        res[leg].update(ipm_mean=float(st[:, 0].mean()), ipm_min=float(st[:, 0].min()), ipm_max=float(st[:, 0].max()),
                        non_finite=int((~np.isfinite(third)).any(axis=tuple(range(1, third.ndim))).sum()),
                        max_violation_m=float(st[:, 3].max()),
                        sha256=hashlib.sha256(out["ctrl"].cpu().numpy().tobytes() + st.tobytes()).hexdigest())
    print("LEGS " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_exit", "time_global_exit.json"))
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=None, help="child mode: the three legs on this library, JSON on stdout")
    ap.add_argument("--what", default="the global legs on the parent commit's build and on this one")
    a = ap.parse_args()
    if a.lib:
        return child(a)
    from spline_trajectory_optimization_amd import _lib
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):   # the children run one after the other, each with the GPU to itself
        for who, lib in (("parent", a.compare_lib), ("this", _lib.LIB_PATH)):
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--N", str(a.N), "--B", str(a.B)],
                               capture_output=True, text=True, timeout=600)
            if o.returncode != 0:
                raise RuntimeError(f"child on {lib} failed ({o.returncode}): {o.stderr[-800:]}")
            runs[who].append(json.loads([ln for ln in o.stdout.splitlines() if ln.startswith("LEGS ")][-1][5:]))
    res = {"what": a.what + ": alternating child processes, device events, one warm-up and three timed calls per leg and child",
           "B": a.B, "N": a.N, "n_outer": N_OUTER, "margin_m": MARGIN, "lon_m": LON, "rounds": a.rounds,
           "order": "parent, this, parent, this, ...", "legs": {}}
    for leg in ("one_offset", "weighted", "xy"):
        d = {}
        for who in ("parent", "this"):
            calls = [x for r in runs[who] for x in r[leg]["calls_ms"]]
            d[who] = {"median_of_rounds_ms": float(np.median([r[leg]["median"] for r in runs[who]])),
                      "rounds_median_ms": [r[leg]["median"] for r in runs[who]], "min_ms": float(min(calls)), "max_ms": float(max(calls)),
                      "ipm_mean": runs[who][0][leg]["ipm_mean"], "ipm_min": runs[who][0][leg]["ipm_min"],
                      "ipm_max": runs[who][0][leg]["ipm_max"], "non_finite_instances": runs[who][0][leg]["non_finite"],
                      "max_violation_m": runs[who][0][leg]["max_violation_m"]}
        p, t = d["parent"], d["this"]
        d["time_ratio"] = t["median_of_rounds_ms"] / p["median_of_rounds_ms"]
        d["iteration_ratio"] = t["ipm_mean"] / p["ipm_mean"]
        d["bit_identical_to_parent"] = bool(runs["this"][0][leg]["sha256"] == runs["parent"][0][leg]["sha256"])
        d["parent_spread_rel"] = (p["max_ms"] - p["min_ms"]) / p["median_of_rounds_ms"]
        d["within_iteration_share_plus_parent_spread"] = bool(d["time_ratio"] <= d["iteration_ratio"] + d["parent_spread_rel"])
        res["legs"][leg] = d
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
