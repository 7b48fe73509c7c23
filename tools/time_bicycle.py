"""Timing of the bicycle min-time NLP solve (include/rl_mincurv.h: rl_bicycle_solve_batch): Monza at the reference
test's 5 m spacing, centre-line initial guess, tol 1e-6, batches of B = 1, 256 and 1024 width-perturbed instances
(tests/bicycle_problem.py: perturbed_widths), plus the CPU twin's seconds per solve.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bicycle_problem as bp  # noqa: E402
import bicycle_twin as bt  # noqa: E402
from spline_trajectory_optimization_amd import ops  # noqa: E402


def main():
    pts, L = bp.monza_table(5.0)
    P0, yaw, dl, dr = bp.table_data(pts)
    N = len(yaw)
    X0, U0, T0 = bt.initial_guess("centerline", P0, yaw)
    out = {"track": "monza", "interval_m": 5.0, "N": N, "tol": 1e-6, "guess": "centerline", "batches": []}
    rep = lambda a, B: np.repeat(a[None], B, axis=0)  # noqa: E731
    for B in [int(b) for b in (sys.argv[1:] or ["1", "256", "1024"])]:
        DL, DR = bp.perturbed_widths(dl, dr, B, seed=11)
        args = (bp.MODEL, P0, yaw, DL, DR, rep(X0, B), rep(U0, B), rep(T0, B))
        ops.bicycle_solve_batch(*args, max_iter=300, tol=1e-6)            # warm-up (scratch, code objects)
        t0 = time.perf_counter()
        X, U, T, st = ops.bicycle_solve_batch(*args, max_iter=300, tol=1e-6)
        ms = (time.perf_counter() - t0) * 1e3
        out["batches"].append({"B": B, "ms": round(ms, 2), "solves_per_s": round(B / ms * 1e3, 1),
                               "iters_mean": float(st[:, 0].mean()), "iters_max": int(st[:, 0].max()),
                               "converged": int((st[:, 5] == 1.0).sum()), "lap_s_mean": float(T.sum(axis=1).mean())})
        print(json.dumps(out["batches"][-1]), file=sys.stderr, flush=True)
    prob = bt.Problem(bp.MODEL, P0, yaw, dl, dr)
    t0 = time.perf_counter()
    _, _, T, st = bt.solve(prob, X0, U0, T0, max_iter=300, tol=1e-6)
    out["cpu_twin_s_per_solve"] = round(time.perf_counter() - t0, 3)
    out["cpu_twin_iters"] = int(st[0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
