"""Python time per call of the two ops wrappers with the most logic, solve_batch_host and tables_host, against the stand-in
library of tests/ops_call_recorder.py (no device, no kernel): medians and ranges over repeats, one JSON line.  Several
checkouts are timed in ONE process, their repeats alternating, so that they share whatever the host does meanwhile.

    python tools/time_ops_wrappers.py --root CHECKOUT_A [--root CHECKOUT_B ...] [--calls 4000] [--repeats 5]
"""
import argparse
import contextlib
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import ops_call_recorder as rec  # noqa: E402


def load(root):
    """The package of one checkout, imported under its usual name (whatever was imported under it before is dropped)."""
    for name in [m for m in sys.modules if m.split(".")[0] == "spline_trajectory_optimization_amd"]:
        del sys.modules[name]
    sys.path.insert(0, root)
    try:
        pkg = importlib.import_module("spline_trajectory_optimization_amd")
        importlib.import_module("spline_trajectory_optimization_amd.ops")
    finally:
        sys.path.remove(root)
    return pkg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", action="append", required=True, help="checkout whose package is timed (repeatable)")
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    widths, ctrl0 = rec._arr((rec.B, rec.N, 2), 40), rec._arr((rec.B, rec.N_CTRL, 2), 41)
    rows = [[1, 2, 3], [4, 3, 2]]
    cases = {}
    with contextlib.ExitStack() as stack:
        for root in a.root:
            pkg = load(root)
            ops, L = pkg.ops, pkg._lib
            _, track = stack.enter_context(rec.stand_in(pkg, record=False))
            cases[root, "solve_batch_host"] = lambda ops=ops, L=L, track=track: ops.solve_batch_host(
                track, L.BOUNDS_WIDTHS, widths, rows, ctrl0=ctrl0, driver="window")
            cases[root, "tables_host"] = lambda ops=ops, L=L, track=track: ops.tables_host(track, ctrl0, L.BOUNDS_WIDTHS, widths, 123.5)
        us = {key: [] for key in cases}
        for _ in range(a.repeats + 1):   # the first repeat warms up
            for key, fn in cases.items():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                us[key].append((time.perf_counter() - t0) / a.calls * 1e6)
    out = {root: {} for root in a.root}
    for (root, name), v in us.items():
        v = v[1:]
        out[root][name] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "range_us": max(v) - min(v)}
    print(json.dumps({"calls": a.calls, "repeats": a.repeats, "per_call": out}))


if __name__ == "__main__":
    main()
