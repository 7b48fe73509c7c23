#!/usr/bin/env python3
"""Do two builds of the library return the same bytes from the global min-curvature QP?  The five dispatch shapes of
tests/test_weighted_global_gpu.py -- R = 5 / 6 with one group (c100 N = 500), R = 10 (c100 N = 4000), three groups (c30
N = 2000), degree 3 (l10 N = 1000), the generic kernel (c100 N = 500 on a context created under RL_GLOBAL_V1=1) -- at B = 4
width-perturbed instances, each unweighted and with the weights 1 / linspace(20, 80, N), through the device entry.  One fresh
child process per library (as tools/time_weighted_global.py); ctrl, xy, a and stats are compared byte for byte.

    python tools/global_ab_bits.py --compare-lib PARENT.so [--out profiles/global_templates/ab_bits.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from time_vehicle_sweep import load_package  # noqa: E402

MARGIN, B = 0.25, 4
SHAPES = [("rows5or6_one_group", "c100", 500, 6, False), ("rows10", "c100", 4000, 6, False), ("three_groups", "c30", 2000, 3, False),
          ("degree3", "l10", 1000, 2, False), ("generic", "c100", 500, 6, True)]
OUTPUTS = ("ctrl", "xy", "a", "stats")


def child(lib_path, dump):
    _lib, ops = load_package(lib_path)
    import torch
    from spline_trajectory_optimization_amd import batch
    dev = torch.device("cuda", 0)
    os.environ["RL_GLOBAL_V1"] = "1"     # read once, in rl_ctx_create
    v1 = _lib.Context(0)
    del os.environ["RL_GLOBAL_V1"]
    g = np.load(os.path.join(ROOT, "tests", "golden", "G1_spline_fits.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "G1_rings.npz"))
    res = {}
    for name, tag, N, n_outer, generic in SHAPES:
        t, cx, cy, k, length = g[f"{tag}_t"], g[f"{tag}_cx"], g[f"{tag}_cy"], int(g[f"{tag}_k"]), float(g[f"{tag}_length"])
        if tag == "l10":  # the boundary fit: synthetic widths, as the tests
            wl, wr = np.full(N, 4.0) + np.sin(np.arange(N) * 0.05), np.full(N, 3.0) + np.cos(np.arange(N) * 0.03)
        else:
            pts = ops.fill_bounds(ops.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False)), r["ringL"], r["ringR"])
            wl, wr = batch.half_widths_from_bounds(pts)
        trk = _lib.Track(v1 if generic else _lib.Context.get(0), t, cx, cy, k, N)
        W = torch.from_numpy(batch.width_batch(wl, wr, B, seed=3)).to(dev)
        wts = torch.from_numpy(np.ascontiguousarray(np.tile(1.0 / np.linspace(20.0, 80.0, N), (B, 1)))).to(dev)
        for leg, w in (("unweighted", None), ("weighted", wts)):
            out = ops.global_batch_torch(trk, W, MARGIN, n_outer, weights=w)
            torch.cuda.synchronize()
            res[f"{name}/{leg}/block_threads"] = np.array(int(out["rl_stats"].block_threads))
            for o in OUTPUTS:
                res[f"{name}/{leg}/{o}"] = out[o].cpu().numpy()
    np.savez(dump, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_templates", "ab_bits.json"))
    ap.add_argument("--lib", default=None, help="child mode: the library to run")
    ap.add_argument("--dump", default=None, help="child mode: where the outputs go (.npz)")
    a = ap.parse_args()
    if a.dump:
        return child(a.lib, a.dump)
    from spline_trajectory_optimization_amd import _lib
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for who, lib in (("other", a.compare_lib), ("this", _lib.LIB_PATH)):
            dump = os.path.join(tmp, who + ".npz")
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--dump", dump], capture_output=True,
                               text=True, timeout=600)
            if o.returncode != 0:
                raise RuntimeError(f"child on {lib} failed ({o.returncode}): {o.stderr[-800:]}")
            with np.load(dump) as z:
                got[who] = {k_: z[k_] for k_ in z.files}
    res = {"B": B, "margin_m": MARGIN, "weights": "1 / linspace(20, 80, N), every instance", "entry": "ops.global_batch_torch (_dev)",
           "shapes": {}}
    for name, tag, N, n_outer, generic in SHAPES:
        s = res["shapes"][name] = {"spline": tag, "N": N, "n_outer": n_outer, "RL_GLOBAL_V1": int(generic)}
        for leg in ("unweighted", "weighted"):
            this, other = ({o: got[w][f"{name}/{leg}/{o}"] for o in OUTPUTS + ("block_threads",)} for w in ("this", "other"))
            s[leg] = {"block_threads": int(this["block_threads"]), "ipm_iterations": [int(x) for x in this["stats"][:, 0]],
                      "finite": bool(all(np.isfinite(this[o]).all() for o in OUTPUTS)),
                      "equal_bytes": {o: this[o].tobytes() == other[o].tobytes() for o in OUTPUTS}}
        s["weighted_line_differs_from_unweighted"] = got["this"][f"{name}/weighted/xy"].tobytes() != got["this"][f"{name}/unweighted/xy"].tobytes()
    res["all_equal"] = all(all(s[leg]["equal_bytes"].values()) and s[leg]["finite"] for s in res["shapes"].values()
                           for leg in ("unweighted", "weighted"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if res["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
