"""Helper of test_mintime_vehicles_gpu.py: in THIS process (whose environment selects the elimination kernel of the library)
solve the MGKT problem for a few iterations for two vehicles, once as one vehicles call and once as two single calls, and
save both.   python mintime_vehicles_run.py out.npz iterations spacing vehicle_a vehicle_b"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import mintime_vehicle_cases as vc  # noqa: E402
from spline_trajectory_optimization_amd import ops  # noqa: E402

out, iters, spacing, names = sys.argv[1], int(sys.argv[2]), float(sys.argv[3]), sys.argv[4:6]
d, X0, U0, T0 = vc.problem(spacing)
ms = vc.models(names)
args = (d["s"], d["kappa"], d["left"], d["right"], vc.margin(ms[0]), d["L"])
kw = dict(average_track_width=vc.defaults.SOLVER["average_track_width"], speed_cap=vc.defaults.SOLVER["speed_cap"],
          max_iter=iters, tol=1e-12)
X, U, T, st = ops.mintime_solve_vehicles(ms, *args, vc.rep(X0, 2), vc.rep(U0, 2), vc.rep(T0, 2), **kw)
single = [ops.mintime_solve_batch(m, *args, X0[None], U0[None], T0[None], **kw) for m in ms]
np.savez(out, X=X, U=U, T=T, st=st, **{f"{k}{b}": single[b][i][0] for b in range(2) for i, k in enumerate(("X", "U", "T", "st"))})
