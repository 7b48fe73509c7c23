"""Inputs of the vehicle-sweep tests (rl_qss_sim_vehicles_*: one vehicle per instance), shared by tests/test_vehicle_sweep_cpu.py
and tests/test_vehicle_sweep_gpu.py.

Tables: the synthetic family of tests/qss_cases.py -- sawtooth at N = 256, loguniform (seed 7) at N = 319, seam4 at N = 320 -- and
for the mixed batch sawtooth, loguniform and seam4 at N = 320.

Vehicles: six, derived from each of qss_cases' two lookups ("2p": the kernels' register path, "43p": their LDS path) by a grip g
and a power p -- acc values x p, dcc values x g, params = (10 g, -20 g, 15 g, -15 g, vmax, jerk).  Vehicle 0 is qss_cases' own.

What the strict CPU oracle and the schedule model (tests/qss_schedule_model.py, window 24) say about them is pinned in
tests/test_vehicle_sweep_cpu.py; the GPU tests give the kernels nothing that has not passed model_all() first."""
import numpy as np

import qss_cases as qc

#        g    p    vmax   jerk
GRID = ((1.0, 1.0, 100.0, 30.0),
        (0.8, 1.0, 100.0, 30.0),
        (1.2, 0.7, 100.0, 30.0),
        (1.0, 1.0, 60.0, 30.0),
        (1.0, 1.3, 100.0, 10.0),
        (0.6, 0.5, 45.0, 50.0))
NV = len(GRID)
TAGS = qc.VEHICLES                                                   # "2p", "43p"
INPUTS = (("sawtooth", 256), ("loguniform", 319), ("seam4", 320))    # one batch each: the same table under the six vehicles
MIXED = (("sawtooth", 0), ("loguniform", 5), ("seam4", 2))           # (profile, vehicle) of the mixed batch, all N = 320
MIXED_N = 320
RAISES = {("seam4", 1), ("seam4", 4)}                                # (profile, vehicle) on which the reference raises, both lookups
# iterations of the oracle with the "2p" lookups, vehicles 0 - 5
ITERS_2P = {"sawtooth": (6, 3, 6, 6, 4, 3), "loguniform": (9, 19, 19, 9, 10, 12), "seam4": (227, -1, 253, 204, -1, 263)}
LOGUNIFORM_LAP_TIMES_2P = (39.8, 50.8)                               # s, fastest and slowest of the six, to 0.1 s


def vehicle(tag, v):
    """Vehicle v of the grid on lookup `tag`: the 5-tuple rl_qss_sim takes."""
    ax, av, dx, dv = qc.LOOKUPS[tag]
    g, p, vmax, jerk = GRID[v]
    return qc.vehicle_from_lookups(np.column_stack([ax, np.asarray(av) * p]), np.column_stack([dx, np.asarray(dv) * g]),
                                   (10.0 * g, -20.0 * g, 15.0 * g, -15.0 * g, vmax, jerk))


def vehicles(tag):
    return [vehicle(tag, v) for v in range(NV)]


def table(profile, N):
    return qc.synthetic(profile, N, qc.LOGUNIFORM_SEED)


def label(profile, N, tag, v):
    return f"{profile}-N{N}-{tag}-v{v}"


def single_runs():
    """(label, profile, vehicle index, points, vehicle) of every (table, vehicle) pair the GPU tests run."""
    out = []
    for tag in TAGS:
        for prof, N in INPUTS:
            out += [(label(prof, N, tag, v), prof, v, table(prof, N), vehicle(tag, v)) for v in range(NV)]
        out += [(label(prof, MIXED_N, tag, v), prof, v, table(prof, MIXED_N), vehicle(tag, v)) for prof, v in MIXED]
    return out


def model_all(window=24):
    """Every pair of single_runs() through the oracle and, where it finishes, through the scheduler's rules:
    label -> (iterations, result of qss_schedule_model.run | None).  run() raises on a violated dependency, a pass without
    progress or a numbering that differs from the reference's."""
    import tempfile
    import qss_schedule_model as model
    res = {}
    with tempfile.TemporaryDirectory() as wd:
        lib = model.build_logging_oracle(wd)
        for lab, prof, v, pts, veh in single_runs():
            it, lg = model.step_log(lib, pts, veh)
            if lg is None:
                assert it == -1, lab
                res[lab] = (-1, None)
                continue
            r = model.run(lg, len(pts), window)
            assert r["iterations"] == it, lab
            res[lab] = (it, r)
    return res
