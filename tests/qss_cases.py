"""Inputs of the QSS simulator tests, shared by tests/test_qss_cpu.py and tests/test_qss_gpu.py.

  * g15_cases(): fixture G15 -- Simulator.run_simulation of the REFERENCE on the kart centre line (N = 400: the dataflow kernel's
    size; N = 200: the list order's), with 4/3-piece lookup tables, max_speed beyond the last breakpoint and max_jerk = 10, on
    Monza with a bank column of both signs and with a speed cap that binds on every straight, and on a table with a zero turn
    radius (the reference raises).
  * synthetic(profile, N): tables built directly, no spline: X, Y at uniform 2 m spacing on a circle of circumference 2 N m, a
    radius column per profile, bank 0.  Every input so far was the Monza fit with its apexes in the same places; these put
    them where the scheduler's tables wrap (trains across the start line, N mod 64 = 63), make hundreds of one-sample apexes,
    a few very long trains, and an infinite radius over most of the lap.

A vehicle is the 5-tuple (acc_x, acc_c, dcc_x, dcc_c, params) rl_qss_sim takes."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# the two vehicles of tools/validate_qss.py: 2 pieces (the kernels' register path) and 4 / 3 pieces (their LDS path)
LOOKUPS = {
    "2p": ([0.0, 50.0, 100.0], [10.0, 7.0, 0.5], [0.0, 50.0, 100.0], [-13.0, -15.0, -20.0]),
    "43p": ([0.0, 20.0, 45.0, 70.0, 100.0], [11.0, 9.0, 6.0, 3.0, 0.4], [0.0, 30.0, 60.0, 100.0], [-12.0, -14.0, -17.0, -21.0]),
}
PARAMS = (10.0, -20.0, 15.0, -15.0, 100.0, 30.0)   # max lon acc / dcc, max left / right acc, max speed, max jerk (fixture G6's)
VEHICLES = tuple(LOOKUPS)

PROFILES = ("sawtooth", "loguniform", "seam1", "seam4", "zero", "circle")
SIZES = (256, 319, 320)          # the smallest the dataflow kernel takes; N mod 64 = 63; a multiple of 64
LOGUNIFORM_SEED = 7              # the default member of the loguniform family
# members of the loguniform family (N = 320) on which the scheduler's rule about fronts NOT YET BORN decides an examination:
# found by unborn_rule_search() below; DESIGN.md records the search
UNBORN_PINNED = (("2p", 16), ("43p", 16))


def vehicle_from_lookups(acc_lookup, dcc_lookup, params):
    from scipy.interpolate import CubicSpline
    acc_lookup, dcc_lookup = np.asarray(acc_lookup, dtype=np.float64), np.asarray(dcc_lookup, dtype=np.float64)
    acc, dcc = CubicSpline(acc_lookup[:, 0], acc_lookup[:, 1]), CubicSpline(dcc_lookup[:, 0], dcc_lookup[:, 1])
    return (np.ascontiguousarray(acc.x), np.ascontiguousarray(acc.c), np.ascontiguousarray(dcc.x), np.ascontiguousarray(dcc.c),
            np.asarray(params, dtype=np.float64))


def vehicle(tag):
    ax, av, dx, dv = LOOKUPS[tag]
    return vehicle_from_lookups(np.column_stack([ax, av]), np.column_stack([dx, dv]), PARAMS)


def table(cols_in):
    """[N,19] Trajectory table from the six columns the fixtures store (X, Y, turn radius, distances, bank)."""
    N = len(cols_in)
    pts = np.zeros((N, 19))
    pts[:, [0, 1, 5, 6, 7, 13]] = cols_in
    pts[:, 17] = np.arange(N)
    pts[:, 18] = -1
    return pts


def radius_profile(profile, N, seed=LOGUNIFORM_SEED):
    r = np.full(N, np.inf)
    if profile == "sawtooth":            # every other sample an apex
        r[:] = 900.0
        r[0::2] = 15.0
    elif profile == "loguniform":
        r = np.exp(np.random.default_rng(seed).uniform(np.log(8.0), np.log(3000.0), N))
    elif profile == "seam1":             # one apex at the last sample: its trains run across the start line
        r[N - 1] = 12.0
    elif profile == "seam4":             # an apex of four samples astride the start line
        r[[N - 2, N - 1, 0, 1]] = [30.0, 12.0, 12.0, 30.0]
    elif profile == "zero":              # the reference raises: division by a zero speed
        r[:] = 200.0
        r[N // 3] = 0.0
    elif profile == "circle":            # the reference never returns: every front rewrites its neighbour for ever
        r[:] = 80.0
    else:
        raise ValueError(profile)
    return r


def synthetic(profile, N, seed=LOGUNIFORM_SEED):
    ang = 2.0 * np.pi * np.arange(N) / N
    R = 2.0 * N / (2.0 * np.pi)          # 2 m of arc per sample
    s = 2.0 * np.arange(N)
    cols = np.column_stack([R * np.cos(ang), R * np.sin(ang), radius_profile(profile, N, seed), s, 2.0 * N - s, np.zeros(N)])
    return table(cols)


def synthetic_cases(profiles=PROFILES, sizes=SIZES, vehicles=VEHICLES):
    """(label, profile, points, vehicle) for every profile x size x vehicle, then the pinned loguniform members."""
    out = []
    for prof in profiles:
        for N in sizes:
            for v in vehicles:
                out.append((f"{prof}-N{N}-{v}", prof, synthetic(prof, N), vehicle(v)))
    if "loguniform" in profiles:
        for v, seed in UNBORN_PINNED:
            out.append((f"loguniform-N320-{v}-seed{seed}", "loguniform", synthetic("loguniform", 320, seed), vehicle(v)))
    return out


def g15_cases():
    """(name, points, vehicle, expected) per case of fixture G15; expected: iters, raised (text, '' = no), and for a case that
    did not raise speed / lon_acc / lat_acc / time / iter_flag / summary."""
    g = np.load(os.path.join(HERE, "golden", "G15_simulator_cases.npz"))
    out = []
    for name in [str(n) for n in g["names"]]:
        exp = {"iters": int(g[f"{name}_iters"]), "raised": str(g[f"{name}_raised"])}
        if not exp["raised"]:
            for k in ("speed", "lon_acc", "lat_acc", "time", "iter_flag", "summary"):
                exp[k] = g[f"{name}_{k}"]
        veh = vehicle_from_lookups(g[f"{name}_acc_lookup"], g[f"{name}_dcc_lookup"], g[f"{name}_params"])
        out.append((name, table(g[f"{name}_cols_in"]), veh, exp))
    return out


# the written columns and the tolerances test_qss_simulator_golden holds fixture G6 to
VALUE_COLUMNS = ((4, "speed", 1e-12), (14, "lon_acc", 1e-11), (15, "lat_acc", 1e-12), (16, "time", 1e-14))


# ---- what k_qss_dfw says when it gives an instance back, visible with the test hook "qss_df_redo" = 0 (include/rl_mincurv.h)
HANDED_BACK = -100               # RL_QSS_HANDED_BACK: iters = HANDED_BACK - reason
REASONS = {2: "an agent beyond iteration N - 1", 3: "more unnumbered fronts than the scratch holds", 4: "no free exit record",
           5: "front ids beyond the table", 6: "SCHEDULER: empty queue with live agents", 7: "the hook qss_df_bail_at",
           8: "SCHEDULER: window-counter guard", 9: "SCHEDULER: more than 3 N + 64 passes per iteration"}
CAPACITY_REASONS = (2, 3, 4, 5)


def hand_back_reasons(iters):
    """Per instance: 0 = not handed back, else the reason code."""
    it = np.atleast_1d(np.asarray(iters)).astype(np.int64)
    return np.where(it <= HANDED_BACK, HANDED_BACK - it, 0)


def assert_not_handed_back(iters, label, allowed=0):
    """With redo off no instance may come back from the dataflow kernel, except for the capacity reason `allowed` that the
    caller names in advance for this input.  The reason code is in the message."""
    assert allowed == 0 or allowed in CAPACITY_REASONS
    for b, reason in enumerate(hand_back_reasons(iters)):
        reason = int(reason)
        assert reason == allowed, (f"{label}: instance {b} was handed back by k_qss_dfw with reason {reason} "
                                   f"({REASONS.get(reason, 'unknown')}); expected " +
                                   (f"reason {allowed}" if allowed else "no hand-back"))


def model_all(window=24):
    """Every input of the GPU tests that the oracle finishes (all but `circle`, `zero`, the G15 raise case and `seam1` with the
    4/3-piece tables), replayed under the scheduler's rules: label -> (iterations, result of qss_schedule_model.run).  run()
    raises on a violated dependency, a pass without progress or a numbering that differs from the reference's."""
    import tempfile
    import qss_schedule_model as model
    res = {}
    with tempfile.TemporaryDirectory() as wd:
        lib = model.build_logging_oracle(wd)      # also checks that the model's substitutions still apply to the oracle's source
        inputs = [(lab, p, v) for lab, prof, p, v in synthetic_cases() if prof != "circle"] + [(n, p, v) for n, p, v, _ in g15_cases()]
        for lab, pts, veh in inputs:
            it, lg = model.step_log(lib, pts, veh)
            if lg is None:
                assert it == -1, lab
                res[lab] = (-1, None)
                continue
            r = model.run(lg, len(pts), window)
            assert r["iterations"] == it, lab
            res[lab] = (it, r)
    return res


def unborn_rule_search(max_seeds=200, N=320, window=24, log=print):
    """The first loguniform seed per vehicle on which the schedule model reports that the rule about fronts not yet born
    decided an examination (None when no seed up to max_seeds does).   python tests/qss_cases.py"""
    import tempfile
    import qss_schedule_model as model
    found = {}
    with tempfile.TemporaryDirectory() as wd:
        lib = model.build_logging_oracle(wd)
        for v in VEHICLES:
            found[v] = None
            for seed in range(max_seeds):
                it, lg = model.step_log(lib, synthetic("loguniform", N, seed), vehicle(v))
                if lg is None:
                    continue
                res = model.run(lg, N, window)
                n = sum(res["rules"][r] for r in model.UNBORN)
                if n:
                    found[v] = (seed, n, it)
                    log(f"vehicle {v}: seed {seed} fires the rule {n} times ({it} iterations)")
                    break
            else:
                log(f"vehicle {v}: 0 firings over seeds 0 .. {max_seeds - 1}")
    return found


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    unborn_rule_search()
