"""The QSS simulator's checkers without a GPU: the C oracle (oracle/mincurv_oracle.c: orc_qss_sim) against the REFERENCE's own
Simulator.run_simulation beyond one Monza lap (fixture G15), its two -1 returns, and the dataflow kernel's scheduler rules
(tests/qss_schedule_model.py, window 24 = kDfR) on every input tests/test_qss_gpu.py gives to the kernels.

Tolerances of the value columns are fixture G6's (test_qss_simulator_golden): 1e-12, 1e-11, 1e-12, 1e-14.  Measured on G15: the
oracle returns the reference's speed, lon_acc and lat_acc bit for bit and its time column within 1.2e-16 s."""
import os
import subprocess
import sys

import numpy as np
import pytest

import qss_cases as qc
import qss_schedule_model as model
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G15 = qc.g15_cases()
WINDOW = 24        # kDfR of csrc/rl_qss_df.hpp


@pytest.mark.parametrize("case", G15, ids=[c[0] for c in G15])
def test_oracle_vs_reference_run(case):
    """orc_qss_sim against what the reference's run_simulation returned (G15): owner flags and the iteration count exactly, the
    value columns and the summary to G6's tolerances; -1 where the reference raised."""
    name, pts, veh, exp = case
    out, it = orc.qss_sim(pts, *veh)
    assert it == exp["iters"], (name, it, exp["iters"])
    if exp["raised"]:
        assert it == -1 and exp["raised"].startswith("FloatingPointError"), exp["raised"]
        return
    np.testing.assert_array_equal(out[:, 18], exp["iter_flag"])
    for col, key, tol in qc.VALUE_COLUMNS:
        dev = float(np.abs(out[:, col] - exp[key]).max())
        print(f"{name}: {key} max |oracle - reference| = {dev:.3e} (tolerance {tol:g})")
        assert dev <= tol, (name, key, dev)
    untouched = [c for c in range(19) if c not in (4, 14, 15, 16, 18)]
    np.testing.assert_array_equal(out[:, untouched], pts[:, untouched])
    s = exp["summary"]   # total_time, average_speed, max / min speed, max lat, max / min lon
    assert abs(out[0, 16] - s[0]) <= 1e-14 and abs(out[:, 4].max() - s[2]) <= 1e-12 and abs(out[:, 4].min() - s[3]) <= 1e-12
    assert abs(out[:, 15].max() - s[4]) <= 1e-12 and abs(out[:, 14].max() - s[5]) <= 1e-11 and abs(out[:, 14].min() - s[6]) <= 1e-11


def test_g15_covers_what_it_is_for():
    """The fixture's cases are in the regimes they were made for (a regenerated fixture that lost one would pin nothing new)."""
    by = {c[0]: c for c in G15}
    assert len(by["kart_N400"][1]) == 400 and len(by["kart_N200"][1]) == 200
    name, pts, veh, exp = by["kart_N400_tab43_v120_j10"]
    assert len(veh[0]) == 5 and len(veh[2]) == 4 and veh[4][4] == 120.0 and veh[4][5] == 10.0
    # the kart never gets beyond 43 m/s, but every front's first step starts from min(calc_v, max_speed): on the straights that is
    # beyond the last breakpoint (100 m/s), so iteration 0 evaluates the extrapolated piece at more than 100 samples
    v0 = np.minimum(np.sqrt(15.0 * pts[:, 5]), 120.0)
    assert (v0 > veh[0][-1]).sum() > 100 and exp["speed"].max() < 50.0
    name, pts, veh, exp = by["monza_N320_bank_pm9"]
    assert pts[:, 13].min() < 0.0 < pts[:, 13].max()
    name, pts, veh, exp = by["monza_N320_v40"]
    assert (exp["speed"] == 40.0).sum() > len(pts) // 4             # the cap binds
    assert all((exp_["iter_flag"] >= 0).all() for _, _, _, exp_ in G15 if not exp_["raised"])
    assert sum(1 for c in G15 if c[3]["raised"]) == 1


@pytest.mark.parametrize("N", qc.SIZES)
@pytest.mark.parametrize("veh", qc.VEHICLES)
def test_oracle_returns_minus_one_where_the_reference_raises(N, veh):
    """A zero turn radius: a zero speed, and the step that divides by it (simulator.py:165 under np.seterr(all='raise')).  With the
    4/3-piece tables `seam1` ends the same way: braking from 100 m/s the deceleration table gives -21 m/s^2, beyond max_lon_dcc,
    the friction ellipse leaves no lateral acceleration, and 0 * inf (infinite radius) is not a number."""
    out, it = orc.qss_sim(qc.synthetic("zero", N), *qc.vehicle(veh))
    assert it == -1
    out, it = orc.qss_sim(qc.synthetic("seam1", N), *qc.vehicle(veh))
    assert (it == -1) == (veh == "43p"), (veh, it)


def test_oracle_gives_up_on_the_circle():
    """Constant radius: every front rewrites its neighbour's speed with the same value and the reference never returns.  The oracle
    returns -1 after 16 N + 64 global iterations, as rl_mincurv.h documents for the kernels (measured: 0.14 - 0.23 s per call).
    In a child process with a time limit: a regression fails here instead of hanging the suite."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import qss_cases as qc\nfrom oracle import oracle as orc\n"
            "for N in qc.SIZES:\n    for v in qc.VEHICLES:\n"
            "        out, it = orc.qss_sim(qc.synthetic('circle', N), *qc.vehicle(v))\n        print('circle', N, v, it)\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-1500:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("circle")]
    assert len(lines) == len(qc.SIZES) * len(qc.VEHICLES) and all(ln[3] == "-1" for ln in lines), out.stdout


@pytest.fixture(scope="module")
def modelled():
    """Every input of the GPU tests that the oracle finishes, replayed under the scheduler's rules: label -> (iterations, result)."""
    return {lab: v for lab, v in qc.model_all(WINDOW).items() if v[1] is not None}


def test_schedule_model_on_every_gpu_input(modelled):
    """No violated dependency, no pass without progress, the reference's numbering of spawned fronts (model.run asserts all three)
    and its iteration count; the inputs reach what they were built for.  Prints how often each rule decided an examination."""
    print(model.rule_table([(lab, r["rules"]) for lab, (it, r) in modelled.items()]))
    for lab, (it, r) in modelled.items():
        assert r["iterations"] == it, lab
        assert sum(r["rules"].values()) == r["examinations"] and r["rules"]["ready"] == r["steps"], lab
    finished = {lab for lab, prof, p, v in qc.synthetic_cases() if prof in ("sawtooth", "loguniform", "seam4")}
    finished |= {lab for lab, prof, p, v in qc.synthetic_cases() if prof == "seam1" and lab.endswith("2p")}
    finished |= {n for n, p, v, exp in G15 if not exp["raised"]}
    assert finished == set(modelled)
    for lab, (it, r) in modelled.items():
        if lab.startswith("seam"):
            assert it > 6 * WINDOW and r["rules"]["window"] > 0, (lab, it)      # trains far longer than the iteration window
        if lab.startswith("sawtooth"):
            assert it <= 6 and r["steps"] > 4 * int(lab.split("-N")[1].split("-")[0]), (lab, it)


def test_rule_about_fronts_not_yet_born_fires(modelled):
    """csrc/rl_qss_df.hpp says of this rule that it never fires on real profiles.  It decides examinations on the kart line, on the
    capped Monza lap and on the pinned members of the loguniform family -- which are the FIRST seeds of a search from 0 that
    fire it (at most 200 are tried; the search stops at the pinned seed)."""
    fired = {lab: sum(r["rules"][k] for k in model.UNBORN) for lab, (it, r) in modelled.items()}
    for v, seed in qc.UNBORN_PINNED:
        assert fired[f"loguniform-N320-{v}-seed{seed}"] > 0
    assert fired["kart_N400"] > 0 and fired["monza_N320_v40"] > 0
    found = qc.unborn_rule_search(max_seeds=200)
    assert {v: found[v][0] for v in found if found[v]} == dict(qc.UNBORN_PINNED), found
