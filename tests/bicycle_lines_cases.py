"""Shared case data of the per-instance bicycle tests (rl_bicycle_solve_lines*): five ovals of N = 48, each with its own
line and its own model; three rings of N = 64 with an analytic optimum; one-parameter changes of the model on the first
oval that each move the optimum visibly.  The CPU twin (tests/bicycle_twin.py) takes one instance at a time; its solutions
are computed once per process and shared (twin_solution)."""
import functools

import numpy as np

import bicycle_problem as bp
import bicycle_twin as bt

MODEL = bp.MODEL
N_OVAL, N_RING = 48, 64


def moved(pts, angle=0.0, shift=(0.0, 0.0)):
    """A table rotated by `angle` about the origin, then shifted: the line, its bounds and its headings (kept in (-pi, pi])."""
    out = pts.copy()
    c, s = np.cos(angle), np.sin(angle)
    for ix in (0, 9, 11):
        x, y = pts[:, ix], pts[:, ix + 1]
        out[:, ix], out[:, ix + 1] = c * x - s * y + shift[0], s * x + c * y + shift[1]
    out[:, 3] = np.arctan2(np.sin(pts[:, 3] + angle), np.cos(pts[:, 3] + angle))
    return out


def model(**changes):
    return dict(MODEL, **changes)


# (table, model): the five instances of one mixed batch
OVALS = (
    (bp.oval_table(N_OVAL, 120.0, 60.0, 5.0), model()),
    (moved(bp.oval_table(N_OVAL, 90.0, 70.0, 4.0), 0.6, (300.0, -200.0)), model(acc_max=12.0)),
    (moved(bp.oval_table(N_OVAL, 150.0, 50.0, 6.0), -1.1, (-50.0, 80.0)), model(v_max=30.0)),
    (bp.oval_table(N_OVAL, 120.0, 60.0, 5.0), model(L=2.6, lr=1.2, a_lon_max=6.0, a_lon_min=-10.0)),
    (moved(bp.oval_table(N_OVAL, 100.0, 40.0, 5.0), 2.0), model(delta_max=0.1, delta_dot_max=0.3)),
)
# the twin's converged laps [s] from the centre-line guess at tol 1e-6 (23 to 28 iterations)
OVAL_LAPS = (13.778620, 15.988490, 22.439058, 14.573535, 12.706613)

# (R, acc_max): rings with left = right = 4 m; the optimum is the inner circle at the traction limit
RINGS = ((100.0, 20.0), (60.0, 12.0), (150.0, 8.0))
RING_LAPS = tuple(2.0 * np.pi * np.sqrt((R - 4.0) / a) for R, a in RINGS)   # 13.766, 13.573, 26.842 s


def ring_case(i):
    R, a = RINGS[i]
    return bp.ring_table(N_RING, R, 4.0, 4.0), model(acc_max=a)


# one group of MODEL changed on the first oval -> (changes, sign of lap - base lap, the twin's lap [s]); the L / lr row
# moves the lap only in the fifth digit and is checked on max |delta| instead (0.119 -> 0.103)
BASE_LAP, BASE_MAX_DELTA, LR_MAX_DELTA = 13.778620, 0.1192, 0.1034
PARAM_ROWS = (
    ({"v_max": 25.0}, +1, 22.054480),
    ({"a_lon_max": 5.0}, +1, 14.714835),
    ({"a_lon_min": -5.0}, +1, 14.802012),
    ({"delta_dot_max": 0.05}, +1, 13.816977),
    ({"acc_max": 12.0}, +1, 17.788121),
    ({"delta_max": 0.10}, +1, 13.811430),
    ({"L": 2.6, "lr": 1.2}, 0, 13.778535),
)


def data(pts):
    """P0 [N,2], yaw [N], dl [N], dr [N] of a table, as set_up_bicycle_problem derives them."""
    return bp.table_data(pts)


def stacked(cases):
    """(models, P0 [B,N,2], yaw [B,N], dl [B,N], dr [B,N], X0 [B,N,5], U0 [B,N,2], T0 [B,N]) of (table, model) pairs, the
    centre-line guess on every line."""
    rows = [data(pts) for pts, _ in cases]
    guess = [bt.initial_guess("centerline", r[0], r[1]) for r in rows]
    return ([m for _, m in cases],) + tuple(np.stack(a) for a in zip(*rows)) + tuple(np.stack(a) for a in zip(*guess))


_CASES = {}
for _i, _c in enumerate(OVALS):
    _CASES["oval%d" % _i] = _c
for _i in range(len(RINGS)):
    _CASES["ring%d" % _i] = ring_case(_i)
for _i, (_ch, _, _) in enumerate(PARAM_ROWS):
    _CASES["param%d" % _i] = (OVALS[0][0], model(**_ch))
_CASES["oval70"] = (moved(bp.oval_table(70, 110.0, 55.0, 5.0), 0.3, (10.0, -20.0)), model(acc_max=15.0))


def case(key):
    return _CASES[key]


@functools.lru_cache(maxsize=None)
def twin_solution(key, max_iter=200, tol=1e-6):
    """(prob, X, U, T, stats) of the twin on case `key` from the centre-line guess; computed once per process.  The
    arrays are shared between tests: read only."""
    pts, m = _CASES[key]
    P0, yaw, dl, dr = data(pts)
    prob = bt.Problem(m, P0, yaw, dl, dr)
    X0, U0, T0 = bt.initial_guess("centerline", P0, yaw)
    X, U, T, st = bt.solve(prob, X0, U0, T0, max_iter=max_iter, tol=tol)
    for a in (X, U, T, st):
        a.setflags(write=False)
    return prob, X, U, T, st
