"""Test helper: bicycle min-time problem data built on the CPU with scipy + the C oracle -- the reference test's
Monza set-up (tests/test_min_time_optm.py:56-63: centre line bspline s = 3.0, k = 5, sampled every `interval`
metres; RaceTrack boundaries as splines s = 10, k = 3 sampled every 2 m, fill_trajectory_boundaries) and a ring."""
import os
import warnings

import numpy as np
from scipy import integrate, interpolate
from scipy.interpolate import splprep

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONZA = os.path.join(ROOT, "spline_trajectory_optimization_amd", "examples", "race_track", "monza")
MODEL = {"lr": 1.5, "L": 3.0, "delta_max": 0.314158999998341, "v_max": 80.0, "a_lon_max": 20.0, "a_lon_min": -20.0,
         "delta_dot_max": 1.0, "acc_max": 20.0}     # tests/test_min_time_optm.py:69-78


def _load(name):
    return np.loadtxt(os.path.join(MONZA, name), delimiter=",", skiprows=1, usecols=(0, 1))


def _sample(pts, s, k, interval):
    loop = np.vstack([pts, pts[:1]])
    (t, c, kk), _ = splprep([loop[:, 0], loop[:, 1]], s=s, per=True, k=k)
    speed = lambda u: np.hypot(interpolate.splev(u, (t, c[0], kk), der=1), interpolate.splev(u, (t, c[1], kk), der=1))  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        L, _ = integrate.quad(speed, 0, 1, limit=1000)
    n = int(L // interval)
    return orc.sample_along(t, c[0], c[1], kk, L, np.linspace(0, 1, n, endpoint=False)), L


def monza_table(interval=5.0):
    """The reference test's traj_d [N,19] with bounds filled, and the centre line's length."""
    pts, L = _sample(_load("MONZA_UNOPTIMIZED_LINE_enu.csv"), 3.0, 5, interval)
    ringL, _ = _sample(_load("MONZA_LEFT_BOUNDARY_enu.csv"), 10.0, 3, 2.0)
    ringR, _ = _sample(_load("MONZA_RIGHT_BOUNDARY_enu.csv"), 10.0, 3, 2.0)
    orc.fill_bounds(pts, np.ascontiguousarray(ringL[:, :2]), np.ascontiguousarray(ringR[:, :2]), 100.0)
    return pts, L


def table_data(pts):
    """P0 [N,2], yaw [N], dl [N] > 0, dr [N] < 0 as set_up_bicycle_problem derives them (:26-31, :66-67)."""
    P0 = pts[:, 0:2].copy()
    dl = np.hypot(pts[:, 9] - pts[:, 0], pts[:, 10] - pts[:, 1])
    dr = -np.hypot(pts[:, 11] - pts[:, 0], pts[:, 12] - pts[:, 1])
    return P0, pts[:, 3].copy(), dl, dr


def ring_table(N, R=100.0, left=4.0, right=4.0):
    """Counter-clockwise circle of centre radius R: the left bound is the inner one."""
    ang = np.arange(N) * 2 * np.pi / N
    pts = np.zeros((N, 19))
    pts[:, 0], pts[:, 1] = R * np.cos(ang), R * np.sin(ang)
    pts[:, 3] = np.arctan2(np.cos(ang), -np.sin(ang))
    pts[:, 9], pts[:, 10] = (R - left) * np.cos(ang), (R - left) * np.sin(ang)
    pts[:, 11], pts[:, 12] = (R + right) * np.cos(ang), (R + right) * np.sin(ang)
    return pts


def oval_table(N, a=120.0, b=60.0, w=5.0):
    """Closed ellipse-like oval with half-width w on both sides."""
    ang = np.arange(N) * 2 * np.pi / N
    x, y = a * np.cos(ang), b * np.sin(ang)
    tx, ty = -a * np.sin(ang), b * np.cos(ang)
    nrm = np.hypot(tx, ty)
    nx_, ny_ = -ty / nrm, tx / nrm
    pts = np.zeros((N, 19))
    pts[:, 0], pts[:, 1], pts[:, 3] = x, y, np.arctan2(ty, tx)
    pts[:, 9], pts[:, 10] = x + w * nx_, y + w * ny_
    pts[:, 11], pts[:, 12] = x - w * nx_, y - w * ny_
    return pts


def perturbed_widths(dl, dr, B, seed=0, amp=0.1):
    """B width sets: both distances scaled by smooth random factors in [1 - amp, 1 + amp]."""
    rng = np.random.default_rng(seed)
    N = len(dl)
    s = np.arange(N) * 2 * np.pi / N
    fl = np.ones((B, N)); fr = np.ones((B, N))
    for h in (1, 2, 3):
        fl += amp / 3 * np.sin(h * s[None] + rng.uniform(0, 2 * np.pi, (B, 1)))
        fr += amp / 3 * np.sin(h * s[None] + rng.uniform(0, 2 * np.pi, (B, 1)))
    return dl[None] * fl, dr[None] * fr
