"""CPU statement of rl_pose_tables_batch_*: RaceTrack.frenet_to_global, the oracle's fill_bounds (orc.fill_bounds; orc.width_rings
for the width form), Trajectory.fill_distance of models/trajectory.py and the TIME roll, composed per instance.  No arithmetic
of its own beyond that composition.  Next to it: a RaceTrack of the MGKT example built without a GPU (the class's own
interpolants over a centre-line table the oracle sampled), and the conditioning figures the GPU tests assert on their inputs."""
import functools

import numpy as np

from mintime_problem import _fit, _load
from oracle import oracle as orc
from spline_trajectory_optimization_amd.models.race_track import RaceTrack, Ring
from spline_trajectory_optimization_amd.models.trajectory import Trajectory

X, Y, YAW, SPEED, BWD, FWD, TIME, IDX, FLAG = 0, 1, 3, 4, 6, 7, 16, 17, 18
BOUND_COLS = [9, 10, 11, 12]
COPIED_COLS = [2, 5, 8, 13, 14, 15, 17, 18]   # from the base table, or the constants of an empty one


def global_table(x, y, yaw, speed, rings, base=None, T=None):
    """One instance from global poses: X / Y / YAW / SPEED into a copy of `base` (an empty Trajectory without one), fill_bounds
    against rings = (ringL, ringR) with max_dist 100, fill_distance, TIME[(i+1) % N] = T[i] when T is given."""
    traj = Trajectory(len(x))
    if base is not None:
        traj.points = np.array(base, dtype=np.float64, copy=True, order="C")
    traj[:, X] = x
    traj[:, Y] = y
    traj[:, YAW] = yaw
    traj[:, SPEED] = speed
    orc.fill_bounds(traj.points, np.ascontiguousarray(rings[0]), np.ascontiguousarray(rings[1]), 100.0)
    traj.fill_distance()
    if T is not None:
        traj[:, TIME] = np.roll(T, 1)
    return traj.points


def frenet_table(race_track, Xb, rings, base=None, T=None):
    """One instance from Xb [N,6] = (s, n, xi, ., ., v) in race_track's curvilinear frame."""
    pose = np.asarray(race_track.frenet_to_global(Xb[:, 0], Xb[:, 1], Xb[:, 2]))
    return global_table(pose[:, 0], pose[:, 1], pose[:, 2], Xb[:, 5], rings, base, T)


def tables(race_track, Xs, rings, base=None, T=None):
    """Xs [B,N,6] (race_track given) or [B,N,5] global poses (race_track None); rings one pair or a list of B pairs; base None,
    [N,19] or [B,N,19]; T None or [B,N]."""
    out = []
    for b in range(len(Xs)):
        rg = rings[b] if isinstance(rings, list) else rings
        bs = None if base is None else (base[b] if np.ndim(base) == 3 else base)
        tb = None if T is None else T[b]
        out.append(frenet_table(race_track, Xs[b], rg, bs, tb) if race_track is not None else
                   global_table(Xs[b][:, 0], Xs[b][:, 1], Xs[b][:, 2], Xs[b][:, 4], rg, bs, tb))
    return np.stack(out)


def width_rings(t, cx0, cy0, k, N, widths):
    return orc.width_rings(t, cx0, cy0, k, N, np.ascontiguousarray(widths))


# ---------------------------------------------------------------- the MGKT example without a GPU
class _Length:
    def __init__(self, length):
        self._length = float(length)

    def get_length(self):
        return self._length


@functools.lru_cache(maxsize=None)
def mgkt_fits():
    """{"c" | "l" | "r": (t, cx, cy, k, length)}: the k = 3 fits RaceTrack(..., s=1.0) makes of the MGKT example."""
    files = {"c": "MGKT_CENTER_enu.csv", "l": "MGKT_OUT_BOUND_enu.csv", "r": "MGKT_IN_BOUND_enu.csv"}
    return {name: _fit(_load(f), 1.0, 3) for name, f in files.items()}


def mgkt_ring(side, n):
    """[n,2]: the boundary fit `side` ("l" | "r") sampled at n uniform parameters."""
    t, cx, cy, k, L = mgkt_fits()[side]
    return np.ascontiguousarray(orc.sample_along(t, cx, cy, k, L, np.linspace(0, 1, n, endpoint=False))[:, :2])


@functools.lru_cache(maxsize=None)
def mgkt_race_track(interval=8.0):
    """RaceTrack("MGKT", ..., s=1.0, interval) as tests/mintime_problem.mgkt_problem samples it: the tables from the oracle
    instead of the HIP kernels, the interpolants the class's own."""
    fits = mgkt_fits()
    tabs = {}
    for name, (t, cx, cy, k, L) in fits.items():
        tabs[name] = orc.sample_along(t, cx, cy, k, L, np.linspace(0, 1, int(L // interval), endpoint=False))
    ringL, ringR = np.ascontiguousarray(tabs["l"][:, :2]), np.ascontiguousarray(tabs["r"][:, :2])
    orc.fill_bounds(tabs["c"], ringL, ringR, 100.0)
    rt = RaceTrack.__new__(RaceTrack)
    rt.name = "MGKT"
    rt.center_s = _Length(fits["c"][4])
    rt.center_d = Trajectory(len(tabs["c"]))
    rt.center_d.points = tabs["c"]
    rt.left_r, rt.right_r = Ring(ringL), Ring(ringR)
    rt._build_interpolants()
    return rt


def synthetic_frenet(race_track, N, B, shift=0.0, amp_n=0.3, amp_xi=0.05, seed=0):
    """[B,N,6]: s uniform over the lap (+ shift of a step, so some s < 0 and some > L when shift is not 0), n = amp_n sin,
    xi = amp_xi cos with a phase and a wave number per instance, v > 0."""
    L = race_track.center_s.get_length()
    rng = np.random.default_rng(seed)
    out = np.zeros((B, N, 6))
    i = np.arange(N)
    for b in range(B):
        ds = L / N
        s = i * ds
        if shift and b == B - 1:
            s = s + shift * ds
            s[: N // 4] -= L          # a quarter of the lap below 0 ...
            s[-(N // 4):] += L        # ... and a quarter beyond L
        ph = rng.uniform(0, 2 * np.pi)
        out[b, :, 0] = s
        out[b, :, 1] = amp_n * np.sin(2 * np.pi * (b + 2) * i / N + ph)
        out[b, :, 2] = amp_xi * np.cos(2 * np.pi * (b + 3) * i / N + ph)
        out[b, :, 5] = 10.0 + 3.0 * np.sin(2 * np.pi * i / N + ph)
    return out


# ---------------------------------------------------------------- conditioning of fill_bounds on a table
def crossing_margins(points, ring, side):
    """For the normal segments of fill_bounds (side = +1 left, -1 right; +-100 m along YAW + side pi/2) against the closed
    polyline `ring`: (smallest gap between the closest and the second closest crossing of a node, smallest distance of a
    closest crossing from a ring vertex), both in metres; inf where there is nothing to compare."""
    p = np.asarray(points)[:, [X, Y]]
    yaw = np.asarray(points)[:, YAW] + side * np.pi / 2.0
    d = 100.0 * np.stack([np.cos(yaw), np.sin(yaw)], 1)                       # [N,2]
    v0 = np.asarray(ring, dtype=np.float64)
    e = np.roll(v0, -1, axis=0) - v0                                            # [R,2]
    w = v0[None, :, :] - p[:, None, :]                                          # [N,R,2]
    den = d[:, None, 0] * e[None, :, 1] - d[:, None, 1] * e[None, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (w[..., 0] * e[None, :, 1] - w[..., 1] * e[None, :, 0]) / den       # along the normal, in units of 100 m
        u = (w[..., 0] * d[:, None, 1] - w[..., 1] * d[:, None, 0]) / den       # along the edge
    hit = (den != 0) & (np.abs(s) <= 1.0) & (u >= 0.0) & (u <= 1.0)
    dist = np.where(hit, np.abs(s) * 100.0, np.inf)
    order = np.sort(dist, axis=1)
    gap = order[:, 1] - order[:, 0] if dist.shape[1] > 1 else np.full(len(p), np.inf)
    gap = np.where(np.isfinite(order[:, 0]) & np.isfinite(gap), gap, np.inf)
    j = np.argmin(dist, axis=1)
    uj = u[np.arange(len(p)), j]
    elen = np.hypot(e[j, 0], e[j, 1])
    vert = np.where(np.isfinite(order[:, 0]), np.minimum(uj, 1.0 - uj) * elen, np.inf)
    return float(gap.min()), float(vert.min())


def assert_well_conditioned(tag, points, rings):
    """The issue's condition on a test's inputs: closest crossing ahead of the second closest by >= 1e-6 m and >= 1e-9 m from
    a ring vertex, for every node and both sides.  points [.., N, 19] of the twin; rings one pair or a list of pairs."""
    pts = np.asarray(points).reshape((-1,) + np.asarray(points).shape[-2:])
    gaps, verts = [], []
    for b in range(len(pts)):
        rg = rings[b] if isinstance(rings, list) else rings
        for ring, side in ((rg[0], 1.0), (rg[1], -1.0)):
            g, v = crossing_margins(pts[b], ring, side)
            gaps.append(g); verts.append(v)
    print(f"[pose tables {tag}] conditioning: closest vs second crossing {min(gaps):.2e} m, crossing to ring vertex {min(verts):.2e} m")
    assert min(gaps) >= 1e-6 and min(verts) >= 1e-9
