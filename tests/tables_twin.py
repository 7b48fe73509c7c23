"""CPU statement of rl_tables_batch_* and rl_table_summary_*: the oracle's sample_along + fill_bounds (pinned to the
reference-generated fixtures G2 / G4 / G1 in tests/test_oracle_golden.py) composed per instance, orc.width_rings for the
width form, numpy on the table for the summary.  No arithmetic of its own beyond that composition."""
import numpy as np

from oracle import oracle as orc

X, Y, YAW, SPEED, CURV, BWD, FWD, LBX, LBY, RBX, RBY, BANK, LON, LAT, TIME, IDX, FLAG = 0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18
BOUND_COLS = [LBX, LBY, RBX, RBY]
ZERO_COLS = [2, SPEED, 8, LON, LAT, TIME]


def table(t, cx, cy, k, length, N, ringL, ringR, bank=None):
    """One instance: sample_along(ts = i/N) of the spline, fill_bounds against the rings (max_dist 100), BANK copied in.
    length <= 0: both DIST columns stay 0 (include/rl_mincurv.h)."""
    u = np.linspace(0.0, 1.0, N, endpoint=False)
    pts = orc.sample_along(t, np.ascontiguousarray(cx), np.ascontiguousarray(cy), k, length, u)
    if not length > 0.0:
        pts[:, [BWD, FWD]] = 0.0
    orc.fill_bounds(pts, ringL, ringR, 100.0)
    if bank is not None:
        pts[:, BANK] = bank
    return pts


def width_rings(t, cx0, cy0, k, N, widths):
    """Rings of one width-form instance [N,2] = (w_left, w_right) on the track's INITIAL control points."""
    return orc.width_rings(t, cx0, cy0, k, N, np.ascontiguousarray(widths))


def tables(t, k, N, ctrl, rings, length, bank=None):
    """ctrl [B,n,2]; rings = one (ringL, ringR) pair for all instances or a list of B pairs; bank None, [N] or [B,N]."""
    B = len(ctrl)
    out = np.empty((B, N, 19))
    for b in range(B):
        rl_, rr_ = rings[b] if isinstance(rings, list) else rings
        bk = None if bank is None else (bank[b] if np.ndim(bank) == 2 else bank)
        out[b] = table(t, ctrl[b, :, 0], ctrl[b, :, 1], k, length, N, rl_, rr_, bk)
    return out


def summary(points):
    """[8] of one simulated table, in the order of ops.SUMMARY_COLUMNS."""
    p = np.asarray(points)
    return np.array([np.cumsum(p[:, TIME])[-1], p[0, TIME], p[0, FWD] / p[0, TIME], p[:, SPEED].max(), p[:, SPEED].min(),
                     p[:, LAT].max(), p[:, LON].max(), p[:, LON].min()])
