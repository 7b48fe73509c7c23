"""rl_pose_tables_batch_* without a GPU: the declarations, RaceTrack.centerline_pieces, the twin (tests/pose_tables_twin.py)
against the host tail of optimise_track, and the argument checks of ops.pose_tables_host."""
import os
import re

import numpy as np
import pytest

import pose_tables_twin as ptw
from oracle import oracle as orc
from spline_trajectory_optimization_amd import _lib, ops
from spline_trajectory_optimization_amd.min_time_optm import min_time_optimizer as mto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rl_pose_tables_batch_dev", "rl_pose_tables_batch_host")


@pytest.fixture(scope="module")
def rt():
    return ptw.mgkt_race_track(8.0)


def test_header_declares_and_lib_binds_the_symbols():
    header = open(os.path.join(ROOT, "include", "rl_mincurv.h")).read()
    for name in SYMBOLS:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/rl_mincurv.h"
        assert name in _lib.EXPORTED_SYMBOLS
        res, args = _lib._SIGNATURES[name]
        assert len(args) == decl.group(1).count(",") + 1 == 16
    assert re.search(r"RL_POSE_FRENET\s*=\s*0\s*,\s*RL_POSE_GLOBAL\s*=\s*1", header)
    assert (_lib.POSE_FRENET, _lib.POSE_GLOBAL) == (0, 1)


def _eval_pieces(ss, c, q, der):
    """The pieces by hand: interval by binary search, the cubic and its derivative in powers of (q - ss[j])."""
    j = np.clip(np.searchsorted(ss, q, side="right") - 1, 0, len(ss) - 2)
    d = q - ss[j]
    if der == 0:
        return c[3, j] + c[2, j] * d + c[1, j] * d ** 2 + c[0, j] * d ** 3
    return c[2, j] + 2.0 * c[1, j] * d + 3.0 * c[0, j] * d ** 2


def test_centerline_pieces_reproduce_the_interpolants(rt):
    ss, cxs, cys = rt.centerline_pieces()
    M = len(ss) - 1
    L = rt.center_s.get_length()
    assert ss.dtype == cxs.dtype == cys.dtype == np.float64 and cxs.shape == cys.shape == (4, M)
    assert ss.flags.c_contiguous and cxs.flags.c_contiguous and cys.flags.c_contiguous
    assert ss[0] == 0.0 and ss[M] == L and M == len(rt.abscissa)
    s = np.random.default_rng(3).uniform(-1.5 * L, 2.5 * L, size=1000)
    assert (s < 0).sum() > 100 and (s > L).sum() > 100
    q = np.mod(s, L)
    x, y = _eval_pieces(ss, cxs, q, 0), _eval_pieces(ss, cys, q, 0)
    yaw = np.arctan2(_eval_pieces(ss, cys, q, 1), _eval_pieces(ss, cxs, q, 1))
    dx, dy, dyaw = np.abs(x - rt.x_intp(s)).max(), np.abs(y - rt.y_intp(s)).max(), np.abs(yaw - rt.yaw_intp(s)).max()
    print(f"[pose tables pieces] |dx| {dx:.2e} |dy| {dy:.2e} |dyaw| {dyaw:.2e}")
    assert max(dx, dy) <= 1e-12 and dyaw <= 1e-12


def test_twin_is_the_host_tail_of_optimise_track(rt, monkeypatch):
    """optimise_track ends in min_time_optimizer.pose_table (frenet_to_global, the four columns, fill_trajectory_boundaries,
    fill_distance); its fill_bounds is the HIP kernel, which this test replaces by the oracle's -- the twin's."""
    def fill_bounds(points, ringL, ringR, max_dist=100.0, device=None):
        orc.fill_bounds(points, np.ascontiguousarray(ringL), np.ascontiguousarray(ringR), max_dist)
        return points
    monkeypatch.setattr(ops, "fill_bounds", fill_bounds)
    N = len(rt.abscissa)
    i = np.arange(N)
    X = np.zeros((N, 6))
    X[:, 0] = rt.abscissa
    X[:, 1] = 0.3 * np.sin(2 * np.pi * 3 * i / N)
    X[:, 2] = 0.05 * np.cos(2 * np.pi * 5 * i / N)
    X[:, 5] = 12.0 + np.sin(2 * np.pi * i / N)
    base = rt.center_d.copy()
    base[:, 4] = 7.0; base[:, 14] = 0.5; base[:, 16] = 0.1; base[:, 18] = 2.0     # a table the simulator has been over
    host = mto.pose_table(rt, base, X).points
    rings = (rt.left_r.coords, rt.right_r.coords)        # what Trajectory.fill_bounds hands on (trajectory.py: _ring_coords)
    twin = ptw.frenet_table(rt, X, rings, base=base.points)
    for c in (0, 1, 3, 4, 6, 7, 9, 10, 11, 12):
        np.testing.assert_array_equal(twin[:, c], host[:, c])
    np.testing.assert_array_equal(twin, host)
    assert np.abs(host[:, 9:13] - base.points[:, 9:13]).max() > 1e-3    # the bounds moved with the line
    # TIME: the duration of the step that starts at node i lands on node i + 1
    T = np.linspace(0.1, 0.2, N)
    tt = ptw.frenet_table(rt, X, rings, base=base.points, T=T)
    assert tt[0, 16] == T[-1] and np.array_equal(tt[1:, 16], T[:-1])
    np.testing.assert_array_equal(np.delete(tt, 16, axis=1), np.delete(twin, 16, axis=1))
    # no base: the columns of an empty Trajectory
    empty = ptw.frenet_table(rt, X, rings)
    np.testing.assert_array_equal(empty[:, 17], i)
    assert (empty[:, 18] == -1).all() and not empty[:, [2, 5, 8, 13, 14, 15, 16]].any()
    ptw.assert_well_conditioned("cpu", twin, (rt.left_r.vertices, rt.right_r.vertices))


class _FakeTrack:
    """ops.pose_tables_host reads N before it checks; any access to the library fails the test."""
    N = 10

    @property
    def ctx(self):
        raise AssertionError("argument checks must come before any library call")
    h = ctx


def test_argument_checks_raise_before_any_library_call():
    trk = _FakeTrack()
    F, G, S, W, P = _lib.POSE_FRENET, _lib.POSE_GLOBAL, _lib.BOUNDS_SHARED_RINGS, _lib.BOUNDS_WIDTHS, _lib.BOUNDS_POINTS
    B, N, M = 2, 7, 5
    X6, X5 = np.zeros((B, N, 6)), np.zeros((B, N, 5))
    pieces = (np.linspace(0, 1, M + 1), np.zeros((4, M)), np.zeros((4, M)))
    bad = [
        dict(form=3, X=X6, pieces=pieces, bounds_form=S, bounds=None),                           # form
        dict(form=F, X=X6, pieces=pieces, bounds_form=7, bounds=None),                           # bounds form
        dict(form=F, X=X5, pieces=pieces, bounds_form=S, bounds=None),                           # width of X
        dict(form=G, X=X6, pieces=None, bounds_form=S, bounds=None),
        dict(form=F, X=X6[0], pieces=pieces, bounds_form=S, bounds=None),                        # rank
        dict(form=F, X=np.zeros((B, 1, 6)), pieces=pieces, bounds_form=S, bounds=None),          # N < 2
        dict(form=F, X=X6, pieces=None, bounds_form=S, bounds=None),                             # FRENET without pieces
        dict(form=F, X=X6, pieces=(pieces[0], np.zeros((4, M + 1)), pieces[2]), bounds_form=S, bounds=None),
        dict(form=F, X=X6.astype(np.float32), pieces=pieces, bounds_form=S, bounds=None),        # dtype
        dict(form=F, X=np.zeros((B, N, 12))[:, :, ::2], pieces=pieces, bounds_form=S, bounds=None),   # not contiguous
        dict(form=F, X=X6, pieces=pieces, bounds_form=W, bounds=None),                           # widths without bounds
        dict(form=F, X=X6, pieces=pieces, bounds_form=S, bounds=np.zeros((B, 10, 2))),           # bounds with shared rings
        dict(form=F, X=X6, pieces=pieces, bounds_form=P, bounds=np.zeros((B, N, 4))),            # track.N vertices, not N
        dict(form=G, X=X5, pieces=None, bounds_form=S, bounds=None, base=np.zeros((N, 18))),
        dict(form=G, X=X5, pieces=None, bounds_form=S, bounds=None, base=np.zeros((B + 1, N, 19))),
        dict(form=G, X=X5, pieces=None, bounds_form=S, bounds=None, T=np.zeros((B, N + 1))),
        dict(form=G, X=X5, pieces=None, bounds_form=S, bounds=None, T=[[0.0] * N] * B),
    ]
    for kw in bad:
        kw = dict(kw)
        args = (kw.pop("form"), kw.pop("X"), kw.pop("pieces"), kw.pop("bounds_form"), kw.pop("bounds"))
        with pytest.raises(ValueError):
            ops.pose_tables_host(trk, *args, **kw)
