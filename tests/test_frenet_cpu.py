"""rl_frenet_batch_* / rl_frenet_resample_* without a GPU: the twin (tests/frenet_twin.py) against RaceTrack.frenet_to_global and
numpy.interp, the declarations, the Python entry points and their argument checks (which raise before any device call).

Bounds: the twin inverts frenet_to_global to 1e-10 m (s cyclic, n) and 1e-10 rad (xi); measured on these inputs 5.7e-14 m in s,
4e-14 m in n with gaps >= 19 m between the best and the second-best local minimum and g >= 0.59.  The resample twin against
periodic numpy.interp: 1e-12 (the same formula on the same brackets; the bridged wrap pair subtracts L once more)."""
import inspect
import os
import re

import numpy as np
import pytest

import frenet_twin as ft
import pose_tables_twin as ptw
from spline_trajectory_optimization_amd import _lib, batch, ops
from spline_trajectory_optimization_amd.min_time_optm import min_time_optimizer as mto
from spline_trajectory_optimization_amd.models.race_track import RaceTrack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"rl_frenet_batch_dev": 13, "rl_frenet_batch_host": 13, "rl_frenet_resample_dev": 11, "rl_frenet_resample_host": 11}


@pytest.fixture(scope="module")
def rt():
    return ptw.mgkt_race_track(8.0)


@pytest.mark.parametrize("amp_n", [0.3, 2.0, 4.0])
def test_twin_inverts_frenet_to_global(rt, amp_n):
    pieces = rt.centerline_pieces()
    L = rt.center_s.get_length()
    X = ptw.synthetic_frenet(rt, 257, 3, shift=0.37, amp_n=amp_n)
    assert (X[-1, :, 0] < 0).sum() > 5 and (X[-1, :, 0] > L).sum() > 5
    fr, gap = ft.project_batch(pieces, ft.line_tables(rt, X))
    ft.assert_well_conditioned(f"twin amp_n={amp_n}", fr, gap)
    es = ft.cyclic(fr[..., 0], np.mod(X[..., 0], L), L).max()
    en, exi = np.abs(fr[..., 1] - X[..., 1]).max(), np.abs(fr[..., 2] - X[..., 2]).max()
    print(f"[frenet twin amp_n={amp_n}] round trip: s {es:.2e} m, n {en:.2e} m, xi {exi:.2e} rad")
    assert es <= 1e-10 and en <= 1e-10 and exi <= 1e-10
    assert (fr[..., 0] >= 0).all() and (fr[..., 0] < L).all()
    # g is 1 - kappa n whatever the parametric speed of the pieces: N . c'' = kappa |c'|^2
    kn = 1.0 - rt.curvature_intp(fr[..., 0].reshape(-1)).reshape(fr.shape[:2]) * fr[..., 1]
    assert np.abs(fr[..., 3] - kn).max() <= 1e-9


def test_twin_takes_the_global_minimum(rt):
    """A point 1 m off the centre line is projected where it came from even when started from far away: no hint in the twin."""
    pieces = rt.centerline_pieces()
    L = rt.center_s.get_length()
    s = np.array([0.0, 0.25 * L, np.nextafter(L, 0.0)])
    pts = np.asarray(rt.frenet_to_global(s, np.full(3, -1.0), np.zeros(3)))[None, :, :2]
    fr, _ = ft.project_batch(pieces, np.ascontiguousarray(pts))
    assert ft.cyclic(fr[0, :, 0], s, L).max() <= 1e-10 and np.abs(fr[0, :, 1] + 1.0).max() <= 1e-10
    assert (fr[0, :, 2] == 0).all()


def _line(P, L, rot=0, seed=0):
    rng = np.random.default_rng(seed)
    s = np.sort(rng.uniform(0.0, L, size=P))
    fr = np.stack([s, rng.normal(size=P), rng.uniform(-0.4, 0.4, size=P), np.ones(P)], 1)
    vals = rng.uniform(5.0, 20.0, size=(P, 2))
    return np.roll(fr, rot, axis=0), np.roll(vals, rot, axis=0)


@pytest.mark.parametrize("rot", [0, 17])
def test_resample_twin_equals_periodic_interp(rot):
    L, P = 100.0, 50
    fr, vals = _line(P, L, rot)
    nodes = np.r_[np.linspace(0.0, L, 37, endpoint=False), np.sort(fr[:, 0])[[0, 11, P - 1]], 0.5 * np.sort(fr[:, 0])[0]]
    out, st = ft.resample(fr, vals, nodes, L)
    assert st == 0
    k = np.argsort(fr[:, 0])
    for c, col in enumerate([fr[k, 1], fr[k, 2], vals[k, 0], vals[k, 1]]):
        ref = np.interp(nodes, fr[k, 0], col, period=L)
        assert np.abs(out[:, c] - ref).max() <= 1e-12
    j = np.nonzero(nodes == np.sort(fr[:, 0])[11])[0][0]
    assert out[j, 0] == fr[k[11], 1] and out[j, 2] == vals[k[11], 0]      # a node on a sample: the sample itself


def test_resample_twin_aligns_xi_across_pi():
    fr = np.array([[10.0, 0.0, 3.1, 1.0], [20.0, 0.0, -3.1, 1.0], [30.0, 0.0, -3.0, 1.0]])
    out, st = ft.resample(fr, None, np.array([15.0]), 100.0)
    assert st == 0 and abs(out[0, 1] - (3.1 + 0.5 * (2 * np.pi - 6.2))) <= 1e-15


def test_resample_twin_rejects_non_monotone_and_bad_points():
    L = 100.0
    fr, vals = _line(20, L)
    nodes = np.linspace(0, L, 7, endpoint=False)
    sw = fr.copy(); sw[[4, 9]] = sw[[9, 4]]
    for bad in (sw, np.where(np.arange(20)[:, None] == 3, np.nan, fr)):
        out, st = ft.resample(bad, vals, nodes, L)
        assert st == 1 and (out == 0).all() and out.shape == (7, 4)
    out, st = ft.resample(fr[:1], vals[:1], nodes, L)                       # a single point: constant
    assert st == 0 and (out[:, 0] == fr[0, 1]).all()


def test_guess_twin_step_times(rt):
    """On the centre line itself (n = xi = 0) the guess's step times are ds / v."""
    s = rt.abscissa
    L = rt.center_s.get_length()
    fr = np.stack([s, 0 * s, 0 * s, 1 + 0 * s], 1)
    v = np.full(len(s), 12.5)
    X, T, st = ft.guess(fr, v, s, rt.curvature_intp(s), L, v, np.ones(len(s)))
    assert st == 0 and np.abs(T - (np.r_[s[1:], L] - s) / 12.5).max() <= 1e-15 and (X[:, 5] == 12.5).all()
    X, T, st = ft.guess(fr, -v, s, rt.curvature_intp(s), L, v, np.ones(len(s)))
    assert st == 2 and (T == 1).all() and (X[:, 1] == 0).all()


def test_header_declares_and_lib_binds_the_symbols():
    header = open(os.path.join(ROOT, "include", "rl_mincurv.h")).read()
    for name, nargs in SYMBOLS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/rl_mincurv.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._SIGNATURES[name][1]) == decl.group(1).count(",") + 1 == nargs
    assert getattr(_lib.load(), "rl_frenet_batch_dev") is not None
    assert '"frenet_search"' in header
    assert re.search(r"#define\s+RL_VERSION\s+103\b", header)


def test_python_entry_points_exist():
    for fn, args in ((ops.frenet_torch, ["pieces", "points", "yaw"]), (ops.frenet_host, ["pieces", "points", "yaw"]),
                     (ops.frenet_resample_torch, ["fr", "vals", "s_nodes", "length"]),
                     (ops.frenet_resample_host, ["fr", "vals", "s_nodes", "length"]),
                     (batch.min_time_guess_from_lines_torch, ["race_track", "points", "s_nodes", "kappa_nodes", "base", "pieces"]),
                     (RaceTrack.global_to_frenet, ["self", "x", "y", "yaw"])):
        assert list(inspect.signature(fn).parameters)[:len(args)] == args
    p = inspect.signature(mto.optimise_track_batch).parameters
    assert p["start_points"].default is None


def test_argument_checks_raise_before_any_device_call(rt, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib.Context, "get", classmethod(no_device))
    pieces = rt.centerline_pieces()
    pts = np.zeros((2, 5, 2))
    bad = [
        lambda: ops.frenet_host(pieces[:2], pts),
        lambda: ops.frenet_host((pieces[0][:3], pieces[1][:, :2], pieces[2][:, :2]), pts),       # M = 2
        lambda: ops.frenet_host(pieces, np.zeros((2, 5, 3))),                                     # stride
        lambda: ops.frenet_host(pieces, np.zeros((5, 2))),                                        # rank
        lambda: ops.frenet_host(pieces, np.zeros((2, 0, 2))),                                     # P < 1
        lambda: ops.frenet_host(pieces, pts.astype(np.float32)),
        lambda: ops.frenet_host(pieces, np.zeros((2, 5, 4))[:, :, :2]),                           # not contiguous
        lambda: ops.frenet_host(pieces, pts, yaw=np.zeros((2, 4))),
        lambda: ops.frenet_host(pieces, np.zeros((2, 5, 19)), yaw=np.zeros((2, 5))),
        lambda: ops.frenet_host((pieces[0], pieces[1][:, :-1], pieces[2]), pts),
        lambda: ops.frenet_torch(pieces, pts),                                                    # numpy where cuda tensors belong
        lambda: ops.frenet_resample_host(np.zeros((2, 5, 3)), None, np.zeros(4), 10.0),
        lambda: ops.frenet_resample_host(np.zeros((2, 5, 4)), np.zeros((2, 4, 1)), np.zeros(4), 10.0),
        lambda: ops.frenet_resample_host(np.zeros((2, 5, 4)), np.zeros((2, 5)), np.zeros(4), 10.0),
        lambda: ops.frenet_resample_host(np.zeros((2, 5, 4)), None, np.zeros((4, 1)), 10.0),
        lambda: ops.frenet_resample_host(np.zeros((2, 5, 4)), None, np.zeros(4), 0.0),
        lambda: ops.frenet_resample_host(np.zeros((2, 5, 4)), None, np.zeros(4, dtype=np.float32), 10.0),
        lambda: ops.frenet_resample_torch(np.zeros((2, 5, 4)), None, np.zeros(4), 10.0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
