"""Region tagging and the command-line tools, on the host.

The pin of Trajectory.fill_region is an exact rational twin defined here: Fraction arithmetic, the ray towards +x with the
half-open rule on y, a point on an edge or a vertex is not contained (shapely's Polygon.contains).  The twin is checked on
hand-made cases here; tests/test_region_gpu.py holds the kernel against it."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from spline_trajectory_optimization_amd import ops
from spline_trajectory_optimization_amd.models.trajectory import Region, Trajectory, save_ttl
from spline_trajectory_optimization_amd.utils.casadi_txt import read_txt, write_txt


# ---------------------------------------------------------------------------------------------- the exact twin
def _on_segment(ax, ay, bx, by, px, py):
    if not (min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)):
        return False
    F = Fraction
    return (F(bx) - F(ax)) * (F(py) - F(ay)) == (F(by) - F(ay)) * (F(px) - F(ax))


def twin_contains(vertices, px, py):
    """True when (px, py) lies in the interior of the polygon (even-odd rule), decided exactly."""
    if not (math.isfinite(px) and math.isfinite(py)):
        return False
    v = np.asarray(vertices, dtype=np.float64)[:, :2]
    if not np.all(np.isfinite(v)):
        return False
    w = np.roll(v, -1, axis=0)
    ax, ay, bx, by = v[:, 0], v[:, 1], w[:, 0], w[:, 1]
    xlo, xhi = np.minimum(ax, bx), np.maximum(ax, bx)
    ylo, yhi = np.minimum(ay, by), np.maximum(ay, by)
    # float comparisons are exact: they only select the edges that need rational arithmetic
    near = (xlo <= px) & (px <= xhi) & (ylo <= py) & (py <= yhi)
    for j in np.nonzero(near)[0]:
        if _on_segment(ax[j], ay[j], bx[j], by[j], px, py):
            return False
    cross = (ay > py) != (by > py)
    odd = int(np.count_nonzero(cross & (px < xlo))) & 1
    for j in np.nonzero(cross & (xlo <= px) & (px <= xhi))[0]:
        F = Fraction
        xc = F(ax[j]) + (F(py) - F(ay[j])) * (F(bx[j]) - F(ax[j])) / (F(by[j]) - F(ay[j]))
        odd ^= int(xc > F(px))
    return bool(odd)


def twin_index(regions, xy):
    """Index of the first region (a Region, a vertex array or a (vertices, code) pair) containing each point of xy [n,2], -1
    where none does."""
    out = np.full(len(xy), -1, dtype=np.int32)
    for i, (px, py) in enumerate(np.asarray(xy, dtype=np.float64)):
        for r, reg in enumerate(regions):
            verts = reg.vertices if hasattr(reg, "vertices") else reg if isinstance(reg, np.ndarray) else reg[0]
            if twin_contains(verts, float(px), float(py)):
                out[i] = r
                break
    return out


def twin_fill_region(points, regions):
    idx = twin_index(regions, points[:, :2])
    out = np.array(points, copy=True)
    hit = idx >= 0
    out[hit, Trajectory.REGION] = np.array([regions[r].code for r in idx[hit]], dtype=np.float64)
    return out


SQUARE = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])
DIAMOND = np.array([[2.0, 0.0], [4.0, 2.0], [2.0, 4.0], [0.0, 2.0]])
NOTCH = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [2.0, 1.0], [0.0, 4.0]])   # concave: a notch from the top down to (2,1)


def test_twin_edges_and_vertices_are_outside():
    for p in [(0.0, 0.0), (4.0, 4.0), (2.0, 0.0), (4.0, 1.5), (0.0, 3.0), (2.0, 4.0)]:
        assert not twin_contains(SQUARE, *p), p
    for p in [(3.0, 1.0), (1.0, 3.0), (1.5, 0.5), (2.0, 0.0), (0.0, 2.0)]:   # diagonal edges and vertices
        assert not twin_contains(DIAMOND, *p), p
    assert twin_contains(SQUARE, 2.0, 2.0) and twin_contains(DIAMOND, 2.0, 2.0)
    # the nearest doubles beside a diagonal edge point: one inside, one outside
    assert twin_contains(DIAMOND, np.nextafter(3.0, 0.0), 1.0)
    assert not twin_contains(DIAMOND, np.nextafter(3.0, 4.0), 1.0)


def test_twin_horizontal_edge_and_ray_through_vertex():
    # horizontal edges at the point's y: on them -> outside; beside them -> decided by the other edges
    assert not twin_contains(SQUARE, 1.0, 0.0) and not twin_contains(SQUARE, 1.0, 4.0)
    assert not twin_contains(SQUARE, -1.0, 0.0) and not twin_contains(SQUARE, 5.0, 4.0)
    # rays through the vertices (4,2) and (0,2) of the diamond: counted once
    assert twin_contains(DIAMOND, 1.0, 2.0) and twin_contains(DIAMOND, 3.5, 2.0)
    assert not twin_contains(DIAMOND, -1.0, 2.0) and not twin_contains(DIAMOND, 5.0, 2.0)
    # ray through the apex (2,4) and through the bottom vertex (2,0): points outside stay outside
    assert not twin_contains(DIAMOND, 0.0, 4.0) and not twin_contains(DIAMOND, 0.0, 0.0)


def test_twin_concave_notch():
    assert twin_contains(NOTCH, 1.0, 1.0) and twin_contains(NOTCH, 3.0, 1.0) and twin_contains(NOTCH, 2.0, 0.5)
    assert not twin_contains(NOTCH, 2.0, 3.0)            # inside the notch
    assert not twin_contains(NOTCH, 2.0, 1.0)            # its tip
    assert twin_contains(NOTCH, 0.5, 3.0)                # left prong; the ray crosses the notch twice
    assert not twin_contains(NOTCH, 3.0, 3.5)            # right of the notch's tip, still in the notch


def test_twin_zero_area_and_closing_vertex():
    line = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    for p in [(0.5, 0.5), (0.5, 0.6), (1.0, 1.0), (-1.0, 0.5), (0.5, 0.4)]:
        assert not twin_contains(line, *p), p
    closed = np.vstack([NOTCH, NOTCH[:1]])
    pts = np.random.default_rng(3).uniform(-1, 5, size=(300, 2))
    pts = np.vstack([pts, NOTCH, [[2.0, 0.0], [1.0, 2.5]]])
    for p in pts:
        assert twin_contains(closed, *p) == twin_contains(NOTCH, *p), p


def test_twin_first_region_wins_and_untouched_region():
    regions = [Region("a", 7, SQUARE), Region("b", 9, DIAMOND), Region("c", 11, SQUARE + 10.0)]
    pts = np.zeros((5, 19))
    pts[:, :2] = [[2.0, 2.0], [0.1, 0.1], [12.0, 12.0], [20.0, 20.0], [4.0, 2.0]]
    pts[:, Trajectory.REGION] = [-5, -5, -5, 3, 3]
    out = twin_fill_region(pts, regions)
    assert out[:, Trajectory.REGION].tolist() == [7, 7, 11, 3, 3]
    assert twin_index(regions[::-1][:2], pts[:1, :2]).tolist() == [1]   # c does not contain (2,2), b comes next
    assert twin_index([Region("b", 9, DIAMOND), Region("a", 7, SQUARE)], pts[:2, :2]).tolist() == [0, 1]


def test_twin_nan_points():
    for p in [(np.nan, 2.0), (2.0, np.nan), (np.inf, 2.0), (2.0, -np.inf)]:
        assert not twin_contains(SQUARE, *p)


# ---------------------------------------------------------------------------------------------- host-side contract
def test_region_tables_and_short_polygons():
    V, off, codes = ops.region_tables([Region("a", 3, SQUARE), (DIAMOND, 5)])
    assert V.shape == (8, 2) and off.tolist() == [0, 4, 8] and codes.tolist() == [3, 5]
    for bad in (SQUARE[:2], SQUARE[:0], np.zeros(6)):
        with pytest.raises(ValueError):
            ops.region_tables([Region("x", 1, bad)])
    with pytest.raises(ValueError):
        Trajectory(4).fill_region([Region("ok", 1, SQUARE), Region("x", 2, SQUARE[:2])])


def test_fill_region_needs_no_shapely():
    """Before the kernel existed, fill_region imported shapely (absent here); with no regions it is a no-op."""
    traj = Trajectory(3)
    traj[:, Trajectory.REGION] = [1, 2, 3]
    traj.fill_region([])
    assert traj[:, Trajectory.REGION].tolist() == [1, 2, 3]


# ---------------------------------------------------------------------------------------------- CasADi txt
def test_casadi_txt_round_trip(tmp_path):
    a = np.random.default_rng(0).normal(size=(7, 4)) * 10.0 ** np.arange(-3, 4)[:, None]
    a[2, 1] = 0.0
    a[3, 3] = -0.0
    write_txt(tmp_path / "a.txt", a)
    b = read_txt(tmp_path / "a.txt")
    assert b.shape == a.shape and np.array_equal(a, b)
    write_txt(tmp_path / "v.txt", np.arange(5.0))
    assert read_txt(tmp_path / "v.txt").shape == (5, 1)
    (tmp_path / "c.txt").write_text("% a CasADi header\n\n1.5 00 -2\n# comment\n00 nan Inf\n  \n-inf 3e-300 00\n")
    c = read_txt(tmp_path / "c.txt")
    assert c.shape == (3, 3)
    assert c[0].tolist() == [1.5, 0.0, -2.0] and c[1, 0] == 0.0 and np.isnan(c[1, 1]) and c[1, 2] == np.inf
    assert c[2, 0] == -np.inf and c[2, 1] == 3e-300 and c[2, 2] == 0.0
    (tmp_path / "d.txt").write_text("1 2\n3\n")
    with pytest.raises(ValueError):
        read_txt(tmp_path / "d.txt")


# ---------------------------------------------------------------------------------------------- the CLI tools
def _ttl(path, n=6):
    traj = Trajectory(n, ttl_num=4, origin=(1.0, 2.0, 3.0))
    traj[:, 0] = np.arange(n) * 1.5
    traj[:, 1] = np.arange(n) * -0.5
    traj[:, Trajectory.SPEED] = 12.0
    traj[:, Trajectory.REGION] = 2
    traj[:, Trajectory.TIME] = 0.25
    traj.fill_distance()
    save_ttl(str(path), traj)
    return traj


def test_convert_to_casadi_end_to_end(tmp_path):
    from spline_trajectory_optimization_amd.entrypoints import traj_opt_convert_to_casadi as cli
    traj = _ttl(tmp_path / "in.csv")
    cli.main([str(tmp_path / "in.csv"), str(tmp_path / "out.txt")])
    m = read_txt(tmp_path / "out.txt")
    assert m.shape == (len(traj), Trajectory.TIME + 1)
    want = traj.points[:, :Trajectory.TIME + 1].copy()
    want[:, Trajectory.SPEED] = -100.0
    assert np.array_equal(m, want)


@pytest.mark.parametrize("name,nargs", [("traj_opt_convert_to_casadi", 2), ("traj_opt_encode_region", 3)])
def test_cli_wrong_argument_count(name, nargs, tmp_path, capsys, monkeypatch):
    import importlib
    cli = importlib.import_module(f"spline_traj_optm.entrypoints.{name}")
    monkeypatch.chdir(tmp_path)
    for n in (0, nargs - 1, nargs + 1):
        monkeypatch.setattr(sys, "argv", [name] + [f"arg{i}" for i in range(n)])
        assert cli.main() is None
        assert capsys.readouterr().out.startswith("Usage:")
    assert os.listdir(tmp_path) == []


def test_double_track_needs_yaml(tmp_path, monkeypatch):
    from spline_traj_optm.entrypoints import traj_opt_double_track as cli
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="traj_opt_double_track.yaml"):
        cli.main()


def test_cli_modules_run_with_python_m(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "spline_traj_optm.entrypoints.traj_opt_encode_region", "only-one"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("Usage:"), r.stderr
    r = subprocess.run([sys.executable, "-m", "spline_trajectory_optimization_amd.entrypoints.traj_opt_double_track"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "FileNotFoundError" in r.stderr
