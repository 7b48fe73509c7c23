"""Host check of csrc/rl_cone.hpp -- the direction cone of a search window and the predicate "the side values are monotone
along this window for this direction" that lets the sweep's window scan bracket a crossing with four vertices instead of 25
(csrc/rl_device.hpp: scan_window) -- against exact evaluations.  tests/cone_check.cpp states what is checked per window,
direction and point; the header is plain IEEE arithmetic with error bounds that cover a fused and an unfused evaluation, so
what holds for the host build holds for the device's.

Rings: the width-form rings (vertex i on sample i's normal, which is the direction tried there, and that turned by +-0.1 rad)
about the Monza and the kart centre lines at N = 2000, 400 and 104; the Monza and kart boundary rings in both orientations;
noisy circles of 97, 101 and 333 vertices; a hairpin that turns round inside one window; a vertex three times in a row; an
infinite and a NaN vertex; rings of 48 and 40 vertices (the windowed search does not take them: every record invalid).

The predicate is not vacuous: wherever the exact evaluation finds the window strictly monotone with every |sin(edge, d)| >
2^-10 (the margin 2^-12, the cone's outward turn 2^-18 and the float roundings together stay below 2^-11) and every edge
within 89 degrees of the window's chord, it must hold -- cone_check counts a miss as an error.  Measured here, as shares of
the (hinted vertex, direction) pairs, direction = the sample's normal and that turned by +-0.1 rad:
  Monza widths N = 2000: 99.4 % exactly monotone, every one of them with that room, the predicate holds on every one;
  Monza widths N = 400 (edges of 14 m): 90.8 % exactly monotone, 98.5 % of those with room, the predicate holds on 99.4 %;
  Monza widths N = 104: 54 % exactly monotone, the predicate holds on 92 % of those (a window is a quarter of the lap);
  kart widths N = 2000: 100 %, 100 %, 100 %;  N = 400: 91 %, 99 %, 99 %;  N = 104: 16 % exactly monotone, 94 % of those."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kart_cases
from conftest import spline
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


def _width_rings_with_normals(t, cx, cy, k, length, ringL, ringR, N):
    """[(vertices and directions [N,4])] of the left and the right width-form ring about the line at N samples."""
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    pts = orc.fill_bounds(pts, ringL, ringR, 100.0)
    wl = np.hypot(pts[:, 9] - pts[:, 0], pts[:, 10] - pts[:, 1])
    wr = np.hypot(pts[:, 11] - pts[:, 0], pts[:, 12] - pts[:, 1])
    x, y, yaw = pts[:, 0], pts[:, 1], pts[:, 3]
    out = []
    for w, a in ((wl, yaw + np.pi / 2), (wr, yaw - np.pi / 2)):
        c, s = np.cos(a), np.sin(a)
        out.append(np.column_stack([x + w * c, y + w * s, 100.0 * c, 100.0 * s]))
    return out


def _circle_ring(nr, radius=50.0, seed=0, noise=0.5):
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(nr) / nr
    rr = radius + rng.uniform(-noise, noise, nr)
    return np.stack([rr * np.cos(a) + 13.0, rr * np.sin(a) - 7.0], axis=1)


def _hairpin_ring():
    """Two straights 4 m apart joined by half circles of six edges each: a window over a half circle turns by pi."""
    n = 60
    top = np.stack([np.linspace(0.0, 118.0, n), np.full(n, 2.0)], axis=1)
    a = np.linspace(np.pi / 2, -np.pi / 2, 7)[1:-1]
    right = np.stack([118.0 + 2.0 * np.cos(a), 2.0 * np.sin(a)], axis=1)
    bottom = top[::-1] * np.array([1.0, -1.0])
    left = np.stack([-2.0 * np.cos(a), -2.0 * np.sin(a)], axis=1)
    return np.vstack([top, right, bottom, left])


def _records(fits, rings):
    """[(label, kind, array)]: kind 0 a ring [nr,2], kind 1 vertices with directions [nr,4]."""
    rec = []
    t, cx, cy, k, length = spline(fits, "c100")
    for N in (2000, 400, 104):
        for side, r in zip("LR", _width_rings_with_normals(t, cx, cy, k, length, rings[0], rings[1], N)):
            rec.append((f"monza widths N={N} {side}", 1, r))
    kt, kcx, kcy, kk, klength, kL, kR = kart_cases.case("base")
    for N in (2000, 400, 104):
        for side, r in zip("LR", _width_rings_with_normals(kt, kcx, kcy, kk, klength, kL, kR, N)):
            rec.append((f"kart widths N={N} {side}", 1, r))
    rec += [("monza ringL", 0, rings[0]), ("monza ringR reversed", 0, rings[1][::-1]), ("kart ringL", 0, kL), ("kart ringR reversed", 0, kR[::-1])]
    for nr in (97, 101, 333):
        rec.append((f"circle nr={nr}", 0, _circle_ring(nr, seed=nr)))
    rec.append(("circle nr=333 reversed, rough", 0, _circle_ring(333, radius=20.0, seed=5, noise=2.0)[::-1]))
    rec.append(("hairpin", 0, _hairpin_ring()))
    dup = _circle_ring(203, seed=3)
    rec.append(("a vertex three times", 0, np.insert(dup, [40, 40], dup[[40, 40]], axis=0)))
    bad = _circle_ring(203, seed=4)
    bad[17, 0] = np.inf
    bad[120, 1] = np.nan
    rec.append(("inf and NaN vertex", 0, bad))
    rec.append(("circle nr=48", 0, _circle_ring(48, seed=48)))
    rec.append(("circle nr=40", 0, _circle_ring(40, seed=40)))
    return rec


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cone_records_and_the_bracket_against_exact_evaluations(tmp_path, fits, rings):
    exe = str(tmp_path / "cone_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "cone_check.cpp"), "-o", exe])
    rec = _records(fits, rings)
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        for _, kind, arr in rec:
            arr = np.ascontiguousarray(arr, dtype=np.float64)
            np.array([kind, arr.shape[0]], dtype=np.int64).tofile(f)
            arr.tofile(f)
    out = subprocess.run([exe, path], capture_output=True, text=True)
    lines = [l for l in out.stdout.splitlines() if l.startswith("rec ")]
    for (label, _, _), l in zip(rec, lines):
        print(f"{label:32s} {l}")
    print(out.stdout[-3000:] if out.returncode else "", out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-4000:]
    assert len(lines) == len(rec) and "TOTAL 0" in out.stdout
    stat = {}
    for (label, _, _), l in zip(rec, lines):
        w = l.replace(" of ", " windows ").split()
        stat[label] = dict(zip(w[2::2], map(int, w[3::2])))
    # every adversarial input reaches the code it is meant for
    for label in ("circle nr=48", "circle nr=40"):
        assert stat[label]["valid"] == 0 and stat[label]["tests"] == 0, (label, stat[label])
    assert 0 < stat["hairpin"]["valid"] < stat["hairpin"]["windows"], stat["hairpin"]          # the straights: valid; over a half circle: not
    assert stat["a vertex three times"]["windows"] - stat["a vertex three times"]["valid"] >= 3   # the windows over the zero edges
    assert stat["inf and NaN vertex"]["windows"] - stat["inf and NaN vertex"]["valid"] >= 6
    for label in ("circle nr=97", "circle nr=101", "monza ringR reversed", "kart ringR reversed"):
        assert stat[label]["valid"] > 0 and stat[label]["holds"] > 0 and stat[label]["brackets"] > 0, (label, stat[label])
    # the floor: what the exact evaluation finds monotone with the margin's room (cone_check fails on a miss, so holds >= that),
    # and on smooth rings that is nearly all it finds monotone at all
    for label in [l for l in stat if " widths " in l]:
        s = stat[label]
        assert s["smooth_holds"] >= s["smooth_margin"] > 0, (label, s)
        if "N=2000" in label:   # the benchmark's sampling
            assert s["smooth_exact"] >= 0.98 * s["smooth"], (label, s)            # the inputs are what they are taken for: 99 % of Monza's windows are monotone
            assert s["smooth_margin"] >= 0.99 * s["smooth_exact"], (label, s)     # the margin's share: directions within 1e-3 rad of an edge
        if "N=104" not in label:
            assert s["brackets"] > s["smooth"], (label, s)                        # and the bracket is taken: more than one point in three
