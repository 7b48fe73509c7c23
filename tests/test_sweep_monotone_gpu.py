"""The bracket path of the sweep's window scan (csrc/rl_device.hpp: scan_window, BRACKET; csrc/rl_cone.hpp): where a window's
direction cone proves the side values monotone, four vertices around the hinted edge stand for all 25.  It may not move a
bit.  Every case runs with the rings in global memory (the staged path, RL_FORCE_RESIDENCY=0), in the reference-order, the
fast and the branch arithmetic, and compares control points, sampled line, success counts and status as bit patterns

  * with the path on (context option "sweep_bracket" = 1, the default) against the path off, and
  * the windowed search (path on) against the brute-force search, which has no window at all.

Cases: the two smallest width-form rings the staged search takes (104 vertices, and 131 -- no multiple of the chunk, windows
run over the seam; vertex i of a width-form ring sits exactly on sample i's first normal, so the exact-zero pass and the bracket
meet in one wave), the kart circuit's hairpins (valid and invalid cone records inside one tile), reversed rings, a ring with a
vertex twice in a row (a zero edge: its windows' records are invalid), start lines 2.5 m off the centre line (crossings several
edges from their hints: the fall-back) and fixture G12 under numpy's raise mode (the raise instantiation)."""
import numpy as np
import pytest

import kart_cases
from conftest import golden, spline
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
FAST, REF, BRANCH = 0, 1, 2   # _lib.ARITH_FAST, _REFERENCE, _BRANCH
BRUTE, WINDOWED = 0, 2        # _lib.SEARCH_BRUTE, _WINDOWED


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch = _lib, ops, batch
    ns.ctx = _lib.Context.get(0)
    assert (_lib.ARITH_FAST, _lib.ARITH_REFERENCE, _lib.ARITH_BRANCH) == (FAST, REF, BRANCH)
    assert (_lib.SEARCH_BRUTE, _lib.SEARCH_WINDOWED) == (BRUTE, WINDOWED)
    return ns


def _bits(label, got, want):
    for name, g, w in zip(("ctrl", "xy", "n_success", "status"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (label, name)
        same = g.view(np.uint8) == w.view(np.uint8)
        assert same.all(), f"{label}: {name} differs in {int((~same).sum())} bytes"


def _on_off_brute(rl, monkeypatch, run, label, ariths=(REF, FAST, BRANCH)):
    """run(search, arith) -> (ctrl, xy, ns, status, stats), rings in global memory."""
    monkeypatch.setenv("RL_FORCE_RESIDENCY", "0")
    try:
        for arith in ariths:
            what = f"{label} arith {arith}"
            rl.ctx.set_option("sweep_bracket", 1)
            on = run(WINDOWED, arith)
            assert on[4].rings_in_lds == 0 and on[4].reserved[0] == arith, what
            assert np.isfinite(on[0]).all() and on[2].sum() > 0, what
            rl.ctx.set_option("sweep_bracket", 0)
            off = run(WINDOWED, arith)
            rl.ctx.set_option("sweep_bracket", 1)
            brute = run(BRUTE, arith)
            assert off[4].rings_in_lds == 0 and brute[4].rings_in_lds == 0, what
            _bits(what + ", bracket on against off", on[:4], off[:4])
            _bits(what + ", windowed against brute", on[:4], brute[:4])
    finally:
        rl.ctx.set_option("sweep_bracket", 1)


def _half_widths(rl, t, cx, cy, k, length, ringL, ringR, N):
    pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
    orc.fill_bounds(pts, ringL, ringR, 100.0)
    return rl.batch.half_widths_from_bounds(pts)


@pytest.mark.parametrize("N", [104, 131])
def test_smallest_staged_width_rings(rl, fits, rings, monkeypatch, N):
    t, cx, cy, k, length = spline(fits, "c100")
    B = 3
    wl, wr = _half_widths(rl, t, cx, cy, k, length, rings[0], rings[1], N)
    widths = rl.batch.width_batch(wl, wr, B, seed=N)
    ist = rl.batch.default_i_start(len(cx), k, 2, seed=0)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    _on_off_brute(rl, monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, search=search,
                                                                                 arith=arith), f"monza widths N={N}")


def test_kart_hairpins_width_form(rl, monkeypatch):
    t, cx, cy, k, length, ringL, ringR = kart_cases.case("base")
    N, B = 200, 3
    widths = kart_cases.widths("base", N, B, seed=5)
    ist = kart_cases.i_start("base", 2)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    _on_off_brute(rl, monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, ist, search=search,
                                                                                 arith=arith), "kart widths N=200")


def test_reversed_rings(rl, monkeypatch):
    t, cx, cy, k, length, ringL, ringR = kart_cases.case("rings_reversed")
    N, B = 200, 2
    ist = kart_cases.i_start("rings_reversed", 1)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    trk.set_rings(ringL, ringR)
    _on_off_brute(rl, monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_SHARED_RINGS, None, ist, search=search,
                                                                                 B=B, arith=arith), "kart rings reversed")


def test_duplicated_vertex_inside_a_window(rl, fits, rings, monkeypatch):
    t, cx, cy, k, length = spline(fits, "c100")
    N, B = 200, 2
    ringL = np.insert(rings[0], [13, 13, len(rings[0]) // 2], rings[0][[13, 13, len(rings[0]) // 2]], axis=0)   # vertex 13 three times in a row
    ringR = np.insert(rings[1], [len(rings[1]) - 1], rings[1][[len(rings[1]) - 1]], axis=0)                      # the last vertex twice: a zero edge at the seam
    assert (np.diff(ringL, axis=0) == 0).all(axis=1).sum() == 3 and (np.diff(ringR, axis=0) == 0).all(axis=1).sum() == 1
    ist = golden("G7_run_min_curvature_qp.npz")["c100_N200_it3_seed1_i_start"][:2]
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    trk.set_rings(np.ascontiguousarray(ringL), np.ascontiguousarray(ringR))
    _on_off_brute(rl, monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_SHARED_RINGS, None, ist, search=search,
                                                                                 B=B, arith=arith), "monza rings with zero edges")


def test_start_lines_off_the_centre_line(rl, fits, rings, monkeypatch):
    t, cx, cy, k, length = spline(fits, "c100")
    N, B, max_iter = 200, 3, 2
    m = len(cx) - k
    ctrl0 = []
    for b in range(B):   # instance b's line: the track's, shifted by 2 + b / 2 metres along a direction that turns round the lap
        a = 2.0 * np.pi * (np.arange(m) / m + b / 3.0)
        x1, y1 = cx[:m] + (2.0 + 0.5 * b) * np.cos(a), cy[:m] + (2.0 + 0.5 * b) * np.sin(a)
        ctrl0.append(np.column_stack([np.concatenate([x1, x1[:k]]), np.concatenate([y1, y1[:k]])]))
    ctrl0 = np.stack(ctrl0)
    rows = rl.batch.default_i_start_batch(len(cx), k, max_iter, B, seed=3)
    wl, wr = _half_widths(rl, t, cx, cy, k, length, rings[0], rings[1], N)
    widths = rl.batch.width_batch(wl, wr, B, seed=1234)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    _on_off_brute(rl, monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, rows, search=search,
                                                                                 arith=arith, ctrl0=ctrl0), "start lines 2-3 m off")


def test_g12_under_raise_mode(rl, monkeypatch):
    g = golden("G12_numpy_raise_semantics.npz")
    t, cx, cy, k = g["t"], g["cx"], g["cy"], int(g["k"])
    N, B = 300, 2
    ist = g["sweep_N300_i_start"][:2]
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    trk.set_rings(g["ringL"], g["ringR"])
    rl.ctx.set_numpy_raise(True)
    try:
        _on_off_brute(rl, monkeypatch, lambda search, arith: rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_SHARED_RINGS, None, ist,
                                                                                     search=search, B=B, arith=arith), "G12 raise mode")
    finally:
        rl.ctx.set_numpy_raise(False)
