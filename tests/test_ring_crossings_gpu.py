"""The ring-crossing search of the HIP kernels (csrc/rl_device.hpp: edge_side / edge_hit / edge_cross under search_ring_brute,
search_ring_culled and search_ring_windowed / scan_window) against the exact reference of tests/ring_cases.py: exact ties on
opposite sides and on one side, vertex hits, collinear edges, the range limit, zero distance, combs, underflowing side values
and rings without a hit, at ring sizes 4, 48, 49 (the first windowed one), 57, 64 and 65, with the decisive edges on edge 0,
the closing edge, a chunk's first and a chunk's last edge, in tables of 1, 63, 64, 65 and 513 nodes whose crossings jump
across the ring or advance along it.

Every asserted bound column must equal the reference BIT FOR BIT: the cases are exact in double arithmetic, fused or not
(ring_cases.check_exact, asserted while the cases are built), so there is no tolerance and no case is filtered.  A row with
yaw = -M_PI/2 is asserted on LBX / LBY, a row with yaw = +M_PI/2 on RBX / RBY (ring_cases' module docstring).

Entry points: rl_fill_bounds (k_fill_bounds: the brute-force search), rl_pose_tables_batch_host in the POSE_GLOBAL form
(k_pose_tables: all three searches, rings in LDS and in the arena) with shared rings and with per-instance bound points.
rl_pose_tables_batch_host needs two nodes, so its tables start at 63."""
import numpy as np
import pytest

import ring_cases as rc
from conftest import golden, spline

pytestmark = pytest.mark.gpu

KEEP = [c for c in range(19) if c not in (rc.LBX, rc.LBY, rc.RBX, rc.RBY)]
ORDERS = ("jump", "mono")


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, ops
    ctx = _lib.Context.get(0)
    ctx.set_arith(_lib.ARITH_DEFAULT)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.ctx = _lib, ops, ctx
    t, cx, cy, k, _ = spline(golden("G1_spline_fits.npz"), "c100")
    ns.track = lambda N: _lib.Track(ctx, t, cx, cy, k, N)   # noqa: E731  (any spline serves: the poses are given, the rings attached)
    yield ns
    ctx.set_arith(_lib.ARITH_DEFAULT)
    ctx.set_option("tables_search", _lib.SEARCH_WINDOWED)
    ctx.set_option("tables_rings", 0)


@pytest.mark.parametrize("fam,nr", rc.GROUPS, ids=rc.GROUP_IDS)
def test_fill_bounds_is_exact(rl, fam, nr):
    """rl_fill_bounds under the fast and the default arithmetic: asserted columns exact, every other column untouched."""
    try:
        for arith in (rl.lib.ARITH_FAST, rl.lib.ARITH_DEFAULT):
            rl.ctx.set_arith(arith)
            for case in rc.cases(fam, nr):
                ring = rc.ring_array(case)
                for N, order in [(1, "single0"), (1, "single1")] + [(N, o) for N in rc.NODE_COUNTS[1:] for o in ORDERS]:
                    pts, side, exp = rc.table(case, N, order)
                    out = rl.ops.fill_bounds(pts.copy(), ring, ring, rc.MAX_DIST)
                    what = f"{rc.describe(case)} arith={arith} N={N} {order}"
                    rc.assert_bits(rc.asserted(out, side), exp, what)
                    rc.assert_bits(out[:, KEEP], pts[:, KEEP], what + ": other columns")
    finally:
        rl.ctx.set_arith(rl.lib.ARITH_DEFAULT)


def poses(tables):
    """X [B,N,5] = (x, y, yaw, 0, v) of B tables of ring_cases.table()."""
    Xg = np.zeros((len(tables), len(tables[0]), 5))
    for b, pts in enumerate(tables):
        Xg[b, :, 0] = pts[:, rc.X]
        Xg[b, :, 1] = pts[:, rc.Y]
        Xg[b, :, 2] = pts[:, rc.YAW]
        Xg[b, :, 4] = 10.0 + np.arange(len(pts))
    return np.ascontiguousarray(Xg)


def configurations(lib):
    return [(s, r) for s in (lib.SEARCH_BRUTE, lib.SEARCH_CULLED, lib.SEARCH_WINDOWED) for r in (0, 1)]


@pytest.mark.parametrize("fam,nr", rc.GROUPS, ids=rc.GROUP_IDS)
def test_pose_tables_shared_rings_are_exact(rl, fam, nr):
    """k_pose_tables with the rings attached to the track, under the brute, culled and windowed searches, rings in LDS and in
    the arena: asserted columns exact in every configuration (hence equal across the six); the poses come back as given.
    Both node orders ride in one launch (B = 2).

    Nothing the library reports says which search ran: no statistic, context query or output of rl_pose_tables_batch_* names
    the mode in effect, and this test adds no kernel hook for it.  That rings of 49 vertices and more take the windowed path
    under SEARCH_WINDOWED rests on reading tables_chunk_tables (nL > 2 * kWinEdges = 48); ring sizes 48 and 49 sit on both
    sides of that threshold here."""
    lib = rl.lib
    trk = rl.track(64)
    try:
        for case in rc.cases(fam, nr):
            trk.set_rings(rc.ring_array(case), rc.ring_array(case))
            for N in rc.NODE_COUNTS[1:]:
                tabs = [rc.table(case, N, o) for o in ORDERS]
                Xg = poses([t[0] for t in tabs])
                seen = []
                for search, arena in configurations(lib):
                    rl.ctx.set_option("tables_search", search)
                    rl.ctx.set_option("tables_rings", arena)
                    pts = rl.ops.pose_tables_host(trk, lib.POSE_GLOBAL, Xg, None, lib.BOUNDS_SHARED_RINGS, None)
                    got = np.stack([rc.asserted(pts[b], tabs[b][1]) for b in range(len(tabs))])
                    what = f"{rc.describe(case)} search={search} arena={arena} N={N}"
                    for b, o in enumerate(ORDERS):
                        rc.assert_bits(got[b], tabs[b][2], f"{what} {o}")
                    rc.assert_bits(pts[..., [rc.X, rc.Y, rc.YAW]], Xg[..., [0, 1, 2]], what + ": poses")
                    seen.append(got)
                for got in seen[1:]:
                    rc.assert_bits(got, seen[0], f"{rc.describe(case)} N={N}: configurations disagree")
    finally:
        rl.ctx.set_option("tables_search", lib.SEARCH_WINDOWED)
        rl.ctx.set_option("tables_rings", 0)


QUADS = [("a", "b", "d", "h"), ("e", "f", "h", "i"), ("c", "h", "b", "e"), ("g", "i", "h", "f")]


@pytest.mark.parametrize("nr", rc.SIZES)
def test_bound_points_batch_of_different_families(rl, nr):
    """BOUNDS_POINTS: one launch of B = 4 instances, each with another family's ring of the same size (a degenerate neighbour
    must not leak into an instance): asserted columns exact, and instance b of the batch == the same instance alone, all 19
    columns bit for bit."""
    lib = rl.lib
    trk = rl.track(nr)      # the points form takes track.N vertices per ring
    try:
        for q, quad in enumerate(QUADS):
            quad = tuple("c" if (f == "g" and nr == 4) else f for f in quad)
            picks = [rc.cases(f, nr)[(q + 3 * b) % len(rc.cases(f, nr))] for b, f in enumerate(quad)]
            bounds = np.ascontiguousarray(np.stack([np.concatenate([rc.ring_array(c), rc.ring_array(c)], 1) for c in picks]))
            for N, order in ((65, "jump"), (513, "mono"), (64, "jump")):
                tabs = [rc.table(c, N, order) for c in picks]
                Xg = poses([t[0] for t in tabs])
                for search, arena in ((lib.SEARCH_WINDOWED, 0), (lib.SEARCH_WINDOWED, 1), (lib.SEARCH_CULLED, 0), (lib.SEARCH_BRUTE, 0)):
                    rl.ctx.set_option("tables_search", search)
                    rl.ctx.set_option("tables_rings", arena)
                    pts = rl.ops.pose_tables_host(trk, lib.POSE_GLOBAL, Xg, None, lib.BOUNDS_POINTS, bounds)
                    for b, c in enumerate(picks):
                        what = f"{rc.describe(c)} as instance {b} of {quad} search={search} arena={arena} N={N}"
                        rc.assert_bits(rc.asserted(pts[b], tabs[b][1]), tabs[b][2], what)
                        one = rl.ops.pose_tables_host(trk, lib.POSE_GLOBAL, np.ascontiguousarray(Xg[b:b + 1]), None, lib.BOUNDS_POINTS,
                                                      np.ascontiguousarray(bounds[b:b + 1]))
                        rc.assert_bits(one[0], pts[b], what + ": alone")
    finally:
        rl.ctx.set_option("tables_search", lib.SEARCH_WINDOWED)
        rl.ctx.set_option("tables_rings", 0)
