"""Ring-crossing cases on a lattice and their exact reference (tests/test_ring_crossings_cpu.py, _gpu.py).

The decision under test: which edge of a closed ring does a waypoint's normal segment  p + s d, s in [-1, 1]  cross first.
The rule is the one stated above oracle/mincurv_oracle.c: closest_hit and implemented by csrc/rl_device.hpp (edge_hit):

  * an edge whose two end points are STRICTLY on one side of the line is no crossing;
  * an edge parallel to or lying on the line (den == 0) is no crossing;
  * s = cross(P - p, Q - P) / cross(d, Q - P); |s| > 1 is beyond max_dist and no crossing;
  * the smallest |s| wins, equal |s| keep the LOWEST edge index;
  * no crossing at all: the bound is the waypoint itself.

exact_closest_hit() evaluates that rule in fractions.Fraction on the given doubles.  Every case here is built so that the right
answer is unique AND every operation an implementation performs up to (and including) the bound point is exact in double --
fused or not -- so implementations are compared with the reference bit for bit, with no tolerance and no conditioning filter:

  * The normal is exact: with yaw = -M_PI/2 (the double) the LEFT normal's angle yaw + M_PI/2 is exactly 0.0, with
    yaw = +M_PI/2 the RIGHT normal's angle is; cos(0.0) = 1, sin(0.0) = 0 in every libm, so d = (100, 0) exactly.  A row with
    yaw = -M_PI/2 is asserted on LBX / LBY only, a row with yaw = +M_PI/2 on RBX / RBY only (the other side's direction,
    100 (cos, sin)(+-pi), is not exact; it is covered by the track tests).  The same ring serves as left and right ring.
  * Coordinates are dyadic with at most 20 significant bits (the underflow family adds +-2^-600 and +-2^-590, one bit each).
  * check_exact() -- run by the case builder on every ring and waypoint, never skipped -- proves per vertex and per edge that
    the differences, the products and the cross products are doubles, that the winning s, s d and p + s d are doubles, that a
    rejected crossing (|s| > 1) stays rejected after rounding, and that a losing crossing stays behind the winner after
    rounding.

Families (rings of 4 vertices where the family has such a form; padded to 48, 49, 57, 64 and 65 vertices along edges no test
normal reaches, and rotated so that the decisive edges land on edge 0, the closing edge, a chunk's first and a chunk's last
edge; 48 is the last size at which the windowed search falls back, 57 and 65 leave a partial chunk of 8):

  a  vertex hit: the normal passes through a ring vertex (crossing the ring there; a reflex vertex that only touches the line)
  b  equal distance on opposite sides, the two edges >= 30 indices apart (opposite edges of the 4-ring), both index orders
  c  equal distance on the same side: two distinct edges through one point (edges crossing each other; a revisited vertex)
  d  a ring edge lying on the line: skipped, its neighbours meet the line at its end vertices; waypoint inside that edge
  e  the range limit: |s| == 1 accepted, one lattice step beyond rejected, s == -1; only rejected crossings: the waypoint itself
  f  zero distance: the waypoint on an edge (s = +0.0 and s = -0.0) and on a vertex
  g  a comb crossed 3, 5 and 7 times at distinct distances, nearest on either side (no 4-vertex form: four edges cannot be
     crossed at three distinct distances without a tie)
  h  underflow: end points 2^-600 and 2^-590 off the line on the SAME side (side values' product is 0.0: no crossing) and on
     opposite sides (a crossing)
  i  no hit: the whole ring beyond max_dist, or on one side of the line

Plain Python inside the reference: no numpy scalar reaches a Fraction."""
import functools
import math
from collections import namedtuple
from fractions import Fraction as F

import numpy as np

MAX_DIST = 100.0
YAW_LEFT_EXACT = -math.pi / 2.0    # + M_PI/2 == 0.0: the left normal is (100, 0)
YAW_RIGHT_EXACT = math.pi / 2.0    # - M_PI/2 == 0.0: the right normal is (100, 0)
assert YAW_LEFT_EXACT + math.pi / 2.0 == 0.0 and YAW_RIGHT_EXACT - math.pi / 2.0 == 0.0
SIZES = (4, 48, 49, 57, 64, 65)
NODE_COUNTS = (1, 63, 64, 65, 513)
FAMILIES = "abcdefghi"
K_WIN_EDGES, K_CHUNK = 24, 8       # csrc/rl_device.hpp
TINY, TINY2 = 2.0 ** -600, 2.0 ** -590
X, Y, YAW, LBX, LBY, RBX, RBY = 0, 1, 3, 9, 10, 11, 12


# ---------------------------------------------------------------- the exact reference
def exact_hits(px, py, dx, dy, ring):
    """[(s, edge)] of every edge of the closed polyline `ring` (a sequence of (x, y) doubles, closing edge included) that the
    rule counts as a crossing of the line through p along d -- before the range test |s| <= 1.  Fractions."""
    px, py, dx, dy = F(px), F(py), F(dx), F(dy)
    v = [(F(x) - px, F(y) - py) for x, y in ring]
    side = [ax * dy - ay * dx for ax, ay in v]
    out = []
    n = len(v)
    for j in range(n):
        j1 = j + 1 if j + 1 < n else 0
        ea, eb = side[j], side[j1]
        if (ea > 0 and eb > 0) or (ea < 0 and eb < 0):
            continue
        (ax, ay), (bx, by) = v[j], v[j1]
        sx, sy = bx - ax, by - ay
        den = dx * sy - dy * sx
        if den == 0:
            continue
        out.append(((ax * sy - ay * sx) / den, j))
    return out


def exact_closest_hit(px, py, dx, dy, ring):
    """(s, edge) of the closest crossing within |s| <= 1, ties in |s| to the lowest edge index; None without one."""
    best = None
    for s, j in exact_hits(px, py, dx, dy, ring):
        if abs(s) > 1:
            continue
        if best is None or abs(s) < abs(best[0]):
            best = (s, j)
    return best


def exact_bound(px, py, dx, dy, ring):
    """The bound point as Fractions: p + s d, p itself without a hit."""
    h = exact_closest_hit(px, py, dx, dy, ring)
    s = h[0] if h else F(0)
    return F(px) + s * F(dx), F(py) + s * F(dy)


# ---------------------------------------------------------------- exactness of a case in double arithmetic
def is_double(v):
    return F(float(v)) == v


def sig_bits(x):
    n = abs(F(x).numerator)
    return (n >> ((n & -n).bit_length() - 1)).bit_length() if n else 0


def check_exact(ring, px, py, dx=MAX_DIST, dy=0.0):
    """Assert that an implementation of the rule in double arithmetic, fused or not, performs only exact operations on this
    ring and waypoint up to the bound point (module docstring).  Returns the reference's (s, edge) or None."""
    for c in [px, py] + [c for p in ring for c in p]:
        assert isinstance(c, float) and sig_bits(c) <= 20, c
    fpx, fpy, fdx, fdy = F(px), F(py), F(dx), F(dy)
    v = [(F(x) - fpx, F(y) - fpy) for x, y in ring]
    for ax, ay in v:
        assert all(map(is_double, (ax, ay, ax * fdy, ay * fdx, ax * fdy - ay * fdx))), (px, py, ax, ay)
    n = len(v)
    for j in range(n):
        (ax, ay), (bx, by) = v[j], v[(j + 1) % n]
        ea, eb = ax * fdy - ay * fdx, bx * fdy - by * fdx
        if (ea > 0 and eb > 0) or (ea < 0 and eb < 0):
            # the product may underflow to 0.0 (family h), never to the other sign; nothing else is computed for this edge
            continue
        sx, sy = bx - ax, by - ay
        assert all(map(is_double, (sx, sy, fdx * sy, fdy * sx, fdx * sy - fdy * sx, ax * sy, ay * sx, ax * sy - ay * sx))), (px, py, j)
    hits = exact_hits(px, py, dx, dy, ring)
    best = None
    for s, j in hits:
        if abs(s) <= 1 and (best is None or abs(s) < abs(best[0])):
            best = (s, j)
    for s, j in hits:
        if abs(s) > 1:
            assert abs(float(s)) > 1.0, (px, py, j, s)          # stays rejected after the division's rounding
        elif abs(s) != abs(best[0]):
            assert abs(float(s)) > abs(float(best[0])), (px, py, j, s)   # stays behind the winner
    if best is not None:
        s = best[0]
        assert all(map(is_double, (s, s * fdx, s * fdy, fpx + s * fdx, fpy + s * fdy))), (px, py, s)
    return best


# ---------------------------------------------------------------- ring construction
FAR, TOP = 512.0, 512.0


def far_close(path):
    """Close an open path A .. B (running left to right inside |x| < FAR, |y| < TOP) through the far corners
    (FAR, B.y), (FAR, TOP), (-FAR, TOP), (-FAR, A.y).  No test normal reaches those four edges within max_dist: waypoints
    keep |px| <= 201.  Returns (vertices, index of the top edge: the default place for padding)."""
    ay, by = path[0][1], path[-1][1]
    return list(path) + [(FAR, by), (FAR, TOP), (-FAR, TOP), (-FAR, ay)], len(path) + 1


def pad_ring(core, pads, nr):
    """core with nr - len(core) lattice vertices inserted along the edges named in pads = [(core edge, count | None)]:
    fixed counts first, the one None entry takes the rest.  Edge P -> Q gets P + (Q - P) i / D, i = 1..m, D = 2^k > m."""
    extra = nr - len(core)
    assert extra >= 0, (nr, len(core))
    fixed = sum(c for _, c in pads if c is not None)
    assert fixed <= extra and sum(1 for _, c in pads if c is None) == 1, (pads, extra)
    count = {e: (extra - fixed if c is None else c) for e, c in pads}
    out = []
    for e, p in enumerate(core):
        out.append(p)
        m = count.get(e, 0)
        if m:
            q = core[(e + 1) % len(core)]
            D = 1 << m.bit_length()
            for i in range(1, m + 1):
                out.append((float(F(p[0]) + (F(q[0]) - F(p[0])) * i / D), float(F(p[1]) + (F(q[1]) - F(p[1])) * i / D)))
    assert len(out) == nr
    return out


def rotate(ring, r):
    """The same closed polyline starting at vertex r: edge j becomes edge (j - r) mod n."""
    r %= len(ring)
    return ring[r:] + ring[:r]


def mirror(ring):
    return [(-x, y) for x, y in ring]


def placement_targets(nr, fam):
    """Edge indices the decisive edges are moved to: edge 0, the closing edge, a chunk's first and a chunk's last edge (of a
    chunk in the middle of the ring; family b, whose two edges must stay 31 indices apart, takes chunk 1)."""
    if nr == 4:
        return [("edge0", 0), ("edge1", 1), ("edge2", 2), ("closing", 3)]
    c = 1 if fam == "b" else ((nr + K_CHUNK - 1) // K_CHUNK) // 2
    return [("edge0", 0), ("closing", nr - 1), ("chunk_first", K_CHUNK * c), ("chunk_last", K_CHUNK * c + K_CHUNK - 1)]


# ---------------------------------------------------------------- the families
# A variant: (name, core vertices, pads, waypoints).  A waypoint: (px, py, want) with want = the set of bound x the family
# expects (the winner of an opposite-side tie depends on the edge order, so both are listed), or None: no hit, the bound is
# the waypoint.  The first waypoint is the PRIMARY one: its decisive edges are what the placements move around.
def _variants(fam, small):
    a, b = TINY, TINY2
    if fam == "a":
        if small:
            return [("diamond", [(50.0, 0.0), (10.0, 40.0), (-25.0, 0.0), (10.0, -40.0)], None,
                     [(25.0, 0.0, {50.0}), (0.0, 0.0, {-25.0}), (12.5, 0.0, {50.0, -25.0})])]
        core, top = far_close([(-300.0, 20.0), (-35.0, 20.0), (-25.0, 0.0), (-15.0, 20.0), (40.0, 30.0), (50.0, 0.0), (60.0, -30.0), (300.0, -30.0)])
        return [("cross+reflex", core, [(top, None)],
                 [(25.0, 0.0, {50.0}),              # through the vertex where the ring crosses the line
                  (0.0, 0.0, {-25.0}),              # the reflex vertex: the ring only touches the line
                  (12.5, 0.0, {50.0, -25.0}),       # both vertices at the same distance: four candidate edges
                  (-25.0, 0.0, {-25.0})])]          # the waypoint ON the reflex vertex
    if fam == "b":
        way = [(0.0, 0.0, {-25.0, 25.0}), (0.0, 8.0, {-25.0, 25.0}), (-12.5, -8.0, {-25.0}), (12.5, 0.0, {25.0})]
        if small:
            sq = [(-25.0, -40.0), (25.0, -40.0), (25.0, 40.0), (-25.0, 40.0)]
            return [("square", sq, None, way)]
        core, top = far_close([(-25.0, -40.0), (-25.0, 40.0), (25.0, 40.0), (25.0, -40.0)])
        pads = [(1, 30), (top, None)]              # 30 vertices BETWEEN the two tied edges: 31 indices apart
        return [("minus_first", core, pads, way), ("plus_first", mirror(core), pads, [(-x, y, {-w for w in want}) for x, y, want in way])]
    if fam == "c":
        if small:
            return [("bowtie", [(40.0, -10.0), (60.0, 10.0), (60.0, -10.0), (40.0, 10.0)], None, [(46.875, 0.0, {50.0})])]
        cross = [(40.0, -10.0), (60.0, 10.0), (100.0, 10.0), (100.0, -10.0), (60.0, -10.0), (40.0, 10.0), (-400.0, 10.0),
                 (-400.0, -200.0), (40.0, -200.0)]
        revisit = [(40.0, -10.0), (50.0, 0.0), (60.0, 10.0), (100.0, 10.0), (100.0, -10.0), (60.0, -10.0), (50.0, 0.0), (40.0, 10.0),
                   (-400.0, 10.0), (-400.0, -200.0), (40.0, -200.0)]
        way = [(0.0, 0.0, {50.0}),                  # two edges through (50, 0) at s = 1/2; the edge at x = 100 at s = 1
               (62.5, 0.0, {50.0}),                 # the same point from the other side
               (75.0, 0.0, {50.0, 100.0})]          # three-way tie: (50, 0) twice on the minus side, (100, 0) on the plus side
        return [("edges_cross", cross, [(7, None)], way), ("vertex_revisited", revisit, [(9, None)], way)]
    if fam == "d":
        way = [(0.0, 0.0, {25.0}), (50.0, 0.0, {25.0, 75.0}), (62.5, 0.0, {75.0}), (100.0, 0.0, {75.0}), (37.5, 0.0, {25.0})]
        if small:
            return [("rectangle", [(25.0, 0.0), (75.0, 0.0), (75.0, 40.0), (25.0, 40.0)], None, way)]
        core, top = far_close([(-300.0, -30.0), (15.0, -30.0), (25.0, 0.0), (75.0, 0.0), (85.0, 30.0), (300.0, 30.0)])
        return [("collinear", core, [(top, None)], way)]
    if fam == "e":
        if small:
            return [("rectangle", [(-100.0, -30.0), (100.0, -30.0), (100.0, 30.0), (-100.0, 30.0)], None,
                     [(0.0, 0.0, {-100.0, 100.0}), (200.0, 0.0, {100.0}), (-200.0, 0.0, {-100.0}), (200.5, 0.0, None), (-200.5, 0.0, None)])]
        core, top = far_close([(-100.0, -30.0), (-100.0, 30.0), (100.0, 30.0), (100.0, -30.0), (100.5, -30.0), (100.5, 30.0)])
        return [("limits", core, [(top, None)],
                 [(0.0, 0.0, {-100.0, 100.0}),      # s = -1 and s = +1 accepted (a tie at the limit), 1.005 rejected
                  (200.5, 0.0, {100.5}),            # s = -1 accepted, -1.005 rejected
                  (-200.0, 0.0, {-100.0}),          # s = +1 accepted, the far connector rejected
                  (201.0, 0.0, None),               # -1.005 and -1.01: only rejected crossings
                  (-200.5, 0.0, None),              # 1.005: rejected
                  (-50.0, 0.0, {-100.0})])]
    if fam == "f":
        if small:
            return [("quad", [(-10.0, -30.0), (10.0, 30.0), (40.0, 30.0), (60.0, -30.0)], None,
                     [(0.0, 0.0, {0.0}), (50.0, 0.0, {50.0}), (10.0, 30.0, {10.0}), (5.0, 15.0, {5.0})])]
        core, top = far_close([(-10.0, -30.0), (0.0, 0.0), (20.0, 30.0), (40.0, 30.0), (60.0, -30.0)])
        return [("on_ring", core, [(top, None)],
                 [(0.0, 0.0, {0.0}),                # on a vertex (px = +0.0: p + (+-0) d must be +0.0)
                  (10.0, 15.0, {10.0}),             # on an edge running up: s = +0.0
                  (50.0, 0.0, {50.0}),              # on an edge running down: s = -0.0
                  (45.0, 15.0, {45.0}),
                  (60.0, -30.0, {60.0})])]          # on a vertex whose other edge lies on the line
    if fam == "g":
        if small:
            return []
        path = []
        for k in range(7):                          # vertical edges at x = 0, 25, .., 150, running up and down in turn
            x = 25.0 * k
            path += [(x, -10.0), (x, 10.0)] if k % 2 == 0 else [(x, 10.0), (x, -10.0)]
        core, top = far_close(path)
        return [("comb", core, [(top, None)],
                 [(81.25, 2.0, {75.0}),             # 7 crossings, the nearest on the minus side
                  (6.25, 2.0, {0.0}),               # 5 crossings, the nearest on the minus side
                  (-43.75, 2.0, {0.0}),             # 3 crossings, all on the plus side
                  (93.75, 2.0, {100.0}),            # 7 crossings, the nearest on the plus side
                  (143.75, -2.0, {150.0})])]        # 5 crossings
    if fam == "h":
        out = []
        for name, ya, yb, yrest_a, yrest_b, want in (("same_side_plus", a, b, 40.0, 40.0, None), ("same_side_minus", -a, -b, -40.0, -40.0, None),
                                                     ("opposite_minus_plus", -a, b, -40.0, 40.0, {25.0}), ("opposite_plus_minus", a, -b, 40.0, -40.0, {25.0})):
            way = [(0.0, 0.0, want), (125.0, 0.0, want), (-75.0, 0.0, want)]     # opposite sides: s = 1/4, -1 and +1
            if small:   # opposite sides: the fourth vertex far out, so that the ring's other crossing of the line is out of range
                out.append((name, [(24.875, ya), (153.0, yb), (153.0, yrest_b), (-375.125 if want else 24.875, yrest_a)], None,
                            way[:2] if want else way))
            else:
                core, top = far_close([(-300.0, yrest_a), (24.875, ya), (153.0, yb), (300.0, yrest_b)])
                out.append((name, core, [(top, None)], way))
        return out
    if fam == "i":
        way = [(0.0, 0.0, None), (0.0, -100.0, None), (49.5, 8.0, None), (401.0, 0.0, None)]
        if small:
            return [("box", [(150.0, -30.0), (300.0, -30.0), (300.0, 30.0), (150.0, 30.0)], None, way)]
        core, top = far_close([(150.0, -30.0), (150.0, 30.0), (300.0, 30.0), (300.0, -30.0)])
        return [("box", core, [(top, None)], way[:3])]
    raise KeyError(fam)


Case = namedtuple("Case", "family variant nr place ring way hits")
# ring: tuple of (x, y) doubles; way: tuple of (px, py); hits: per waypoint (s Fraction, edge) | None -- the exact reference


def _decisive_edges(ring, px, py):
    """The edges that hold the primary waypoint's winning crossing (all of them on a tie); without a hit the edges of its
    nearest rejected crossing; without any crossing edge 0."""
    hits = exact_hits(px, py, MAX_DIST, 0.0, ring)
    ok = [h for h in hits if abs(h[0]) <= 1]
    pool = ok or hits
    if not pool:
        return [0]
    m = min(abs(s) for s, _ in pool)
    return [j for s, j in pool if abs(s) == m]


def _placed_edges(ring, px, py):
    """Of the decisive edges, the lowest (the winner) and the highest index: the ones the placements move onto the targets."""
    e = _decisive_edges(ring, px, py)
    return sorted({min(e), max(e)})


@functools.lru_cache(maxsize=None)
def cases(fam, nr):
    """Every ring of family `fam` at `nr` vertices: each variant padded, then rotated so that each decisive edge of the primary
    waypoint lands on each placement target.  Every ring and waypoint passes check_exact; the family's expectation (`want`)
    is asserted against the reference; nothing is filtered."""
    out = []
    for name, core, pads, way in _variants(fam, nr == 4):
        base = list(core) if nr == 4 else pad_ring(core, pads, nr)
        assert len(base) == nr
        seen = set()
        for e in _placed_edges(base, way[0][0], way[0][1]):
            for label, target in placement_targets(nr, fam):
                r = (e - target) % nr
                if r in seen:
                    continue
                seen.add(r)
                ring = rotate(base, r)
                if fam == "b" and nr > 4:
                    j0, j1 = sorted(_decisive_edges(ring, way[0][0], way[0][1]))
                    if j1 - j0 < 30:     # the seam fell between the two edges: this index order is the mirrored variant's
                        continue
                hits = []
                for px, py, want in way:
                    h = check_exact(ring, px, py)
                    if want is None:
                        assert h is None, (fam, name, nr, px, py, h)
                    else:
                        assert h is not None and F(px) + h[0] * 100 in {F(w) for w in want}, (fam, name, nr, px, py, h)
                    hits.append(h)
                out.append(Case(fam, name, nr, f"{label}<-{e}", tuple(ring), tuple((px, py) for px, py, _ in way), tuple(hits)))
    _check_family(fam, nr, out)
    return tuple(out)


def _check_family(fam, nr, cs):
    """What a family promises beyond its waypoints' bounds (module docstring), asserted on the generated rings."""
    if not cs:
        assert fam == "g" and nr == 4
        return
    targets = {t for _, t in placement_targets(nr, fam)}
    on_target = set()
    for c in cs:
        on_target |= set(_decisive_edges(list(c.ring), *c.way[0])) & targets
    assert on_target == targets, (fam, nr, on_target)
    if fam == "a":
        for c in cs:        # the vertex is hit: two consecutive edges tie, their common vertex is the bound
            px, py = c.way[0]
            tied = [j for s, j in exact_hits(px, py, MAX_DIST, 0.0, c.ring) if abs(s) == abs(c.hits[0][0])]
            assert len(tied) == 2 and (tied[1] - tied[0]) % nr in (1, nr - 1), tied
    if fam == "b":
        signs = set()
        for c in cs:
            px, py = c.way[0]
            (s0, j0), (s1, j1) = [h for h in exact_hits(px, py, MAX_DIST, 0.0, c.ring) if abs(h[0]) <= 1]
            assert s0 == -s1 and c.hits[0] == (s0, j0)
            assert j1 - j0 >= (30 if nr > 4 else 2), (nr, j0, j1)
            signs.add(s0 > 0)
        assert signs == {True, False}, "the tie must be won by either side somewhere"
    if fam == "g":
        counts = {sum(1 for s, _ in exact_hits(px, py, MAX_DIST, 0.0, cs[0].ring) if abs(s) <= 1) for px, py in cs[0].way}
        assert counts == {3, 5, 7}, counts
    if fam == "h":
        for c in cs:        # the side values' product underflows
            ys = sorted(abs(y) for _, y in c.ring)[:2]
            assert ys == [TINY, TINY2] and (MAX_DIST * TINY) * (MAX_DIST * TINY2) == 0.0


def all_cases():
    return [c for fam in FAMILIES for nr in SIZES for c in cases(fam, nr)]


GROUPS = [(fam, nr) for fam in FAMILIES for nr in SIZES if not (fam == "g" and nr == 4)]
GROUP_IDS = [f"{fam}-{nr}" for fam, nr in GROUPS]


# ---------------------------------------------------------------- tables of rows for a case
def ring_array(case):
    return np.ascontiguousarray(np.array(case.ring, dtype=np.float64))


def case_rows(case):
    """The rows a case offers: (waypoint index, side) with side 0 = yaw -M_PI/2, asserted on LBX / LBY, and side 1 =
    yaw +M_PI/2, asserted on RBX / RBY.  Row 0 and row 1 are the primary waypoint."""
    return [(w, side) for w in range(len(case.way)) for side in (0, 1)]


def row_order(case, N, order):
    """N row indices into case_rows(): "mono" lets the crossed edge advance monotonically along the table (rows without a hit
    last); "jump" alternates between the two halves of that order, so consecutive crossings jump across the ring and the
    windowed search's hint is wrong more often than right; "single0" / "single1": the primary waypoint's two rows."""
    rows = case_rows(case)
    if order.startswith("single"):
        return [int(order[-1])] * N
    key = lambda r: (case.hits[rows[r][0]] is None, case.hits[rows[r][0]][1] if case.hits[rows[r][0]] else 0)  # noqa: E731
    srt = sorted(range(len(rows)), key=key)
    if order == "mono":
        return [srt[(i * len(srt)) // N] for i in range(N)] if N >= len(srt) else srt[:N]
    assert order == "jump"
    half = (len(srt) + 1) // 2
    seq = []
    for lo, hi in zip(srt[:half], srt[half:] + [None]):
        seq += [lo] if hi is None else [lo, hi]
    return [seq[i % len(seq)] for i in range(N)]


def expected_bound(case, w):
    """(bx, by) doubles of waypoint w: exact by construction (check_exact)."""
    px, py = case.way[w]
    h = case.hits[w]
    if h is None:
        return px, py
    return float(F(px) + h[0] * 100), py


@functools.lru_cache(maxsize=None)
def _row_arrays(case):
    rows = case_rows(case)
    wp = np.array([case.way[w] for w, _ in rows], dtype=np.float64)
    side = np.array([sd for _, sd in rows])
    exp = np.array([expected_bound(case, w) for w, _ in rows], dtype=np.float64)
    return wp, side, exp


def table(case, N, order):
    """(points [N,19] with X, Y, YAW set and a recognisable filler in every other column, side [N] (0: LBX / LBY asserted,
    1: RBX / RBY), expected [N,2] bound point of the asserted side)."""
    wp, side, exp = _row_arrays(case)
    idx = np.array(row_order(case, N, order))
    pts = 1000.0 + np.arange(N * 19, dtype=np.float64).reshape(N, 19) * 0.5
    pts[:, [X, Y]] = wp[idx]
    pts[:, YAW] = np.where(side[idx] == 0, YAW_LEFT_EXACT, YAW_RIGHT_EXACT)
    return np.ascontiguousarray(pts), side[idx], np.ascontiguousarray(exp[idx])


def asserted(points, side):
    """[.., N, 2]: LBX / LBY of the rows with side 0, RBX / RBY of the rows with side 1."""
    return np.where((side == 0)[:, None], points[..., [LBX, LBY]], points[..., [RBX, RBY]])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, exp, what):
    """Bit-for-bit equality of two float64 arrays (distinguishes +0.0 from -0.0); the message names the first rows that differ."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(bits(got) != bits(exp))
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first at {bad[:4].tolist()}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def describe(case):
    return f"{case.family}/{case.variant} nr={case.nr} {case.place}"
