"""Test helper: the MGKT kart circuit (examples/race_track/mgkt/) as inputs of the min-curvature sweep, from fixture
G14_kart_track.npz (FITPACK's output and the boundary rings as the reference produced them: no scipy here).

The track is tight -- hairpins of 6.6 m radius, half-widths of 3 .. 4.3 m, strands 27 m apart -- so the windowed ring search
loses its certificate on about one sample in eight, steps fail, and solved lines touch the boundary.  A case is the tuple
(t, cx, cy, k, length, ringL, ringR); the variants turn what the Monza fixtures never vary (ring orientation, start vertex,
direction of travel, scale, distance from the origin)."""
import numpy as np

from conftest import golden
from oracle import oracle as orc

NAMES = ("base", "rings_reversed", "rings_rolled", "driven_backwards", "small", "far")
ROLL = 137
SCALE = 0.125                        # a power of two: every coordinate of `small` is the exact eighth of `base`'s
FAR = (3.0e5, -7.0e5)                # test_window_scan_quick_sign_pass_far_from_the_origin's offset
FLOOR = {"small": 1.5 * SCALE}       # batch.width_batch's floor of 1.5 m, in the case's own scale

# seed of batch.default_i_start per case: 0, except where the oracle's run from seed 0 (N = 400, two outer iterations) has no
# failing step -- `driven_backwards`; there the first seed of 0..11 whose run fails a step before its last pass (oracle, CPU).
SEED = {"driven_backwards": 6}

_cache = {}


def fixture():
    if "g" not in _cache:
        _cache["g"] = golden("G14_kart_track.npz")
    return _cache["g"]


def _fit(g, tag):
    return g[f"{tag}_t"], g[f"{tag}_cx"], g[f"{tag}_cy"], int(g[f"{tag}_k"]), float(g[f"{tag}_length"])


def case(name):
    """(t, cx, cy, k, length, ringL, ringR) of the named case; the outer boundary is the left ring (mintime_problem.mgkt_problem)."""
    g = fixture()
    t, cx, cy, k, length = _fit(g, "c")
    ringL, ringR = g["ringL"], g["ringR"]
    if name == "base":
        pass
    elif name == "rings_reversed":
        ringL, ringR = ringL[::-1], ringR[::-1]
    elif name == "rings_rolled":
        ringL, ringR = np.roll(ringL, ROLL, axis=0), np.roll(ringR, ROLL, axis=0)
    elif name == "driven_backwards":                       # the centre line fitted from the reversed point order: left is right
        t, cx, cy, k, length = _fit(g, "cb")
        ringL, ringR = ringR, ringL
    elif name == "small":                                  # rings every 0.25 m: the same 426 and 412 vertices
        cx, cy, length, ringL, ringR = cx * SCALE, cy * SCALE, length * SCALE, ringL * SCALE, ringR * SCALE
    elif name == "far":
        off = np.array(FAR)
        cx, cy, ringL, ringR = cx + off[0], cy + off[1], ringL + off, ringR + off
    else:
        raise KeyError(name)
    return t, cx.copy(), cy.copy(), k, length, np.ascontiguousarray(ringL), np.ascontiguousarray(ringR)


def i_start(name, max_iter):
    """The case's pinned sweep order: start index per outer iteration."""
    from spline_trajectory_optimization_amd import batch
    c = case(name)
    return batch.default_i_start(len(c[1]), c[3], max_iter, seed=SEED.get(name, 0))


def centre_table(name, N):
    """The bounds-filled table of the case's centre line at N uniform parameters (the oracle's sample_along + fill_bounds)."""
    key = ("table", name, N)
    if key not in _cache:
        t, cx, cy, k, length, ringL, ringR = case(name)
        pts = orc.sample_along(t, cx, cy, k, length, np.linspace(0.0, 1.0, N, endpoint=False))
        _cache[key] = orc.fill_bounds(pts, ringL, ringR, 100.0)
    return _cache[key]


def widths(name, N, B, seed):
    """Width-form bounds [B,N,2]: batch.width_batch on the half-widths of the case's centre table, the floor passed explicitly."""
    from spline_trajectory_optimization_amd import batch
    wl, wr = batch.half_widths_from_bounds(centre_table(name, N))
    return batch.width_batch(wl, wr, B, seed=seed, floor=FLOOR.get(name, 1.5))


# ---- plain numpy restatement of the windowed search's certificate (csrc/rl_device.hpp: search_ring_windowed)
CHUNK = 8


def chunk_circles(ring):
    """Centre and radius of the circle about each chunk of CHUNK consecutive edges (up to 9 vertices; the last chunk may be
    partial and closes onto vertex 0), as k_sweep's prologue forms them (csrc/rl_sweep.hpp): the centre of the chunk's bounding
    box and the largest distance from it to a vertex of the chunk."""
    n = len(ring)
    closed = np.vstack([ring, ring[:1]])
    cen, rad = [], []
    for e0 in range(0, n, CHUNK):
        v = closed[e0:min(e0 + CHUNK, n) + 1]
        m = 0.5 * (v.min(axis=0) + v.max(axis=0))
        cen.append(m); rad.append(float(np.hypot(*(v - m).T).max()) * (1.0 + 1e-12))
    return np.array(cen), np.array(rad)


def chunk_separation(ring):
    """sep[c]: the smallest gap between chunk c's circle and the circle of any chunk that is not c or one of its two ring
    neighbours (negative: they overlap)."""
    cen, rad = chunk_circles(ring)
    C = len(cen)
    gap = np.hypot(cen[:, None, 0] - cen[None, :, 0], cen[:, None, 1] - cen[None, :, 1]) - rad[:, None] - rad[None, :]
    idx = np.arange(C)
    near = np.minimum((idx[:, None] - idx[None, :]) % C, (idx[None, :] - idx[:, None]) % C) <= 1
    return np.where(near, np.inf, gap).min(axis=1) * (1.0 - 1e-9) - 1e-9


def uncertified_share(points, ring, bound_cols):
    """(share of the samples of a bounds-filled table whose crossing of `ring` fails sep[chunk of the crossed edge] > 2 d with
    d = distance from the sample to its bound point, the smallest sep of the ring)."""
    bx, by = points[:, bound_cols[0]], points[:, bound_cols[1]]
    d = np.hypot(bx - points[:, 0], by - points[:, 1]) * (1.0 + 1e-9) + 1e-9
    closed = np.vstack([ring, ring[:1]])
    a, b = closed[:-1], closed[1:]
    ab = b - a
    # the crossed edge: the one the bound point lies on (smallest point-to-segment distance)
    ap = np.stack([bx, by], axis=1)[:, None, :] - a[None]
    s = np.clip((ap * ab[None]).sum(-1) / (ab * ab).sum(-1)[None], 0.0, 1.0)
    edge = np.hypot(*np.moveaxis(ap - s[..., None] * ab[None], -1, 0)).argmin(axis=1)
    sep = chunk_separation(ring)
    return float(np.mean(~(sep[edge // CHUNK] > 2.0 * d))), float(sep.min())
