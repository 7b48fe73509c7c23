"""CPU statement of rl_frenet_batch_* and rl_frenet_resample_* (csrc/rl_frenet.hpp) in numpy, written independently of the
kernels' search: no circles, no pruning, no hints.

Projection: the closed centre line (RaceTrack.centerline_pieces()) is sampled SAMPLES_PER_PIECE times per piece; every sample
that is a local minimum of the distance on the cyclic grid is polished by Newton on f(s) = (c(s) - p) . c'(s), kept inside the
two neighbouring samples; the smallest polished distance wins.  Next to the result come the conditioning figures the GPU tests
assert on their inputs: the gap between the best and the second-best local minimum [m] and g = f'(s) / |c'(s)|^2 at the foot.

Resample: rotate the line to start behind its wrap, bridge the wrap pair with + L, search, interpolate linearly in s."""
import numpy as np

SAMPLES_PER_PIECE = 16
MIN_GAP, MIN_G = 1e-6, 0.1      # the issue's conditions on a test's inputs
TOL = 1e-9                      # s (cyclic) and n [m], xi [rad], g: GPU against this twin, and round trips


def curve(pieces, s, der=0):
    """x, y (der = 0), their first (1) or second (2) derivatives at abscissae s in [0, L]."""
    ss, cxs, cys = pieces
    M = len(ss) - 1
    j = np.clip(np.searchsorted(ss, s, side="right") - 1, 0, M - 1)
    d = s - ss[j]
    out = []
    for c in (cxs, cys):
        c0, c1, c2, c3 = c[0, j], c[1, j], c[2, j], c[3, j]
        out.append(((c0 * d + c1) * d + c2) * d + c3 if der == 0 else
                   (3.0 * c0 * d + 2.0 * c1) * d + c2 if der == 1 else 6.0 * c0 * d + 2.0 * c1)
    return out[0], out[1]


def _f(pieces, s, px, py):
    x, y = curve(pieces, s)
    dx, dy = curve(pieces, s, 1)
    d2x, d2y = curve(pieces, s, 2)
    ex, ey = x - px, y - py
    return ex * dx + ey * dy, dx * dx + dy * dy + ex * d2x + ey * d2y, ex * ex + ey * ey


def project(pieces, points, yaw=None):
    """points [P,2] -> (fr [P,4] = (s, n, xi, g), gap [P]): the global minimiser and the margin it wins by."""
    ss = pieces[0]
    M, L = len(ss) - 1, ss[-1]
    K = SAMPLES_PER_PIECE
    grid = (ss[:-1, None] + (ss[1:] - ss[:-1])[:, None] * (np.arange(K) / K)[None, :]).reshape(-1)   # [M K], increasing
    gx, gy = curve(pieces, grid)
    pts = np.asarray(points, dtype=np.float64)
    D = (gx[None, :] - pts[:, 0:1]) ** 2 + (gy[None, :] - pts[:, 1:2]) ** 2
    is_min = (D <= np.roll(D, 1, axis=1)) & (D <= np.roll(D, -1, axis=1))
    ip, ig = np.nonzero(is_min)
    px, py = pts[ip, 0], pts[ip, 1]
    S = len(grid)
    lo = np.where(ig > 0, grid[ig - 1], grid[-1] - L)           # unwrapped bracket around the sample
    hi = np.where(ig < S - 1, grid[(ig + 1) % S], L)
    x = grid[ig].copy()
    for _ in range(60):
        f, fp, _ = _f(pieces, np.mod(x, L), px, py)
        lo, hi = np.where(f < 0, np.maximum(lo, x), lo), np.where(f < 0, hi, np.minimum(hi, x))
        with np.errstate(divide="ignore", invalid="ignore"):
            xn = np.where(fp > 0, x - f / fp, np.nan)
        x = np.where((xn >= lo) & (xn <= hi), xn, 0.5 * (lo + hi))
    s = np.mod(x, L)
    s = np.where(s >= L, 0.0, s)
    f, fp, D2 = _f(pieces, s, px, py)
    dist = np.sqrt(D2)
    P = len(pts)
    fr, gap = np.zeros((P, 4)), np.full(P, np.inf)
    for p in range(P):
        sel = np.nonzero(ip == p)[0]
        order = sel[np.argsort(dist[sel], kind="stable")]
        w = order[0]
        cyc = np.abs((s[order] - s[w] + L / 2) % L - L / 2)
        others = order[cyc > 1e-6]                               # polished copies of the same foot are one minimum
        if len(others):
            gap[p] = dist[others[0]] - dist[w]
        dx, dy = curve(pieces, s[w:w + 1], 1)
        cx, cy = curve(pieces, s[w:w + 1])
        v = np.hypot(dx[0], dy[0])
        fr[p, 0] = s[w]
        fr[p, 1] = ((pts[p, 0] - cx[0]) * -dy[0] + (pts[p, 1] - cy[0]) * dx[0]) / v
        if yaw is not None:
            dd = yaw[p] - np.arctan2(dy[0], dx[0])
            fr[p, 2] = np.arctan2(np.sin(dd), np.cos(dd))
        fr[p, 3] = fp[w] / (v * v)
    return fr, gap


def line_tables(race_track, X):
    """[B,P,19] tables with X, Y, YAW = RaceTrack.frenet_to_global of the poses X [B,P,6] and SPEED = X[..., 5]."""
    pts = np.zeros(X.shape[:2] + (19,))
    for b in range(len(X)):
        g = np.asarray(race_track.frenet_to_global(X[b, :, 0], X[b, :, 1], X[b, :, 2]))
        pts[b, :, 0], pts[b, :, 1], pts[b, :, 3], pts[b, :, 4] = g[:, 0], g[:, 1], g[:, 2], X[b, :, 5]
    return pts


def two_leg_pieces():
    """A closed track with two parallel straights 6 m apart (y = 0 driven towards +x, y = 6 towards -x) joined by half
    circles of radius 3 m: scipy CubicSpline(bc_type="periodic") through points every 5 m, chord-length abscissa."""
    from scipy.interpolate import CubicSpline
    xs = np.arange(0.0, 100.0, 5.0)
    th = np.linspace(-np.pi / 2, np.pi / 2, 7)[1:-1]
    p = np.vstack([np.c_[xs, 0 * xs], [[100.0, 0.0]], np.c_[100 + 3 * np.cos(th), 3 + 3 * np.sin(th)],
                   np.c_[xs[::-1] + 5.0, 0 * xs + 6.0], [[0.0, 6.0]], np.c_[-3 * np.cos(th), 3 - 3 * np.sin(th)]])
    loop = np.vstack([p, p[:1]])
    s = np.r_[0.0, np.cumsum(np.hypot(*np.diff(loop, axis=0).T))]
    sx, sy = CubicSpline(s, loop[:, 0], bc_type="periodic"), CubicSpline(s, loop[:, 1], bc_type="periodic")
    as_c = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    return as_c(sx.x), as_c(sx.c), as_c(sy.c)


def project_batch(pieces, points, yaw=None):
    """points [B,P,2|19] -> (fr [B,P,4], gap [B,P]); stride 19 reads YAW from column 3."""
    pts = np.asarray(points)
    out = [project(pieces, pts[b, :, :2], pts[b, :, 3] if pts.shape[2] == 19 else (None if yaw is None else yaw[b]))
           for b in range(len(pts))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def assert_well_conditioned(tag, fr, gap):
    print(f"[frenet {tag}] conditioning: best vs second-best local minimum {gap.min():.2e} m, min g {fr[..., 3].min():.3f}")
    assert gap.min() >= MIN_GAP and fr[..., 3].min() >= MIN_G


def cyclic(a, b, L):
    """|a - b| on the circle of circumference L."""
    return np.abs((np.asarray(a) - b + L / 2) % L - L / 2)


def resample(fr, vals, s_nodes, L):
    """fr [P,4], vals [P,C] or None, s_nodes [Nn] -> (out [Nn,2+C], status)."""
    fr = np.asarray(fr)
    P = len(fr)
    C = 0 if vals is None else vals.shape[1]
    out = np.zeros((len(s_nodes), 2 + C))
    s = fr[:, 0]
    desc = np.nonzero(np.roll(s, -1) <= s)[0]
    if len(desc) != 1 or not np.isfinite(fr[:, :3]).all():
        return out, 1
    k0 = (desc[0] + 1) % P
    idx = (k0 + np.arange(P)) % P
    r = s[idx]
    q = np.mod(np.asarray(s_nodes, dtype=np.float64), L)
    m = np.searchsorted(r, q, side="right") - 1                 # -1: before the first point, i.e. inside the wrap pair
    il, ir = idx[m % P], idx[(m + 1) % P]
    sl = np.where(m < 0, r[-1] - L, r[m % P])
    sr = np.where(m < 0, r[0], np.where(m == P - 1, r[0] + L, r[(m + 1) % P]))
    lerp = lambda vl, vr: (vr - vl) / (sr - sl) * (q - sl) + vl  # noqa: E731
    out[:, 0] = lerp(fr[il, 1], fr[ir, 1])
    dxi = fr[ir, 2] - fr[il, 2]
    out[:, 1] = lerp(fr[il, 2], np.arctan2(np.sin(dxi), np.cos(dxi)) + fr[il, 2])
    for c in range(C):
        out[:, 2 + c] = lerp(vals[il, c], vals[ir, c])
    return out, 0


def guess(fr, speed, s_nodes, kappa, L, base_speed, base_time):
    """batch.min_time_guess_from_lines_torch for one instance on the host: (X0 [Nn,6], T0 [Nn], status); the centre-line guess
    from (base_speed, base_time) where the line cannot be used."""
    Nn = len(s_nodes)
    res, st = resample(fr, speed[:, None], s_nodes, L)
    X = np.zeros((Nn, 6))
    X[:, 0] = s_nodes
    ds = np.r_[s_nodes[1:], L] - s_nodes
    with np.errstate(divide="ignore", invalid="ignore"):
        T = ds * (1.0 - res[:, 0] * kappa) / (res[:, 2] * np.cos(res[:, 1]))
    if st == 0 and np.isfinite(T).all() and (T > 0).all():
        X[:, 1], X[:, 2], X[:, 5] = res[:, 0], res[:, 1], res[:, 2]
        return X, T, 0
    X[:, 5] = base_speed
    return X, np.array(base_time, dtype=np.float64), 1 if st else 2
