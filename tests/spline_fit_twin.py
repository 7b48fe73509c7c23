"""numpy twin of csrc/rl_spline_fit.hpp and the cases its tests share (tests/test_start_lines_cpu.py, _gpu.py).

The twin solves the same problem the same way in float64 -- periodic least squares on GIVEN knots by the normal equations,
a Cholesky factorisation whose pivots decide the rank -- so that the tolerance rule and the rank rule can be checked against
FITPACK with no GPU:

    max|c - c_FITPACK| <= 4 eps cond2(G) max|c_FITPACK|          (forward error of the normal equations; the factor 4
                                                                  covers a different summation order and fma)
    rank deficient  <=>  smallest pivot <= 1e-12 * largest diagonal of G, or a pivot that is not positive
"""
import numpy as np
from scipy import interpolate

EPS = np.finfo(np.float64).eps
RANK_TOL = 1e-12
COND_MAX = 1e4     # every accuracy case is asserted to be at most this badly conditioned


def uniform_knots(k, m):
    """Uniform periodic knots with m intervals on [0, 1]."""
    t = np.arange(-k, m + k + 1, dtype=np.float64) / m
    n = m + k
    for j in range(1, k + 1):     # the outer knots exactly one period from their images, as FITPACK (clocur) sets them itself
        t[k - j] = t[n - j] - 1.0
        t[n + j] = t[k + j] + 1.0
    return t


def chord_u(xy):
    """Chord-length parameters of the closed polygon through xy [P,2]: u_0 = 0, the perimeter includes the closing chord."""
    d = np.hypot(*(np.roll(xy, -1, axis=0) - xy).T)
    return np.concatenate([[0.0], np.cumsum(d)[:-1]]) / d.sum()


def design(t, k, u):
    """A [P, m]: the periodic design matrix, basis function j + m folded onto j (scipy's periodic layout)."""
    t = np.asarray(t, dtype=np.float64)
    n = len(t) - k - 1
    m = n - k
    u = np.where(np.asarray(u, dtype=np.float64) == 1.0, 0.0, u)
    A = interpolate.BSpline.design_matrix(u, t, k).toarray()
    A[:, :k] += A[:, m:]
    return A[:, :m]


def normal_matrix(t, k, u):
    A = design(t, k, u)
    return A.T @ A


def cholesky_pivots(G):
    """(L, pivots) of the Cholesky factorisation of G in its natural order; a non-positive pivot leaves NaN behind it, as in
    the kernel."""
    m = len(G)
    L = np.zeros_like(G)
    piv = np.zeros(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(m):
            piv[j] = G[j, j] - L[j, :j] @ L[j, :j]
            L[j, j] = np.sqrt(piv[j])
            L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, piv


def twin_fit(t, k, xy, u=None, c0=None):
    """(ctrl [n,2], stats [4]) as rl_spline_fit_batch_* returns them for one instance; status != 0: ctrl = c0."""
    t = np.asarray(t, dtype=np.float64)
    xy = np.asarray(xy, dtype=np.float64)[:, :2]
    n = len(t) - k - 1
    m = n - k
    fail = (np.full((n, 2), np.nan) if c0 is None else np.asarray(c0, dtype=np.float64).copy())
    if u is None:
        with np.errstate(invalid="ignore", divide="ignore"):
            u = chord_u(xy)
    u = np.asarray(u, dtype=np.float64)
    if not (np.isfinite(xy).all() and np.isfinite(u).all() and (u >= 0).all() and (u <= 1).all()):
        return fail, np.array([2.0, np.nan, np.nan, np.nan])
    A = design(t, k, u)
    G = A.T @ A
    L, piv = cholesky_pivots(G)
    finite = piv[np.isfinite(piv)]
    ratio = finite.min() / G.diagonal().max()
    if not (np.isfinite(piv).all() and finite.min() > RANK_TOL * G.diagonal().max()):
        return fail, np.array([1.0, np.nan, np.nan, ratio])
    c = np.linalg.solve(L.T, np.linalg.solve(L, A.T @ xy))
    r = np.hypot(*(xy - A @ c).T)
    return np.vstack([c, c[:k]]), np.array([0.0, np.sqrt(np.mean(r * r)), r.max(), ratio])


def residuals(t, k, ctrl, xy, u):
    """(rms, max) point-to-fit distance of the spline (t, ctrl, k) at the points' parameters, by scipy's own evaluation."""
    u = np.where(np.asarray(u) == 1.0, 0.0, u)
    fx = interpolate.BSpline(t, ctrl[:, 0], k)(u)
    fy = interpolate.BSpline(t, ctrl[:, 1], k)(u)
    r = np.hypot(xy[:, 0] - fx, xy[:, 1] - fy)
    return float(np.sqrt(np.mean(r * r))), float(r.max())


def fitpack(t, k, xy, u=None):
    """FITPACK's least-squares periodic spline on the given knots (clocur, task -1) through the closed loop of xy [P,2].
    Returns (ctrl [n,2], u [P]); raises what splprep raises on input it refuses."""
    loop = np.vstack([xy[:, :2], xy[:1, :2]])
    uu = None if u is None else np.concatenate([u, [1.0]])
    (tt, c, kk), uo = interpolate.splprep([loop[:, 0], loop[:, 1]], u=uu, t=np.asarray(t, dtype=np.float64), task=-1, per=True, k=k,
                                          quiet=1)
    assert kk == k and np.array_equal(tt, t), "FITPACK kept the knots it was given"
    return np.column_stack(c), np.asarray(uo)[:-1]


def tolerance(t, k, u, c_ref):
    """(bound, cond2(G)) of the rule above for one case."""
    cond = float(np.linalg.cond(normal_matrix(t, k, u)))
    return 4.0 * EPS * cond * float(np.abs(c_ref).max()), cond


def ring_points(u, rng):
    a = 2.0 * np.pi * u
    xy = np.column_stack([50.0 * np.cos(a) * (1.0 + 0.2 * np.cos(3.0 * a)), 30.0 * np.sin(a)])
    return xy + rng.normal(0.0, 0.05, xy.shape)


def ring_track_ctrl(t, k):
    """Control points of a smooth closed line on the knots: what a synthetic track is created with."""
    u = np.arange(200) / 200.0
    a = 2.0 * np.pi * u
    return fitpack(t, k, np.column_stack([50.0 * np.cos(a), 30.0 * np.sin(a)]), u)[0]


def ring_cases():
    """[(name, t, k, xy [P,2], u [P])]: uniform periodic knots, m = 2k+1 (the band just does not wrap onto itself), 2k+2 (the
    first clean corner block) and 16; P = 37, 65 with sorted random parameters (no multiple of the wave size), 40 uniform."""
    out = []
    for k, ms in ((3, (7, 8, 16)), (5, (11, 12, 16))):
        for m in ms:
            t = uniform_knots(k, m)
            for P in (37, 65, 40):
                # random parameters can leave a knot span nearly empty: the first draw (seeds in order) whose normal matrix
                # has cond2 <= COND_MAX is the case -- a property of the input alone
                for seed in range(1000 * k + 10 * m + P, 1000 * k + 10 * m + P + 1000, 100):
                    rng = np.random.default_rng(seed)
                    u = np.arange(P) / P if P == 40 else np.concatenate([[0.0], np.sort(rng.uniform(0.0, 1.0, P - 1))])
                    if np.linalg.cond(normal_matrix(t, k, u)) <= COND_MAX:
                        break
                out.append((f"ring_k{k}_m{m}_P{P}", t, k, ring_points(u, rng), u))
    return out


def monza_cases(fits):
    """[(name, tag, xy [P,2], u [P] | None)]: samples of the fixture fits plus N(0, 0.3 m) noise."""
    out = []
    for tag, Ps, chord in (("c100", (333, 500), True), ("c30", (333, 500), True), ("r10", (500,), False), ("l10", (600,), False)):   # (l10 at P = 500: cond2(G) = 4.7e5, above COND_MAX)
        t, cx, cy, k = fits[f"{tag}_t"], fits[f"{tag}_cx"], fits[f"{tag}_cy"], int(fits[f"{tag}_k"])
        for P in Ps:
            rng = np.random.default_rng(P + len(t))
            u = np.arange(P) / P
            xy = np.column_stack([interpolate.BSpline(t, cx, k)(u), interpolate.BSpline(t, cy, k)(u)]) + rng.normal(0.0, 0.3, (P, 2))
            out.append((f"{tag}_P{P}_uniform", tag, xy, u))
            if chord:
                out.append((f"{tag}_P{P}_chord", tag, xy, None))
    return out


def deficient_ring():
    """k = 5, m = 16, 60 points with parameters in [0, 0.45]: rank 13 of 16 (FITPACK refuses it)."""
    k, m = 5, 16
    rng = np.random.default_rng(77)
    u = np.concatenate([[0.0], np.sort(rng.uniform(0.0, 0.45, 59))])
    return uniform_knots(k, m), k, ring_points(u, rng), u


def deficient_monza(fits):
    """Monza k = 3 (83 intervals) with 333 uniform parameters: rank 82 of 83 (FITPACK refuses it)."""
    tag = "l10"
    t, cx, cy, k = fits[f"{tag}_t"], fits[f"{tag}_cx"], fits[f"{tag}_cy"], int(fits[f"{tag}_k"])
    u = np.arange(333) / 333.0
    xy = np.column_stack([interpolate.BSpline(t, cx, k)(u), interpolate.BSpline(t, cy, k)(u)])
    return tag, t, k, xy, u
