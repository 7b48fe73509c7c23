"""CPU twin of the speed-weighted min-curvature sweep: run_min_curvature_qp with line 71 of the reference's optimizer.py
active (`v = 1/traj_d[t_mask, SPEED]` instead of `v = np.ones(M)`), for any positive per-sample weight.

Only the cost loop is written here, in plain Python floats (IEEE doubles, one rounding per operation, no contraction), in
numpy's order of optimizer.py:73-76 with v active:

    nxx = (dTy*dTy)*w      nxy = ((-2.0*dTx)*dTy)*w      nyy = (dTx*dTx)*w      each / denom

and the six sums run sequentially in sample order, H = 2 (...), g as the oracle's orc_min_curvature_cost forms it.  Everything
else is the oracle's own exported pieces (bspline_derivative, bspline_eval, basis_element, track_constraint,
qp_solve_separable, sample_along, fill_bounds) in the order of the oracle's sweep loop (orc_run_min_curvature_qp /
optimize_one).  Call it inside oracle.cr_variant(): the build the reference-order kernels reproduce bit for bit.

numpy's raise mode is NOT modelled: after every refresh the twin asserts that every turn radius of the table is finite and
positive, i.e. that no step could have raised -- then raise mode cannot matter, and a kernel in either state must agree.
"""
import numpy as np

from oracle import oracle as orc


def grid(N):
    return np.linspace(0.0, 1.0, N, endpoint=False)


def support(t, k, idx, N):
    """Indices of the samples u_i = i / N inside the support of basis function idx (optimizer.py:27-29)."""
    u = grid(N)
    return np.nonzero((u >= t[idx]) & (u < t[idx + k + 1]))[0]


def cost(z, idx, t, cx, cy, k, N, w):
    """min_curvature_cost (optimizer.py:24-86) with the weight w[i] of sample i as `v`.  Returns H [2,2], g [2], M."""
    ii = support(t, k, idx, N)
    ti = grid(N)[ii]
    t1, c1, k1 = orc.bspline_derivative(t, cx, k, 1); dTx = orc.bspline_eval(t1, c1[:len(t1) - k1 - 1], k1, ti)
    t1, c1, k1 = orc.bspline_derivative(t, cy, k, 1); dTy = orc.bspline_eval(t1, c1[:len(t1) - k1 - 1], k1, ti)
    t2, c2, k2 = orc.bspline_derivative(t, cx, k, 2); d2Tx = orc.bspline_eval(t2, c2[:len(t2) - k2 - 1], k2, ti)
    t2, c2, k2 = orc.bspline_derivative(t, cy, k, 2); d2Ty = orc.bspline_eval(t2, c2[:len(t2) - k2 - 1], k2, ti)
    B = orc.basis_element(t[idx:idx + k + 2], ti, 2)
    zx, zy = float(z[0]), float(z[1])
    hxx = hyy = fx_pxx_b = fy_pxy_b = fy_pyy_b = b_pxy_fx = 0.0
    for i in range(len(ii)):
        v = float(w[ii[i]])
        b = float(B[i])
        x, y = float(dTx[i]), float(dTy[i])
        Fx = float(d2Tx[i]) - b * zx
        Fy = float(d2Ty[i]) - b * zy
        s2 = x * x + y * y
        denom = s2 * s2 * s2
        Pxx = ((y * y) * v) / denom
        Pxy = (((-2.0 * x) * y) * v) / denom
        Pyy = ((x * x) * v) / denom
        hxx += b * Pxx * b
        hyy += b * Pyy * b
        fx_pxx_b += Fx * Pxx * b
        fy_pxy_b += Fy * Pxy * b
        fy_pyy_b += Fy * Pyy * b
        b_pxy_fx += b * Pxy * Fx
    H = np.array([[2.0 * hxx, 0.0], [0.0, 2.0 * hyy]])
    g = np.array([fx_pxx_b + fx_pxx_b, (fy_pxy_b + fy_pyy_b) + (b_pxy_fx + fy_pyy_b)])
    return H, g, len(ii)


def _table(t, cx, cy, k, length, N, ringL, ringR):
    pts = orc.sample_along(t, cx, cy, k, length, grid(N))
    orc.fill_bounds(pts, ringL, ringR, 100.0)
    radius = pts[:, 5]
    assert np.all(np.isfinite(radius)) and np.all(radius > 0.0), "a sample degenerated: numpy's raise mode would matter"
    return pts


def sweep(t, cx, cy, k, length, N, ringL, ringR, i_start, w):
    """run_min_curvature_qp (optimizer.py:256-341; oracle: orc_run_min_curvature_qp) on the shared rings with the weighted
    cost.  Returns (cx, cy, points [N,19], n_success [max_iter,2])."""
    cx = np.array(cx, dtype=np.float64, copy=True); cy = np.array(cy, dtype=np.float64, copy=True)
    w = np.asarray(w, dtype=np.float64)
    assert w.shape == (N,) and np.all(np.isfinite(w)) and np.all(w > 0.0)
    n = len(cx)
    i_min, i_max = k // 2, n - (k - k // 2)
    pts = _table(t, cx, cy, k, length, N, ringL, ringR)
    ns = []
    for st in i_start:
        for order in (range(0, i_max - i_min), range(i_max - i_min, 0, -1)):
            ok = 0
            for i in order:
                kk = i + int(st)
                if kk >= i_max:
                    kk = kk - i_max + i_min
                H, g, _ = cost((cx[kk], cy[kk]), kk, t, cx, cy, k, N, w)
                A, lba, uba = orc.track_constraint(kk, t, cx, cy, k, pts)
                status, x = orc.qp_solve_separable(H, g, A, lba, uba)
                if status != 0:
                    continue
                cx[kk] = x[0]; cy[kk] = x[1]
                for dst, src in ((0, n - 5), (1, n - 4), (n - 3, 2), (n - 2, 3), (n - 1, 4)):
                    cx[dst] = cx[src]; cy[dst] = cy[src]
                pts = _table(t, cx, cy, k, length, N, ringL, ringR)
                ok += 1
            ns.append(ok)
    return cx, cy, pts, np.array(ns, dtype=np.int32).reshape(len(i_start), 2)


# ---- the cases the tests share: computed once per key, inside cr_variant()
def case_weights(N):
    """The four weightings of the twin tests at N samples: two random exp2(U(-3,3)), 1 / linspace(20, 80), ones."""
    return np.stack([np.exp2(np.random.default_rng(5).uniform(-3.0, 3.0, N)),
                     np.exp2(np.random.default_rng(6).uniform(-3.0, 3.0, N)),
                     1.0 / np.linspace(20.0, 80.0, N),
                     np.ones(N)])


_runs = {}


def sweep_cached(key, *args):
    if key not in _runs:
        with orc.cr_variant():
            orc.lib()
            _runs[key] = sweep(*args)
    return _runs[key]
