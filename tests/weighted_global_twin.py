"""CPU twin of the SPEED-WEIGHTED global min-curvature QP (include/rl_mincurv.h: rl_mincurv_global_weighted_batch_*).

A numpy restatement of the project's own twin of the unweighted problem, oracle/mincurv_oracle.c: orc_global_mincurv (which
cannot change), with the per-sample weight w_i on kappa_i^2, on P and on q:

    cost   sum_i w_i kappa_i(a)^2              P = sc 2 G'WG + 1e-9 I,  q = sc 2 G'W (kappa - G a),  sc = n_p / trace(2 G'WG)

Everything else is orc_global_mincurv's, statement for statement: the sample grid u_i = i (1/N), the Greville normals nu_j, the
constraint rows A and bounds, the Mehrotra predictor-corrector iteration with one common primal/dual step and the 0.995 step to
the boundary, the warm start of the slacks and duals from the previous linearisation (pushed back to >= 1e-2), 80 iterations at
most, and the exit rule ipm_done (mu < 1e-7 before the last linearisation, < 1e-10 on it).  What differs is the ORDER of the
sums: the oracle adds sample by sample, this file lets numpy / BLAS add (A'DA, G'WG as matrix products, dense Cholesky by
LAPACK).  The gap that leaves at w = 1 is measured by tests/test_weighted_global_cpu.py and recorded in DESIGN 6l.

The basis tables come from the oracle's de Boor evaluation (orc.bspline_eval on unit coefficient vectors: exactly the values
orc_global_mincurv tabulates)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import oracle as orc

IPM_TOL_ONE_OFFSET = 1e-7   # oracle/mincurv_oracle.c: kIpmTolOneOffset
IPM_TOL_LAST = 1e-10        # oracle/mincurv_oracle.c: kIpmTolLast


def ipm_done(tol_mid, last_qp, mu):
    return mu < (IPM_TOL_LAST if last_qp else tol_mid)


class Tables:
    """What orc_global_mincurv tabulates before its outer loop, for one (knots, centre line, N)."""

    def __init__(self, t, cx0, cy0, k, N):
        t = np.asarray(t, dtype=np.float64); cx0 = np.asarray(cx0, dtype=np.float64); cy0 = np.asarray(cy0, dtype=np.float64)
        self.t, self.cx0, self.cy0, self.k, self.N = t, cx0, cy0, int(k), int(N)
        n = len(t) - k - 1
        self.n, self.np = n, n - k
        K1 = k + 1
        u = np.arange(N, dtype=np.float64) * (1.0 / N)                       # grid_u
        ell = np.clip(np.searchsorted(t[:n], u, side="right") - 1, k, n - 1)  # find_interval
        self.ell = ell
        eye = np.eye(n)
        self.D = np.empty((3, N, K1))
        rows = np.arange(N)
        for m in range(3):
            full = np.stack([orc.bspline_eval(t, eye[j], k, u, m) for j in range(n)])   # [n, N]
            for a in range(K1):
                self.D[m, :, a] = full[ell - k + a, rows]
        J = ell[:, None] - k + np.arange(K1)[None, :]
        self.Jraw = J
        self.J = np.where(J >= self.np, J - self.np, J)                      # JH
        # control-point normals at the Greville sites
        g = np.zeros(self.np)
        for q in range(1, k + 1):
            g = g + t[q:q + self.np]
        g = g / float(k)
        g = g - np.floor(g)
        dx, dy = orc.bspline_eval(t, cx0, k, g, 1), orc.bspline_eval(t, cy0, k, g, 1)
        s = np.sqrt(dx * dx + dy * dy)
        self.nu = np.stack([-dy / s, dx / s], 1)
        # centre-line samples, normals, constraint rows
        x = np.zeros(N); y = np.zeros(N); dx = np.zeros(N); dy = np.zeros(N)
        for a in range(K1):
            x = x + cx0[J[:, a]] * self.D[0, :, a]; y = y + cy0[J[:, a]] * self.D[0, :, a]
            dx = dx + cx0[J[:, a]] * self.D[1, :, a]; dy = dy + cy0[J[:, a]] * self.D[1, :, a]
        s = np.sqrt(dx * dx + dy * dy)
        self.p0 = np.stack([x, y], 1)
        self.n0 = np.stack([-dy / s, dx / s], 1)
        self.A = self.D[0] * (self.n0[:, 0:1] * self.nu[self.J, 0] + self.n0[:, 1:2] * self.nu[self.J, 1])   # [N, K1]
        self.Afull = self.dense(self.A)

    def dense(self, rows):
        """[N, K1] row entries -> the dense [N, n_p] matrix (a row touches the k+1 control points of its span: no collisions)."""
        M = np.zeros((self.N, self.np))
        M[np.arange(self.N)[:, None], self.J] = rows
        return M

    def ctrl(self, av):
        jj = np.arange(self.n)
        jj = np.where(jj >= self.np, jj - self.np, jj)
        return self.cx0[jj] + av[jj] * self.nu[jj, 0], self.cy0[jj] + av[jj] * self.nu[jj, 1]

    def curvature_rows(self, cx, cy):
        K1, J, D = self.k + 1, self.Jraw, self.D
        dx = np.zeros(self.N); dy = np.zeros(self.N); ddx = np.zeros(self.N); ddy = np.zeros(self.N)
        for a in range(K1):
            dx = dx + cx[J[:, a]] * D[1, :, a]; dy = dy + cy[J[:, a]] * D[1, :, a]
            ddx = ddx + cx[J[:, a]] * D[2, :, a]; ddy = ddy + cy[J[:, a]] * D[2, :, a]
        s2 = dx * dx + dy * dy
        inv3 = 1.0 / (s2 * np.sqrt(s2))
        kp = (dx * ddy - dy * ddx) * inv3
        G = np.empty((self.N, K1))
        for a in range(K1):
            nx, ny, b1, b2 = self.nu[self.J[:, a], 0], self.nu[self.J[:, a], 1], D[1, :, a], D[2, :, a]
            G[:, a] = ((b1 * nx) * ddy + dx * (b2 * ny) - (b1 * ny) * ddx - dy * (b2 * nx)) * inv3 - \
                3.0 * kp * (dx * b1 * nx + dy * b1 * ny) / s2
        return kp, G

    def line(self, cx, cy):
        x = np.zeros(self.N); y = np.zeros(self.N)
        for a in range(self.k + 1):
            x = x + cx[self.Jraw[:, a]] * self.D[0, :, a]; y = y + cy[self.Jraw[:, a]] * self.D[0, :, a]
        return np.stack([x, y], 1)


def weighted_qp(tab, av, weights):
    """(P, q, kappa) of the linearisation at `av`: P = sc 2 G'WG + 1e-9 I, q = sc 2 G'W(kappa - G a)."""
    kp, G = tab.curvature_rows(*tab.ctrl(av))
    Gf = tab.dense(G)
    GW = Gf * weights[:, None]
    P = 2.0 * (GW.T @ Gf)
    q = 2.0 * (GW.T @ (kp - Gf @ av))
    sc = float(tab.np) / np.trace(P)
    return P * sc + 1e-9 * np.eye(tab.np), q * sc, kp


def global_mincurv_weighted(t, cx0, cy0, k, N, w_left, w_right, margin=0.0, n_outer=6, weights=None, tables=None,
                            last_as_mid=False):
    """orc_global_mincurv with the cost sum_i weights[i] kappa_i^2 (None = ones).  Returns (cx [n], cy [n], xy [N,2], a [n-k],
    stats [8]) as oracle.global_mincurv does; stats[1], [2] are the weighted sums.  last_as_mid: the twin of the library's test
    hook "global_last_as_mid" -- the last linearisation leaves at the intermediate tolerance."""
    tab = tables or Tables(t, cx0, cy0, k, N)
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (N,)
    A = tab.Afull
    lo, hi = -(np.asarray(w_right, dtype=np.float64) - margin), np.asarray(w_left, dtype=np.float64) - margin
    av = np.zeros(tab.np)
    sl = su = ll = lu = None
    k2_first = k2_last = last_step = 0.0
    total_it = 0
    for outer in range(n_outer + 1):
        kp, _ = tab.curvature_rows(*tab.ctrl(av))
        k2 = float(np.sum(w * kp * kp))
        if outer == 0:
            k2_first = k2
        k2_last = k2
        if outer == n_outer:
            break
        P, qv, _ = weighted_qp(tab, av, w)
        xv = av.copy()
        ax = A @ xv
        if outer == 0:
            sl, su = np.maximum(ax - lo, 1e-2), np.maximum(hi - ax, 1e-2)
            ll, lu = np.ones(N), np.ones(N)
        else:   # warm start: the previous QP's slacks and duals, pushed back inside
            sl, su, ll, lu = np.maximum(sl, 1e-2), np.maximum(su, 1e-2), np.maximum(ll, 1e-2), np.maximum(lu, 1e-2)
        for _it in range(80):
            ax = A @ xv
            rpl, rpu = ax - lo - sl, hi - ax - su
            rd = P @ xv + qv + A.T @ (lu - ll)
            mu = float(np.sum(sl * ll + su * lu)) / float(2 * N)
            if ipm_done(IPM_TOL_ONE_OFFSET, outer + 1 >= n_outer and not last_as_mid, mu):
                break
            total_it += 1
            dm = ll / sl + lu / su
            Kf = cho_factor(P + A.T @ (dm[:, None] * A), lower=True)
            sigma = 0.0
            dsl = dsu = dll = dlu = None
            for ps in range(2):
                rcl, rcu = sl * ll, su * lu
                if ps == 1:
                    rcl = rcl + (-sigma * mu + dsl * dll); rcu = rcu + (-sigma * mu + dsu * dlu)
                wv = (-rcl - ll * rpl) / sl - (-rcu - lu * rpu) / su
                dxv = cho_solve(Kf, -rd + A.T @ wv)
                adx = A @ dxv
                d_sl, d_su = adx + rpl, -adx + rpu
                d_ll, d_lu = (-rcl - ll * d_sl) / sl, (-rcu - lu * d_su) / su
                alpha = 1.0
                for s_, d_ in ((sl, d_sl), (su, d_su), (ll, d_ll), (lu, d_lu)):   # step to the boundary
                    neg = d_ < 0.0
                    if neg.any():
                        alpha = min(alpha, float(np.min(0.995 * (-s_[neg] / d_[neg]))))
                dsl, dsu, dll, dlu = d_sl, d_su, d_ll, d_lu
                if ps == 0:
                    mu_aff = float(np.sum((sl + alpha * dsl) * (ll + alpha * dll) + (su + alpha * dsu) * (lu + alpha * dlu)))
                    mu_aff /= float(2 * N)
                    r = mu_aff / mu
                    sigma = r * r * r
            xv = xv + alpha * dxv
            sl, su, ll, lu = sl + alpha * dsl, su + alpha * dsu, ll + alpha * dll, lu + alpha * dlu
        last_step = float(np.max(np.abs(xv - av)))
        av = xv
    cx, cy = tab.ctrl(av)
    xy = tab.line(cx, cy)
    lat = ((xy - tab.p0) * tab.n0).sum(1)
    viol = max(0.0, float(np.max(np.maximum(lo - lat, lat - hi))))
    n_active = int(np.sum((lat - lo < 1e-6) | (hi - lat < 1e-6)))
    stats = np.array([total_it, k2_first, k2_last, viol, last_step, n_active, 0.0, 0.0])
    return cx, cy, xy, av, stats
