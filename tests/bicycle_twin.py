"""CPU twin of the bicycle min-time NLP solve (include/rl_mincurv.h: rl_bicycle_*), for tests only.

Its own numpy code, independent of the kernels: the NLP's functions (the reference's set_up_bicycle_problem,
min_time_optm/min_time_optimizer.py:14-90, on the host mirrors' model), exact first and second derivatives by a
small second-order forward-mode jet, and the same primal-dual interior-point iteration as csrc/rl_bicycle.hpp:
slacks for the two general inequalities condensed into the node's 8 x 8 block, the cyclic block-tridiagonal
KKT system (8 unknowns + 6 multipliers per node) eliminated node by node with the border of the wrap-around
carried along, inertia from the pivots of each pivot block's LDL^T without pivoting, fraction to the boundary, filter line search.

Unknowns per node j (scaled like the reference): w = (X[5], U[2], T); x = X * SX + (P0, 0, 0, 0), u = U * SU.
"""
import numpy as np

SX = np.array([10.0, 10.0, 3.14, 0.1, 80.0])
SU = np.array([20.0, 1.0])
KEYS = ("lr", "L", "delta_max", "v_max", "a_lon_max", "a_lon_min", "delta_dot_max", "acc_max")
NV, NE, NB = 8, 6, 10          # unknowns, equalities per node; bounded scalars per node (8 unknowns + 2 slacks)
CURVED = (2, 3, 4, 5, 6, 7)    # theta, delta, v, a, delta_dot, T: the unknowns with curvature


class Jet:
    """Value, gradient [K, ...] and Hessian [K, K, ...] of a function of K seeded unknowns (vectorised)."""

    def __init__(self, v, g, h):
        self.v, self.g, self.h = v, g, h

    @staticmethod
    def seed(vals, k, K):
        vals = np.asarray(vals, dtype=np.float64)
        g = np.zeros((K,) + vals.shape); g[k] = 1.0
        return Jet(vals, g, np.zeros((K, K) + vals.shape))

    def _u(self, f, d1, d2):
        return Jet(f, d1 * self.g, d1 * self.h + d2 * self.g[:, None] * self.g[None, :])

    def __add__(self, o):
        return Jet(self.v + o.v, self.g + o.g, self.h + o.h) if isinstance(o, Jet) else Jet(self.v + o, self.g, self.h)
    __radd__ = __add__

    def __neg__(self):
        return Jet(-self.v, -self.g, -self.h)

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Jet):
            return Jet(self.v * o, self.g * o, self.h * o)
        return Jet(self.v * o.v, self.g * o.v + self.v * o.g,
                   self.h * o.v + self.v * o.h + self.g[:, None] * o.g[None, :] + o.g[:, None] * self.g[None, :])
    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, Jet):
            return self * (1.0 / o)
        r = 1.0 / o.v
        return self * o._u(r, -r * r, 2.0 * r * r * r)


def jsin(a):
    return a._u(np.sin(a.v), np.cos(a.v), -np.sin(a.v)) if isinstance(a, Jet) else np.sin(a)


def jcos(a):
    return a._u(np.cos(a.v), -np.sin(a.v), -np.cos(a.v)) if isinstance(a, Jet) else np.cos(a)


def jtan(a):
    if not isinstance(a, Jet):
        return np.tan(a)
    t = np.tan(a.v); s2 = 1.0 + t * t
    return a._u(t, s2, 2.0 * t * s2)


def jatan(a):
    if not isinstance(a, Jet):
        return np.arctan(a)
    q = 1.0 / (1.0 + a.v * a.v)
    return a._u(np.arctan(a.v), q, -2.0 * a.v * q * q)


def model_vec(model):
    return np.array([float(model[k]) for k in KEYS])


def _dyn(m, th, de, v, a, dd):
    lr, L = m[0], m[1]
    beta = jatan(de * (lr / L))          # atan2(lr delta, L) with L > 0
    cb = jcos(beta)
    om = v * cb * jtan(de) / L
    return [v * jcos(th + beta), v * jsin(th + beta), om, dd, a]


def _rk4_curved(m, x, u, dt):
    """x: [theta, delta, v] (+ x, y handled linearly); returns the RK4 increments of all 5 states."""
    th, de, v = x
    a, dd = u
    k1 = _dyn(m, th, de, v, a, dd)
    k2 = _dyn(m, th + dt * 0.5 * k1[2], de + dt * 0.5 * k1[3], v + dt * 0.5 * k1[4], a, dd)
    k3 = _dyn(m, th + dt * 0.5 * k2[2], de + dt * 0.5 * k2[3], v + dt * 0.5 * k2[4], a, dd)
    k4 = _dyn(m, th + dt * k3[2], de + dt * k3[3], v + dt * k3[4], a, dd)
    return [dt * (1.0 / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(5)]


class Problem:
    """One instance: model dict, P0 [N,2], yaw [N], dl [N] (> 0), dr [N] (< 0)."""

    def __init__(self, model, P0, yaw, dl, dr):
        self.m = model_vec(model)
        self.P0 = np.asarray(P0, dtype=np.float64); self.yaw = np.asarray(yaw, dtype=np.float64)
        self.N = len(self.yaw)
        self.cy, self.sy = np.cos(self.yaw), np.sin(self.yaw)
        m = self.m
        inf = np.inf
        lo = np.array([-inf, -inf, -inf, -m[2] / SX[3], 0.0, m[5] / SU[0], -m[6] / SU[1], 0.0, 0.0, -inf])
        hi = np.array([inf, inf, inf, m[2] / SX[3], m[3] / SX[4], m[4] / SU[0], m[6] / SU[1], inf, 0.0, m[7] * m[7]])
        self.lo = np.tile(lo, (self.N, 1)); self.hi = np.tile(hi, (self.N, 1))
        self.lo[:, 8] = np.asarray(dr, dtype=np.float64); self.hi[:, 8] = np.asarray(dl, dtype=np.float64)

    # ---- scaling
    def to_w(self, X, U, T):
        w = np.zeros((self.N, NV))
        w[:, 0:2] = (X[:, 0:2] - self.P0) / SX[0:2]
        w[:, 2:5] = X[:, 2:5] / SX[2:5]
        w[:, 5:7] = U / SU; w[:, 7] = T
        return w

    def from_w(self, w):
        X = w[:, 0:5] * SX; X[:, 0:2] += self.P0
        return X, w[:, 5:7] * SU, w[:, 7].copy()

    # ---- functions
    def funcs(self, w, jets=False, yc=None, yd=None):
        """c [N,6], d [N,2]; with jets also Jc [N,6,8], Jd [N,2,8] and the Hessian of
        sum_j yc_j . c_j + yd_j . d_j with respect to w_j [N,8,8]."""
        N = self.N
        wn = np.roll(w, -1, axis=0)
        if jets:
            v = [Jet.seed(w[:, k], i, 6) for i, k in enumerate(CURVED)]
        else:
            v = [w[:, k] for k in CURVED]
        th, de, vv = v[0] * SX[2], v[1] * SX[3], v[2] * SX[4]
        a, dd, dt = v[3] * SU[0], v[4] * SU[1], v[5]
        inc = _rk4_curved(self.m, (th, de, vv), (a, dd), dt)
        px, py = w[:, 0] * SX[0], w[:, 1] * SX[1]
        x1 = [px + self.P0[:, 0], py + self.P0[:, 1], w[:, 2] * SX[2], w[:, 3] * SX[3], w[:, 4] * SX[4]]
        x2 = [wn[:, k] * SX[k] for k in range(5)]
        x2[0] = x2[0] + np.roll(self.P0[:, 0], -1); x2[1] = x2[1] + np.roll(self.P0[:, 1], -1)
        dth = x2[2] - x1[2]
        x2[2] = np.arctan2(np.sin(dth), np.cos(dth)) + x1[2]
        val = lambda q: q.v if isinstance(q, Jet) else q  # noqa: E731
        c = np.zeros((N, NE)); d = np.zeros((N, 2))
        for i in range(5):
            c[:, i] = x1[i] + val(inc[i]) - x2[i]
        c[:, 5] = self.cy * px + self.sy * py
        d[:, 0] = -self.sy * px + self.cy * py
        om = _dyn(self.m, th, de, vv, a, dd)
        q = om[2] * om[2] * (om[0] * om[0] + om[1] * om[1]) + a * a
        d[:, 1] = val(q)
        if not jets:
            return c, d
        Jc = np.zeros((N, NE, NV)); Jd = np.zeros((N, 2, NV))
        for i in range(5):
            Jc[:, i, i] = SX[i]
            for t, k in enumerate(CURVED):
                Jc[:, i, k] += inc[i].g[t]
        Jc[:, 5, 0] = self.cy * SX[0]; Jc[:, 5, 1] = self.sy * SX[1]
        Jd[:, 0, 0] = -self.sy * SX[0]; Jd[:, 0, 1] = self.cy * SX[1]
        for t, k in enumerate(CURVED):
            Jd[:, 1, k] = q.g[t]
        H = np.zeros((N, NV, NV))
        if yc is not None:
            h6 = sum(yc[:, i] * inc[i].h for i in range(5)) + yd[:, 1] * q.h    # [6,6,N]
            idx = np.array(CURVED)
            H[:, idx[:, None], idx[None, :]] = np.moveaxis(h6, -1, 0)
        return c, d, Jc, Jd, H

    @staticmethod
    def coupling_t(yc):
        """C_{j-1}^T yc_{j-1} on node j: the defect of pair j-1 holds -x_{j+1} * SX linearly."""
        g = np.zeros((len(yc), NV))
        g[:, 0:5] = -np.roll(yc[:, 0:5], 1, axis=0) * SX
        return g


def initial_guess(kind, P0, yaw, speed=None, v_default=10.0):
    """(X, U, T) physical. 'reference': min_time_optimizer.py:80-83 as written (the affine set_initial puts every
    node at the global origin); 'centerline': on P0 with theta = yaw, speed from the table (else v_default) and
    T = segment length / speed."""
    N = len(yaw)
    X = np.zeros((N, 5)); U = np.zeros((N, 2))
    if kind == "reference":
        X[:, 2] = yaw; X[:, 4] = 1.0
        return X, U, np.ones(N)
    v = np.full(N, v_default) if speed is None else np.where(np.asarray(speed) > 0, speed, v_default)
    X[:, 0:2] = P0; X[:, 2] = np.unwrap(yaw); X[:, 4] = v
    seg = np.linalg.norm(np.roll(P0, -1, axis=0) - P0, axis=1)
    return X, U, seg / v


# ---- the interior-point iteration
MU0, KAPPA_EPS, KAPPA_MU, THETA_MU = 0.1, 10.0, 0.2, 1.5
TAU_MIN, DELTA_C, KAPPA_SIGMA = 0.99, 1e-10, 1e10
GAMMA_TH, GAMMA_PHI, ETA, S_TH, S_PHI, MAX_HALVINGS = 1e-5, 1e-8, 1e-4, 1.1, 2.3, 20
DW0, DW_FIRST_UP, DW_UP, DW_DOWN, DW_MAX = 1e-4, 100.0, 8.0, 1.0 / 3.0, 1e40
PIV_REL = 1e-10


def _push(p, lo, hi):
    """Move p strictly inside its bounds (IPOPT's bound_push / bound_frac, 1e-2)."""
    fl, fh = np.isfinite(lo), np.isfinite(hi)
    wl = np.where(fl, 1e-2 * np.maximum(1.0, np.abs(lo)), 0.0)
    wh = np.where(fh, 1e-2 * np.maximum(1.0, np.abs(hi)), 0.0)
    both = fl & fh
    wl = np.where(both, np.minimum(wl, 1e-2 * (hi - lo)), wl)
    wh = np.where(both, np.minimum(wh, 1e-2 * (hi - lo)), wh)
    p = np.where(fl, np.maximum(p, lo + wl), p)
    return np.where(fh, np.minimum(p, hi - wh), p)


def ldl_pivots(M):
    """Pivots of the LDL^T factorisation of a symmetric block WITHOUT pivoting (unknowns first, then multipliers),
    or None when one is not finite or zero up to cancellation (|pivot| <= PIV_REL |its diagonal entry before the
    elimination|: e.g. y after x when only the rank-1 lateral row acts on them).  Their signs are the block's inertia; a zero pivot counts as a wrong
    inertia, so a block whose unknowns' part is singular (e.g. the heading's diagonal before the multipliers of the
    defect are nonzero) is regularised, as on the GPU."""
    A = np.array(M, dtype=np.float64)
    diag0 = np.abs(np.diag(A)).copy()
    piv = np.empty(len(A))
    for p in range(len(A)):
        d = A[p, p]
        if not (np.isfinite(d) and abs(d) > PIV_REL * diag0[p]):
            return None
        piv[p] = d
        A[p + 1:, p + 1:] -= np.outer(A[p + 1:, p], A[p, p + 1:]) / d
    return piv


def block_solve_factor(D, delta_w):
    """Cyclic block elimination of the KKT matrix: D [N,14,14] node blocks (without delta_w), couplings fixed by
    SX.  Returns (negative eigenvalue count, Dinv [N,14,14], Tk [N,14,14])."""
    N = len(D)
    Dk = D.copy()
    Dk[:, np.arange(NV), np.arange(NV)] += delta_w
    Dk[:, np.arange(NV, 14), np.arange(NV, 14)] -= DELTA_C
    Dinv = np.zeros_like(D); Tk = np.zeros_like(D)
    last = Dk[N - 1].copy()
    Bt = np.zeros((14, 14))
    for c in range(5):
        Bt[NV + c, c] = -SX[c]                # K[N-1, 0] = E_{N-1}^T
    neg = 0
    cur = Dk[0].copy()
    for k in range(N - 1):
        piv = ldl_pivots(cur)
        if piv is None:
            return -1, None, None
        neg += int(np.sum(piv < 0))
        inv = np.linalg.inv(cur)
        Dinv[k] = inv
        T = Bt @ inv
        Tk[k] = T
        last -= T @ Bt.T
        if k + 1 < N - 1:
            nxt = Dk[k + 1].copy()
            nxt[:5, :5] -= np.outer(SX, SX) * inv[NV:NV + 5, NV:NV + 5]
            cur = nxt
            Bn = np.zeros((14, 14))
            Bn[:, 0:5] = T[:, NV:NV + 5] * SX
            if k + 1 == N - 2:
                for c in range(5):
                    Bn[c, NV + c] += -SX[c]   # K[N-1, N-2] = E_{N-2}
            Bt = Bn
    piv = ldl_pivots(last)
    if piv is None:
        return -1, None, None
    neg += int(np.sum(piv < 0))
    Dinv[N - 1] = np.linalg.inv(last)
    return neg, Dinv, Tk


def block_solve(Dinv, Tk, r):
    N = len(r)
    rt = r.copy()
    v = np.zeros_like(r)
    for k in range(N - 1):
        v[k] = Dinv[k] @ rt[k]
        if k + 1 < N - 1:
            rt[k + 1, 0:5] += SX * v[k, NV:NV + 5]
        rt[N - 1] -= Tk[k] @ rt[k]
    z = np.zeros_like(r)
    z[N - 1] = Dinv[N - 1] @ rt[N - 1]
    for k in range(N - 2, -1, -1):
        zk = v[k] - Tk[k].T @ z[N - 1]
        if k + 1 < N - 1:
            zk = zk + Dinv[k][:, NV:NV + 5] @ (SX * z[k + 1, 0:5])
        z[k] = zk
    return z


def solve(prob, X0, U0, T0, max_iter=200, tol=1e-6):
    """-> X [N,5], U [N,2], T [N], stats [12] (include/rl_mincurv.h: rl_bicycle_solve_batch)."""
    P = prob
    N = P.N
    lo, hi = P.lo, P.hi
    fl, fh = np.isfinite(lo), np.isfinite(hi)
    lo0, hi0 = np.where(fl, lo, 0.0), np.where(fh, hi, 0.0)
    p = np.zeros((N, NB))
    p[:, :NV] = P.to_w(np.asarray(X0, float), np.asarray(U0, float), np.asarray(T0, float))
    p[:, :NV] = _push(p[:, :NV], lo[:, :NV], hi[:, :NV])
    c, d = P.funcs(p[:, :NV])
    p[:, NV:] = _push(d, lo[:, NV:], hi[:, NV:])
    yc = np.zeros((N, NE)); yd = np.zeros((N, 2))
    zl = np.where(fl, 1.0, 0.0); zu = np.where(fh, 1.0, 0.0)
    mu = MU0
    filt = []
    dw_last = 0.0
    theta_max = theta_min = None
    stats = np.zeros(12)
    status = 0
    it = 0
    refac = 0
    alpha = 0.0
    amax = 0.0
    halv = 0

    def gaps(pp):
        return np.where(fl, pp - lo0, 1.0), np.where(fh, hi0 - pp, 1.0)

    def theta_phi(pp):
        cc, dd = P.funcs(pp[:, :NV])
        gl, gu = gaps(pp)
        th = np.abs(cc).sum() + np.abs(dd - pp[:, NV:]).sum()
        ph = pp[:, 7].sum() - mu * (np.where(fl, np.log(gl), 0.0).sum() + np.where(fh, np.log(gu), 0.0).sum())
        return th, ph

    def errors(c, d, Jc, Jd, pp, mu_):
        gl, gu = gaps(pp)
        gw = np.zeros((N, NV)); gw[:, 7] = 1.0
        gw += np.einsum("nij,ni->nj", Jc, yc) + P.coupling_t(yc) + np.einsum("nij,ni->nj", Jd, yd)
        gw -= zl[:, :NV]; gw += zu[:, :NV]
        gs = -yd - zl[:, NV:] + zu[:, NV:]
        dual = max(np.abs(gw).max(), np.abs(gs).max())
        prim = max(np.abs(c).max(), np.abs(d - pp[:, NV:]).max())
        comp = max(np.abs(np.where(fl, gl * zl - mu_, 0.0)).max(), np.abs(np.where(fh, gu * zu - mu_, 0.0)).max())
        return dual, prim, comp

    for it in range(max_iter + 1):
        c, d, Jc, Jd, H = P.funcs(p[:, :NV], True, yc, yd)
        e0 = errors(c, d, Jc, Jd, p, 0.0)
        if max(e0) <= tol:
            status = 1
            break
        if it == max_iter:
            break
        while mu > tol / 10.0 and max(errors(c, d, Jc, Jd, p, mu)) <= KAPPA_EPS * mu:
            mu = max(tol / 10.0, min(KAPPA_MU * mu, mu ** THETA_MU))
            filt = []
        gl, gu = gaps(p)
        sig = np.where(fl, zl / gl, 0.0) + np.where(fh, zu / gu, 0.0)
        bar = np.where(fl, -mu / gl, 0.0) + np.where(fh, mu / gu, 0.0)
        sw, ss = sig[:, :NV], sig[:, NV:]
        rs = ss * (d - p[:, NV:]) + bar[:, NV:]
        Hc = H + sw[:, :, None] * np.eye(NV)[None] + np.einsum("nki,nk,nkj->nij", Jd, ss, Jd)
        D = np.zeros((N, 14, 14))
        D[:, :NV, :NV] = Hc; D[:, NV:, :NV] = Jc; D[:, :NV, NV:] = np.transpose(Jc, (0, 2, 1))
        r = np.zeros((N, 14))
        gw = np.zeros((N, NV)); gw[:, 7] = 1.0
        r[:, :NV] = -(gw + np.einsum("nij,ni->nj", Jc, yc) + P.coupling_t(yc) + bar[:, :NV] + np.einsum("nki,nk->ni", Jd, rs))
        r[:, NV:] = -c
        # inertia correction
        dw = 0.0
        tries = 0
        while True:
            neg, Dinv, Tk = block_solve_factor(D, dw)
            tries += 1
            if neg == NE * N:
                break
            if dw == 0.0:
                dw = DW0 if dw_last == 0.0 else max(1e-20, DW_DOWN * dw_last)
            else:
                dw *= DW_FIRST_UP if dw_last == 0.0 else DW_UP
            if dw > DW_MAX:
                status = 2
                break
        if status == 2:
            break
        refac += tries - 1
        if dw > 0.0:
            dw_last = dw
        sol = block_solve(Dinv, Tk, r)
        dwv, dyc = sol[:, :NV], sol[:, NV:]
        ds = np.einsum("nij,nj->ni", Jd, dwv) + (d - p[:, NV:])
        dyd = ss * ds - yd + bar[:, NV:]
        dp = np.concatenate([dwv, ds], axis=1)
        dzl = np.where(fl, mu / gl - zl - zl / gl * dp, 0.0)
        dzu = np.where(fh, mu / gu - zu + zu / gu * dp, 0.0)
        tau = max(TAU_MIN, 1.0 - mu)
        with np.errstate(divide="ignore", invalid="ignore"):
            am = min(1.0, np.min(np.where(fl & (dp < 0), -tau * gl / dp, np.inf)),
                     np.min(np.where(fh & (dp > 0), tau * gu / dp, np.inf)))
            az = min(1.0, np.min(np.where(fl & (dzl < 0), -tau * zl / dzl, np.inf)),
                     np.min(np.where(fh & (dzu < 0), -tau * zu / dzu, np.inf)))
        amax = am
        th0, ph0 = theta_phi(p)
        if theta_max is None:
            theta_max = 1e4 * max(1.0, th0); theta_min = 1e-4 * max(1.0, th0)
        gphi = dwv[:, 7].sum() + np.sum(bar * dp)
        a = am
        accepted = False
        for halv in range(MAX_HALVINGS):
            pt = p + a * dp
            tht, pht = theta_phi(pt)
            ok = tht <= theta_max and not any(tht >= f0 and pht >= f1 for f0, f1 in filt)
            ftype = False
            if ok:
                if gphi < 0 and a * (-gphi) ** S_PHI > th0 ** S_TH and th0 <= theta_min:
                    ftype = True
                    ok = pht <= ph0 + ETA * a * gphi
                else:
                    ok = tht <= (1 - GAMMA_TH) * th0 or pht <= ph0 - GAMMA_PHI * th0
            if ok:
                accepted = True
                break
            if halv < MAX_HALVINGS - 1:
                a *= 0.5
        if not ftype or not accepted:
            filt.append(((1 - GAMMA_TH) * th0, ph0 - GAMMA_PHI * th0))
        alpha = a
        p = p + a * dp
        yc = yc + a * dyc; yd = yd + a * dyd
        zl = zl + az * dzl; zu = zu + az * dzu
        gl, gu = gaps(p)
        zl = np.where(fl, np.clip(zl, mu / (KAPPA_SIGMA * gl), KAPPA_SIGMA * mu / gl), 0.0)
        zu = np.where(fh, np.clip(zu, mu / (KAPPA_SIGMA * gu), KAPPA_SIGMA * mu / gu), 0.0)
    c, d = P.funcs(p[:, :NV])
    c, d, Jc, Jd, _ = P.funcs(p[:, :NV], True, yc, yd)
    e0 = errors(c, d, Jc, Jd, p, 0.0)
    X, U, T = P.from_w(p[:, :NV])
    stats[:] = [it, e0[0], e0[1], e0[2], T.sum(), status, mu, dw_last, alpha, refac, amax, halv]
    return X, U, T, stats
