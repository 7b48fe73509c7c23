"""The node functions of the two min-time NLPs written once over a small math namespace -- TEST INFRASTRUCTURE ONLY.

A scalar-by-scalar restatement of oracle/dt_checker.py (double-track: dynamics, yaw / abscissa alignment, Hermite-Simpson
defect, load-transfer residual, the 14 inequality rows, the pair's cost terms) and of tests/bicycle_twin.py (_dyn,
_rk4_curved, Frenet rows, traction row, with the division and multiplication by SX / SU that rl_bicycle_eval_nodes performs
on its physical inputs).  Three instantiations:

  * MpMath      mpmath at 50 digits: the reference.  First derivatives by central differences at 50 digits, step
                1e-18 max(1, |variable|) (truncation ~1e-36): no chain-rule code at all;
  * FloatMath   Python float with `math`: the double twin (what honest double arithmetic gives);
  * DualMath    a forward-mode dual over float, 21 directions: the double twin of the Jacobian.

Every literal (0.5, 1e-4, 9.8, the model's numbers) is the same double in all three: the reference evaluates the function the
code states, in more digits.  `M.note(key, value)` marks what the tests' input conditions are stated on (arguments of the
device's m_atan / m_sincos call sites, denominators, kink distances); only the recording FloatMath keeps them.

tests/golden/make_golden_nlp_highprec.py draws the input families below and stores inputs, reference, twins and notes in
tests/golden/G16_nlp_highprec.npz; tests/test_nlp_highprec_{cpu,gpu}.py read it."""
import math

import numpy as np

G = 9.8
NVAR = 21            # x (6) | u (4) | t | x_next (6) | u_next (4)
DPS = 50
SX = (10.0, 10.0, 3.14, 0.1, 80.0)
SU = (20.0, 1.0)
BK_KEYS = ("lr", "L", "delta_max", "v_max", "a_lon_max", "a_lon_min", "delta_dot_max", "acc_max")
ATAN_BREAKS = (0.4375, 0.6875, 1.1875, 2.4375)
# the kink conditions of the input families: names, and the least admissible value of each
KINKS = ("yaw", "rate_force", "rate_steer", "ds", "fmod", "denominator", "one_minus_n_kappa", "speed")
KINK_MIN = (1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 0.5, 0.5, 0.5)


# ---------------------------------------------------------------------------------------------------- namespaces
class FloatMath:
    sin, cos, tan, atan, atan2, tanh, fabs, fmod = (staticmethod(f) for f in (
        math.sin, math.cos, math.tan, math.atan, math.atan2, math.tanh, math.fabs, math.fmod))

    def __init__(self, record=False):
        self.notes = {} if record else None

    @staticmethod
    def sign(x):
        return 1.0 if x > 0.0 else (-1.0 if x < 0.0 else 0.0)

    @staticmethod
    def max(a, b):
        return a if a >= b else b

    @staticmethod
    def val(x):
        return float(x)

    def note(self, key, x):
        if self.notes is not None:
            self.notes.setdefault(key, []).append(self.val(x))


class MpMath(FloatMath):
    def __init__(self):
        import mpmath
        FloatMath.__init__(self)
        self.mp = mpmath.mp.clone()
        self.mp.dps = DPS
        for f in ("sin", "cos", "tan", "atan", "atan2", "tanh", "fabs", "fmod"):
            setattr(self, f, getattr(self.mp, f))

    def num(self, x):
        return self.mp.mpf(x)


class Dual:
    """value + NVAR directional derivatives, forward mode, over float"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v, self.d = v, (np.zeros(NVAR) if d is None else d)

    @staticmethod
    def seed(v, i):
        q = Dual(v)
        q.d[i] = 1.0
        return q

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d) if isinstance(o, Dual) else Dual(self.v + o, self.d)
    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d - o.d) if isinstance(o, Dual) else Dual(self.v - o, self.d)

    def __rsub__(self, o):
        return Dual(o - self.v, -self.d)

    def __mul__(self, o):
        return Dual(self.v * o.v, self.d * o.v + self.v * o.d) if isinstance(o, Dual) else Dual(self.v * o, self.d * o)
    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, Dual):
            return Dual(self.v / o, self.d / o)
        r = self.v / o.v
        return Dual(r, (self.d - r * o.d) / o.v)

    def __rtruediv__(self, o):
        r = o / self.v
        return Dual(r, -(r / self.v) * self.d)

    def chain(self, f, df):
        return Dual(f, self.d * df)


class DualMath(FloatMath):
    """The rules of the device's Dual (csrc/rl_dtrack.hpp): |x| by the sign of the value, fmod and max pass the derivative of
    the branch taken."""
    val = staticmethod(lambda x: x.v if isinstance(x, Dual) else float(x))
    sign = staticmethod(lambda x: FloatMath.sign(DualMath.val(x)))
    sin = staticmethod(lambda x: x.chain(math.sin(x.v), math.cos(x.v)))
    cos = staticmethod(lambda x: x.chain(math.cos(x.v), -math.sin(x.v)))
    tan = staticmethod(lambda x: x.chain(math.tan(x.v), 1.0 + math.tan(x.v) ** 2))
    tanh = staticmethod(lambda x: x.chain(math.tanh(x.v), 1.0 - math.tanh(x.v) ** 2))
    atan = staticmethod(lambda x: x.chain(math.atan(x.v), 1.0 / (1.0 + x.v * x.v)))
    fabs = staticmethod(lambda x: x.chain(math.fabs(x.v), -1.0 if x.v < 0.0 else 1.0))
    fmod = staticmethod(lambda x, m: Dual(math.fmod(x.v, m), x.d))
    max = staticmethod(lambda a, b: a if a.v >= b.v else b)

    @staticmethod
    def atan2(y, x):
        return Dual(math.atan2(y.v, x.v), (x.v * y.d - y.v * x.d) / (x.v * x.v + y.v * y.v))


# ---------------------------------------------------------------------------------------------------- double track
def dt_dynamics(M, m, x, u, k):
    """x = s, n, xi, omega, beta, v; u [4]; k curvature -> xdot [6], (Fx, Fy, Fz) [4] each (fl, fr, rl, rr)."""
    n, phi, omega, beta, v = x[1], x[2], x[3], x[4], x[5]
    drive = u[0] * (M.tanh(u[0]) * 0.5 + 0.5)
    brake = u[0] * (M.tanh(-u[0]) * 0.5 + 0.5)
    delta, transfer = u[2], u[3]
    lf, lr = m["lf"], m["lr"]
    l = lf + lr
    mass = m["mass"]
    fx_front = 0.5 * m["kd_f"] * drive + 0.5 * m["kb_f"] * brake - 0.5 * m["fr"] * mass * G * lr / l
    fx_rear = 0.5 * (1 - m["kd_f"]) * drive + 0.5 * (1 - m["kb_f"]) * brake - 0.5 * m["fr"] * mass * G * lf / l
    v2 = v * v
    ax = (drive + brake - 0.5 * m["cd"] * m["A"] * v2 - m["fr"] * mass * G) / mass
    fz_front = 0.5 * mass * G * lr / l - 0.5 * m["hcog"] / l * mass * ax + 0.25 * m["cl_f"] * m["rho"] * m["A"] * v2
    fz_rear = 0.5 * mass * G * lr / l + 0.5 * m["hcog"] / l * mass * ax + 0.25 * m["cl_r"] * m["rho"] * m["A"] * v2
    Fz = [fz_front - m["kroll_f"] * transfer, fz_front + m["kroll_f"] * transfer,
          fz_rear - (1 - m["kroll_f"]) * transfer, fz_rear + (1 - m["kroll_f"]) * transfer]
    M.note("sincos", beta)
    M.note("speed", v)
    sb, cb = M.sin(beta), M.cos(beta)
    slips = []
    for w, (arm, tw, sgn) in enumerate(((lf, m["twf"], -1.0), (lf, m["twf"], 1.0), (lr, m["twr"], -1.0), (lr, m["twr"], 1.0))):
        num = (arm * omega + v * sb) if w < 2 else (arm * omega - v * sb)
        den = (v * cb - 0.5 * tw * omega) if sgn < 0 else (v * cb + 0.5 * tw * omega)
        M.note("denominator", den)
        M.note("atan_kin", num / den)
        a = M.atan(num / den)
        slips.append(delta - a if w < 2 else a)
    mu = m["mu"]
    Fy = []
    for w in range(4):
        B, C = (m["Bf"], m["Cf"]) if w < 2 else (m["Br"], m["Cr"])
        M.note("atan_pac", B * slips[w])
        arg = C * M.atan(B * slips[w])
        M.note("sincos", arg)
        Fy.append(mu * Fz[w] * M.sin(arg))
    Fx = [fx_front, fx_front, fx_rear, fx_rear]
    drag = 0.5 * m["cd"] * m["rho"] * m["A"] * v2
    sum_fx_front, sum_fx_rear = Fx[0] + Fx[1], Fx[2] + Fx[3]
    sum_fy_front, sum_fy_rear = Fy[0] + Fy[1], Fy[2] + Fy[3]
    M.note("sincos", delta)
    M.note("sincos", delta - beta)
    sd, cd, sdb, cdb = M.sin(delta), M.cos(delta), M.sin(delta - beta), M.cos(delta - beta)
    dv = (sum_fx_rear * cb + sum_fx_front * cdb + sum_fy_rear * sb - sum_fy_front * sdb - drag * cb) / mass
    dbeta = -omega + (-sum_fx_rear * sb + sum_fx_front * sdb + sum_fy_rear * cb + sum_fy_front * cdb + drag * sb) / (mass * v)
    domega = ((Fx[3] - Fx[2]) * m["twr"] / 2 - sum_fy_rear * lr
              + ((Fx[1] - Fx[0]) * cd + (Fy[0] - Fy[1]) * sd) * m["twf"] / 2
              + (sum_fy_front * cd + sum_fx_front * sd) * lf) / m["Jzz"]
    M.note("sincos", phi + beta)
    M.note("one_minus_n_kappa", 1 - n * k)
    ds_dt = v * M.cos(phi + beta) / (1 - n * k)
    dn_dt = v * M.sin(phi + beta)
    dxi_dt = omega - k * ds_dt
    return [ds_dt, dn_dt, dxi_dt, domega, dbeta, dv], (Fx, Fy, Fz)


def dt_pair(M, m, trk, x, u, t, xn, un):
    """One node pair.  trk = (s_j, kappa_j, left_j, right_j, margin, track_length).  -> eq [8], ineq [14], cost term."""
    s_j, k, left, right, margin, L = trk
    xn = list(xn)
    d = xn[2] - x[2]
    M.note("sincos", d)
    M.note("yaw", math.fabs(M.val(d) % (2 * math.pi) - math.pi))
    xn[2] = M.atan2(M.sin(d), M.cos(d)) + x[2]
    ds = x[0] - xn[0]
    kk = M.fabs(ds) + L / 2.0
    r = M.val(M.fmod(kk, L))
    M.note("ds", math.fabs(M.val(ds)))
    M.note("fmod", min(r, L - r))
    xn[0] = xn[0] + (kk - M.fmod(kk, L)) * M.sign(ds)
    f1, (Fx, Fy, Fz) = dt_dynamics(M, m, x, u, k)
    f2, _ = dt_dynamics(M, m, xn, u, k)
    xm = [0.5 * (x[c] + xn[c]) + (t / 8.0) * (f1[c] - f2[c]) for c in range(6)]
    fm, _ = dt_dynamics(M, m, xm, u, k)
    eq = [x[c] + (t / 6.0) * (f1[c] + 4 * fm[c] + f2[c]) - xn[c] for c in range(6)]
    delta, transfer, v = u[2], u[3], x[5]
    M.note("sincos", delta)
    eq.append(transfer - m["hcog"] / (0.5 * (m["twf"] + m["twr"])) * (
        Fy[2] + Fy[3] + (Fx[0] + Fx[1]) * M.sin(delta) + (Fy[0] + Fy[1]) * M.cos(delta)))
    eq.append(x[0] - s_j)
    g = []
    for w in range(4):
        qx, qy = Fx[w] / (m["mu"] * Fz[w]), Fy[w] / (m["mu"] * Fz[w])
        g.append(qx * qx + qy * qy - 1.0)
    drive = u[0] * (M.tanh(u[0]) * 0.5 + 0.5)
    g.append(v * drive - m["Pmax"])
    g.append(1.0 - v)
    g += [m["Fb_max"] - u[0], u[0] - m["Fd_max"], -m["delta_max"] - delta, delta - m["delta_max"]]
    ru, rd = (un[0] - u[0]) / t, (un[2] - delta) / t
    lo_u, hi_u = m["Fb_max"] / m["Tb"] - ru, ru - m["Fd_max"] / m["Td"]
    lo_d, hi_d = -m["delta_max"] / m["Tdelta"] - rd, rd - m["delta_max"] / m["Tdelta"]
    M.note("rate_force", math.fabs(M.val(lo_u) - M.val(hi_u)))
    M.note("rate_steer", math.fabs(M.val(lo_d) - M.val(hi_d)))
    g += [M.max(lo_u, hi_u), M.max(lo_d, hi_d)]
    g += [(right + margin) - x[1], x[1] - (left - margin)]
    su = (m["Fd_max"], abs(m["Fb_max"]), m["delta_max"], m["mass"] * 50.0)
    a0, a1 = [u[q] / su[q] for q in range(4)], [un[q] / su[q] for q in range(4)]
    sq = a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2] + a1[3] * a1[3]
    df = [a1[q] - a0[q] for q in range(4)]
    cost = t + 1e-4 * sq + 1e-1 * (df[0] * df[0] + df[1] * df[1] + df[2] * df[2] + df[3] * df[3])
    return eq, g, cost


def pair_inputs(fam, b, j):
    """The 21 local variables of pair (b, j) and its track data."""
    N = fam["T"].shape[1]
    jn = (j + 1) % N
    z = list(fam["X"][b, j]) + list(fam["U"][b, j]) + [fam["T"][b, j]] + list(fam["X"][b, jn]) + list(fam["U"][b, jn])
    trk = (float(fam["s"][j]), float(fam["kappa"][j]), float(fam["left"][j]), float(fam["right"][j]), float(fam["margin"]),
           float(fam["L"]))
    return [float(q) for q in z], trk


def _split(z):
    return z[0:6], z[6:10], z[10], z[11:17], z[17:21]


def dt_values(M, m, trk, z):
    """All 23 outputs (8 eq, 14 ineq, cost term) of one pair at the 21 variables z, in M's scalars."""
    eq, g, cost = dt_pair(M, m, trk, *_split(z))
    return eq + g + [cost]


def dt_float(m, trk, z, record=False, math_ns=None):
    """-> values [23] (float), and the notes as a dict of lists when record."""
    M = math_ns or FloatMath(record)
    out = np.array(dt_values(M, m, trk, z), dtype=np.float64)
    return (out, M.notes) if record else out


def dt_dual(m, trk, z, math_ns=None):
    """-> values [23], Jacobian [23, 21] by the float dual."""
    out = dt_values(math_ns or DualMath(), m, trk, [Dual.seed(q, i) for i, q in enumerate(z)])
    return np.array([o.v for o in out]), np.stack([o.d for o in out])


def hi_lo(M, q):
    """mpf [..] -> float pairs [.., 2]: hi = the nearest double, lo = the rest."""
    flat = np.empty((len(q), 2))
    for i, x in enumerate(q):
        hi = float(x)
        flat[i] = hi, float(x - M.num(hi))
    return flat


def dt_reference(M, m, trk, z, jac=True):
    """mpmath values [23,2] and central-difference Jacobian [23,21,2] as (hi, lo) pairs."""
    zz = [M.num(q) for q in z]
    val = hi_lo(M, dt_values(M, m, trk, zz))
    if not jac:
        return val, None
    J = np.empty((23, NVAR, 2))
    for i in range(NVAR):
        h = M.num(10) ** -18 * max(1.0, abs(z[i]))
        up = dt_values(M, m, trk, [q + h if c == i else q for c, q in enumerate(zz)])
        dn = dt_values(M, m, trk, [q - h if c == i else q for c, q in enumerate(zz)])
        J[:, i] = hi_lo(M, [(a - b) / (2 * h) for a, b in zip(up, dn)])
    return val, J


def kinks_of(notes):
    """The least value of each kink quantity over one pair's evaluation, in the order of KINKS."""
    return np.array([min(abs(q) if key == "denominator" else q for q in notes[key]) for key in KINKS])


# ---------------------------------------------------------------------------------------------------- bicycle
def bk_dyn(M, m, th, de, v, a, dd):
    lr, L = m[0], m[1]
    M.note("atan_bk", de * (lr / L))
    beta = M.atan(de * (lr / L))
    M.note("sincos", beta)
    M.note("sincos", th + beta)
    cb = M.cos(beta)
    om = v * cb * M.tan(de) / L
    return [v * M.cos(th + beta), v * M.sin(th + beta), om, dd, a]


def bk_rk4(M, m, th, de, v, a, dd, dt):
    k1 = bk_dyn(M, m, th, de, v, a, dd)
    k2 = bk_dyn(M, m, th + dt * 0.5 * k1[2], de + dt * 0.5 * k1[3], v + dt * 0.5 * k1[4], a, dd)
    k3 = bk_dyn(M, m, th + dt * 0.5 * k2[2], de + dt * 0.5 * k2[3], v + dt * 0.5 * k2[4], a, dd)
    k4 = bk_dyn(M, m, th + dt * k3[2], de + dt * k3[3], v + dt * k3[4], a, dd)
    return [dt * (1.0 / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(5)], k1


def bk_node(M, m, p0, p0n, yaw, X, U, T, Xn):
    """Node j of rl_bicycle_eval_nodes from PHYSICAL inputs: c [6] (defects, longitudinal), d [2] (lateral, traction)."""
    w = [(X[0] - p0[0]) / SX[0], (X[1] - p0[1]) / SX[1]] + [X[i] / SX[i] for i in range(2, 5)] + [U[0] / SU[0], U[1] / SU[1], T]
    wn = [(Xn[0] - p0n[0]) / SX[0], (Xn[1] - p0n[1]) / SX[1]] + [Xn[i] / SX[i] for i in range(2, 5)]
    th, de, v = w[2] * SX[2], w[3] * SX[3], w[4] * SX[4]
    a, dd, dt = w[5] * SU[0], w[6] * SU[1], w[7]
    inc, k1 = bk_rk4(M, m, th, de, v, a, dd, dt)
    px, py = w[0] * SX[0], w[1] * SX[1]
    x1 = [px + p0[0], py + p0[1], th, de, v]
    x2 = [wn[0] * SX[0] + p0n[0], wn[1] * SX[1] + p0n[1]] + [wn[i] * SX[i] for i in range(2, 5)]
    dth = x2[2] - x1[2]
    M.note("yaw", math.fabs(M.val(dth) % (2 * math.pi) - math.pi))
    x2[2] = M.atan2(M.sin(dth), M.cos(dth)) + x1[2]
    c = [x1[i] + inc[i] - x2[i] for i in range(5)]
    cy, sy = M.cos(yaw), M.sin(yaw)
    c.append(cy * px + sy * py)
    return c + [-sy * px + cy * py, k1[2] * k1[2] * (k1[0] * k1[0] + k1[1] * k1[1]) + a * a]


def bk_eval(M, model, fam, conv=float):
    """All N nodes of a bicycle family (one instance) -> list of N lists of 8 scalars."""
    m = [float(model[k]) for k in BK_KEYS]
    N = len(fam["T"])
    c = lambda a: [conv(float(q)) for q in a]  # noqa: E731
    return [bk_node(M, m, c(fam["P0"][j]), c(fam["P0"][(j + 1) % N]), conv(float(fam["yaw"][j])), c(fam["X"][j]), c(fam["U"][j]),
                    conv(float(fam["T"][j])), c(fam["X"][(j + 1) % N])) for j in range(N)]


# ---------------------------------------------------------------------------------------------------- input families
DT_FAMILIES = ("tame", "cornering", "blend", "wraps", "limits", "shape")
SHAPE_PAIRS = (0, 63, 64, 127, 128, 129)
MARGIN = 1.2


def _corner(rng, X, U, j, b=0):
    X[b, j, 2] = rng.uniform(-3, 3); X[b, j, 4] = rng.uniform(-1.2, 1.2); X[b, j, 3] = rng.uniform(-1.5, 1.5)
    U[b, j, 2] = rng.uniform(-0.4, 0.4); X[b, j, 5] = rng.uniform(3, 80); U[b, j, 0] = rng.uniform(-6000, 6000)


def _fill(name, model, rng, X, U, T, b, j, state):
    """(Re)draw what family `name` changes at node (b, j) of random_problem's draw."""
    N = X.shape[1]
    if name in ("cornering", "shape"):
        _corner(rng, X, U, j, b)
    elif name == "blend":
        special = {1: 0.0, 7: 1e-3, 13: -1e-3, 19: 0.0}
        U[b, j, 0] = special[j] if j in special else rng.uniform(-30.0, 30.0)
    elif name == "wraps":
        k = int(rng.integers(-2, 3))
        if abs(state["turns"][j - 1] + k) > 2 and j > 0:
            k = -k
        if j > 0:
            state["turns"][j] = state["turns"][j - 1] + k
            X[b, j, 2] = X[b, j - 1, 2] + rng.normal(0, 0.05) + 2 * math.pi * k
        X[b, j, 0] = 3.0 * j + rng.normal(0, 0.05) + (0.0 if j % 3 else (3.0 * N if j % 6 else -3.0 * N))
    elif name == "limits":
        # even nodes low, odd nodes high: pair (even, odd) has the upper side of both rate rows active, (odd, even) the lower
        lo_u, hi_u = (model["Fb_max"], -15000.0), (model["Fd_max"], 15000.0)
        U[b, j, 0] = (hi_u if j % 2 else lo_u)[(j // 2) % 2]
        dm = model["delta_max"]
        U[b, j, 2] = (dm if j % 4 == 1 else rng.uniform(0.05, 0.3)) if j % 2 else (-dm if j % 4 == 0 else rng.uniform(-0.3, -0.05))
        if j % 6 == 2:
            X[b, j, 5] = 1.0
            X[b, j, 3] = float(np.clip(X[b, j, 3], -0.3, 0.3))
    if name != "tame":
        T[b, j] = 3.0 / X[b, j, 5] * rng.uniform(0.9, 1.1)


def family_kinks(model, fam):
    """Kink quantities [B, N, len(KINKS)] of every pair of a family, by the recording float twin."""
    B, N = fam["T"].shape
    out = np.empty((B, N, len(KINKS)))
    for b in range(B):
        for j in range(N):
            z, trk = pair_inputs(fam, b, j)
            out[b, j] = kinks_of(dt_float(model, trk, z, record=True)[1])
    return out


def draw_dt_family(name, model, seed):
    """Inputs of one double-track family: random_problem's draw with the family's changes; a pair that misses a kink condition
    has its two nodes drawn again (from the same stream) until every pair holds them.  None if that does not end (`tame`, which
    is random_problem's draw untouched, cannot redraw a node: another seed)."""
    from test_double_track import random_problem
    B, N = (3, 130) if name == "shape" else (1, 24)
    s, kappa, left, right, L, X, U, T = random_problem(B, N, seed=seed)
    fam = dict(s=s, kappa=kappa, left=left, right=right, L=float(L), margin=MARGIN, X=X, U=U, T=T)
    rng = np.random.default_rng([seed, 1])
    state = {"turns": np.zeros(N, dtype=int)}
    todo = [(b, j) for b in range(B) for j in range(N)]
    for _ in range(200):
        for b, j in todo:
            _fill(name, model, rng, X, U, T, b, j, state)
        bad = np.argwhere((family_kinks(model, fam) < np.array(KINK_MIN)).any(axis=2))
        if len(bad) == 0:
            stored = [(b, j) for b in range(B) for j in (SHAPE_PAIRS if name == "shape" else range(N))]
            fam["pairs"] = np.array(stored)
            return fam
        if name == "tame":
            return None
        nodes = sorted({(int(b), int(q) % N) for b, j in bad for q in (j, j + 1)})
        todo = nodes if name != "wraps" else [(0, j) for j in range(min(j for _, j in nodes), N)]
    return None


def bk_sweep_family():
    """rl_bicycle_eval_nodes as a direct sweep of m_sincos: delta = a = delta_dot = 0, v = 40, T = 0.05, P0 = 0, so that the four
    RK4 stages coincide and defect rows 0 / 1 are T v cos(theta) / T v sin(theta) minus nothing."""
    N = 512
    th = []
    for mm in range(-16, 17):
        base = mm * math.pi / 4
        for n_ulp in (-4, -2, -1, 0, 1, 2, 4):
            q = base
            for _ in range(abs(n_ulp)):
                q = float(np.nextafter(q, math.inf if n_ulp > 0 else -math.inf))
            th.append(q)
    th += [0.0, -0.0, 1e-300, -1e-300, 2.0 ** -27, -2.0 ** -27]
    rng = np.random.default_rng(16)
    th += list(rng.uniform(-4 * math.pi, 4 * math.pi, N - len(th)))
    X = np.zeros((N, 5)); X[:, 2] = th; X[:, 4] = 40.0
    return dict(P0=np.zeros((N, 2)), yaw=np.zeros(N), X=X, U=np.zeros((N, 2)), T=np.full(N, 0.05))


def bk_general_family():
    """The first 24 nodes of the perturbed Monza-20 m point of test_bicycle_gpu.test_eval_nodes_matches_the_twin (instance 0)."""
    import bicycle_problem as bp
    import bicycle_twin as bt
    pts, _ = bp.monza_table(20.0)
    P0, yaw, dl, dr = bp.table_data(pts)
    rng = np.random.default_rng(7)
    X, U, T = bt.initial_guess("centerline", P0, yaw)
    Xs = np.stack([X + rng.normal(size=X.shape) * [2, 2, 0.1, 0.1, 5] for _ in range(2)])
    Us = rng.normal(size=(2,) + U.shape) * [5, 0.5]
    N = 24
    return dict(P0=P0[:N].copy(), yaw=yaw[:N].copy(), X=Xs[0, :N].copy(), U=Us[0, :N].copy(), T=(T * 1.2)[:N].copy())


# ---------------------------------------------------------------------------------------------------- coverage
def atan_interval(x):
    return int(np.searchsorted(ATAN_BREAKS, abs(x), side="right"))


def atan_coverage(args):
    """args [P, n]: number of pairs (rows) that enter each of m_atan's five intervals."""
    iv = np.searchsorted(ATAN_BREAKS, np.abs(args), side="right")
    return np.array([(iv == i).any(axis=1).sum() for i in range(5)])


def sincos_coverage(args):
    """[4, 2]: arguments per residue of rint(2x/pi) mod 4 and sign of x (column 0: x < 0, column 1: x > 0)."""
    a = np.asarray(args).ravel()
    k = np.rint(a * (2 / math.pi)).astype(np.int64) % 4
    return np.array([[np.sum((k == r) & (a < 0)), np.sum((k == r) & (a > 0))] for r in range(4)])


# ---------------------------------------------------------------------------------------------------- the tolerance rule
ROW_GROUPS = {"defects": range(0, 6), "load transfer": (6,), "pin": (7,), "ellipses": range(8, 12), "power": (12,),
              "bounds": (13, 14, 15, 16, 17, 20, 21), "rates": (18, 19), "cost": (22,)}
MARGIN_BITS = 16.0     # fma contraction, another association order, 1-ulp elementary functions, three nested dynamics calls


def deviation(x, ref):
    """|x - reference| with the reference a (hi, lo) pair in the last axis."""
    return np.abs((x - ref[..., 0]) - ref[..., 1])


def allowance(ref, twin, axes):
    """Per output row: what honest double arithmetic achieves on the family's inputs (the worst deviation of the double twin),
    floored at one unit in the last place of the row's largest reference value."""
    return np.maximum(deviation(twin, ref).max(axis=axes), 2.0 ** -52 * np.abs(ref[..., 0]).max(axis=axes))


def ratios(x, ref, twin, axes):
    """Per output row: worst |x - reference| in units of the row's allowance (0 / 0 = 0: a row that is exactly 0 in the
    reference and the twin must be exactly 0)."""
    dev, allow = deviation(x, ref).max(axis=axes), allowance(ref, twin, axes)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dev == 0.0, 0.0, dev / allow)


def group_worst(r):
    """{row group: worst ratio} of a per-row vector r (the first len(r) of the 23 rows)."""
    return {k: float(max(r[i] for i in v if i < len(r))) for k, v in ROW_GROUPS.items() if any(i < len(r) for i in v)}
