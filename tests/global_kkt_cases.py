"""Test helper: the ONE list of global min-curvature QP cases that tests/test_optimality_cpu.py certifies on the CPU twins and
tests/test_optimality_gpu.py on the kernels (k_global_qp, k_global_qp2 plain and weighted, k_global_xy), and the procedure.

The procedure.  A run with n_outer = m returns a_m, the answer of the QP linearised about a_{m-1}.  a_{m-1} is NOT what a call
with n_outer = m - 1 returns: that call leaves its last linearisation at the final tolerance, the m-run left the same
linearisation at the intermediate one (rl_device.hpp: ipm_done), and the two points differ by 3e-4 .. 1.2e-2 m.  The test hook
"global_last_as_mid" (include/rl_mincurv.h; the twins have the same switch) makes the (m-1)-call leave like the m-run did, so it
returns the m-run's own a_{m-1}, bit for bit.  a_m is then certified (tests/kkt_certificate.py) on the independently assembled
QP at that point, and held to 1e-4 m (north_star's tolerance) of the exact optimum a* of that QP, an active-set polish
(kkt_certificate.polish_qp) that must itself certify 1000 times under the stationarity bound.

A solver is anything with
    one(inp, W [B,N,2], margin, n_outer, hook, weights=None) -> a [B,n_p], stats [B,8]
    xy(inp, W [B,N,2], margin, lon, n_outer, hook)           -> z [B,n_p,2], stats [B,8]
(TwinSolver here; the GPU module wraps ops.global_batch_host).  Inputs: the kart circuit's splines `c` (n_p = 63: k_global_qp2)
and `cb` (n_p = 67: the generic kernel) of fixture G14 with the half-widths of its own rings (3.02 .. 4.27 m), and Monza."""
import contextlib
import functools
import types

import numpy as np

import kart_cases as kcs
import kkt_certificate as kc
from conftest import golden
from oracle import oracle as orc
from test_global_qp import MARGIN, NumpyGlobal, monza_widths
from test_global_qp_xy import LON, NumpyGlobalXY

DIST = 1e-4          # [m] north_star's tolerance: the returned point against the exact optimum of the QP it solved
POLISH_STAT = 1e-3   # the polished point certifies at this share of the stationarity bound (measured: <= 1e-8)


def case(kind, track, N, margin, n_outer, weights=None, env=None, scale=None):
    tag = f"{kind}-{track}-N{N}-m{margin}-o{n_outer}" + (f"-{weights}" if weights else "") + ("-v1" if env else "") + \
        ("-B4" if scale else "")
    return types.SimpleNamespace(kind=kind, track=track, N=N, margin=margin, n_outer=n_outer, weights=weights, env=env or {},
                                 scale=scale, id=tag)


CASES = (
    # 1. kart, one offset per control point
    [case("one", "kart_c", 400, 2.0, m) for m in (1, 2, 3)] +
    [case("one", "kart_c", 800, 0.25, 3), case("one", "kart_c", 800, 2.0, 2), case("one", "kart_c", 200, 1.0, 2),
     case("one", "kart_c", 400, 1.0, 3), case("one", "kart_cb", 400, 1.5, 2), case("one", "kart_c", 400, 0.25, 1),
     case("one", "kart_c", 400, 0.25, 6), case("one", "kart_c", 400, 0.25, 3, env={"RL_GLOBAL_V1": "1"})] +
    # 2. Monza with a wide margin
    [case("one", "monza_c30", 500, 2.0, 3), case("one", "monza_c100", 500, 2.0, 3)] +
    # 3. the centre line starts outside the corridor
    [case("one", f"monza_c100_off{off}", 500, MARGIN, m) for off in (1.05, 1.5) for m in (1, 3)] +
    # 4. weighted
    [case("one", tr, N, mg, m, weights=w) for tr, N, mg, m in (("kart_c", 400, 1.0, 1), ("kart_c", 400, 1.0, 3),
                                                              ("monza_c100", 500, MARGIN, 3)) for w in ("speed", "exp2")] +
    # 5. both coordinates free
    [case("xy", "kart_c", 400, mg, m) for mg in (0.25, 1.0, 2.0) for m in (1, 3)] +
    # 6. a batch of four, rows 0 and 3 the same instance
    [case("one", "kart_c", 400, 1.0, 3, scale=(1.0, 0.9, 1.1, 1.0))]
)
# The cases that the last linearisation's exit at complementarity 1e-10 (rl_device.hpp: kIpmTolLast) fails, kept in the list as
# strict expected failures.  Figures: the CPU twins (stationarity / complementarity as shares of their bounds, distance to the
# exact optimum of the QP; bound 1e-4 m); the kernels': tests/test_optimality_gpu.py's docstring.  The four one-offset cases
# pass on the twins at 1e-12 (1.6e-8, 2.5e-6, 8.1e-7, 2.3e-6 m), which the kernels do not survive; the two with both
# coordinates free stay at 1.0e-4 / 1.9e-4 m at 1e-12, and one more iteration breaks down.
KNOWN_FAILURES = {
    "one-kart_c-N400-m2.0-o1": "exit at 1e-10: stationarity 1.23x, complementarity 0.42x, 1.09e-4 m from the optimum (1e-12: 1.6e-8 m)",
    "one-kart_c-N800-m0.25-o3": "exit at 1e-10: stationarity 1.06x, complementarity 1.42x, 1.46e-4 m (1e-12: 2.5e-6 m)",
    "one-monza_c100-N500-m2.0-o3": "exit at 1e-10: stationarity 0.06x, 1.13e-3 m from the optimum (1e-11: 1.08e-4 m, 1e-12: 8.1e-7 m)",
    "one-monza_c100-N500-m0.25-o3-exp2": "exit at 1e-10: stationarity 0.002x, 3.13e-4 m from the optimum (1e-12: 2.3e-6 m)",
    "xy-kart_c-N400-m2.0-o1": "exit at 1e-10: stationarity 0.26x, 7.65e-4 m from the optimum (1e-12: 1.02e-4 m, 1e-13: NaN)",
    "xy-kart_c-N400-m2.0-o3": "exit at 1e-10: stationarity 0.11x, 9.49e-4 m from the optimum (1e-12: 1.85e-4 m)",
}
EXIT_RULE_CASES = ("one-kart_c-N400-m2.0-o1", "one-kart_c-N800-m0.25-o3")     # the two that miss the certificate's own bounds
OLD_PREMISE_CASE = "one-monza_c30-N500-m2.0-o3"


def params():
    """The list for pytest.mark.parametrize: every case, the known failures as xfail(strict=True) -- a case that starts to pass
    fails the suite until it is taken off the list."""
    import pytest
    assert set(KNOWN_FAILURES) <= {c.id for c in CASES}
    return [pytest.param(c, id=c.id, marks=[pytest.mark.xfail(strict=True, raises=AssertionError, reason=KNOWN_FAILURES[c.id])]
                         if c.id in KNOWN_FAILURES else []) for c in CASES]


def by_id(tag):
    return next(c for c in CASES if c.id == tag)


@functools.lru_cache(maxsize=None)
def inputs(track, N):
    """-> namespace t, cx, cy, k, u, wl, wr (half-widths of the track's own rings)."""
    if track.startswith("kart"):
        name = {"kart_c": "base", "kart_cb": "driven_backwards"}[track]
        from spline_trajectory_optimization_amd import batch
        t, cx, cy, k = kcs.case(name)[:4]
        wl, wr = batch.half_widths_from_bounds(kcs.centre_table(name, N))
        u = np.linspace(0, 1, N, endpoint=False)
    else:
        tag, _, off = track[len("monza_"):].partition("_off")
        t, cx, cy, k, u, wl, wr = monza_widths(golden("G1_spline_fits.npz"), tag, N)
        if off:                                              # the corridor moved sideways: the centre line is outside it
            w = wl + wr
            wl = (1.0 - float(off)) * w + 0.25
            wr = w - wl
    return types.SimpleNamespace(t=t, cx=cx, cy=cy, k=int(k), u=u, wl=np.ascontiguousarray(wl), wr=np.ascontiguousarray(wr),
                                 n_p=len(cx) - int(k))


WEIGHTS = {"speed": lambda N: 1.0 / np.linspace(20.0, 80.0, N),
           "exp2": lambda N: np.exp2(np.random.default_rng(3).uniform(-10, 10, N))}


def weights_of(name, N):
    return None if name is None else WEIGHTS[name](N)


def widths_of(c):
    inp = inputs(c.track, c.N)
    W = np.stack([inp.wl, inp.wr], 1)[None]
    return np.ascontiguousarray(W * np.asarray(c.scale or (1.0,))[:, None, None])


# ------------------------------------------------------------------------------------------- the independent QPs
def gauss_newton_rows(ng, a, h=1e-3):
    """(G, A, kappa) at a: Gauss-Newton rows by central differences of scipy's curvature, constraint rows by moving one control
    point at a time (NumpyGlobal.qp_at's own loop, with the pieces handed out)."""
    N, m = len(ng.u), ng.np
    G = np.zeros((N, m)); A = np.zeros((N, m))
    for j in range(m):
        e = np.zeros(m); e[j] = 1.0
        G[:, j] = (ng.kappa(a + h * e) - ng.kappa(a - h * e)) / (2 * h)
        A[:, j] = ng.lateral(e)
    return G, A, ng.kappa(a)


def scaled_qp(G, kappa, a, w=None):
    """P = 2 G'WG scaled to trace n_p plus 1e-9 I, q = 2 G'W (kappa - G a) on the same scale (W = I for w = None)."""
    GW = G if w is None else G * w[:, None]
    P = 2 * GW.T @ G
    q = 2 * GW.T @ (kappa - G @ a)
    sc = G.shape[1] / np.trace(P)
    return P * sc + 1e-9 * np.eye(G.shape[1]), q * sc


def weighted_qp_at(ng, a, w=None, h=1e-3):
    """-> P, q, A of the (weighted) linearisation at a; with w = None the numbers of NumpyGlobal.qp_at."""
    G, A, kap = gauss_newton_rows(ng, a, h)
    P, q = scaled_qp(G, kap, a, w)
    return P, q, A


@functools.lru_cache(maxsize=None)
def statement(kind, track, N):
    inp = inputs(track, N)
    return (NumpyGlobal if kind == "one" else NumpyGlobalXY)(inp.t, inp.cx, inp.cy, inp.k, inp.u)


# ------------------------------------------------------------------------------------------------------ the solvers
class TwinSolver:
    """The CPU twins: oracle.global_mincurv / global_mincurv_xy, tests/weighted_global_twin.py for the weighted cost."""

    def one(self, inp, W, margin, n_outer, hook, weights=None):
        import weighted_global_twin as tw
        out = []
        for b in range(len(W)):
            if weights is None:
                with orc.global_last_as_mid(hook):
                    r = orc.global_mincurv(inp.t, inp.cx, inp.cy, inp.k, W.shape[1], W[b, :, 0], W[b, :, 1], margin, n_outer)
            else:
                r = tw.global_mincurv_weighted(inp.t, inp.cx, inp.cy, inp.k, W.shape[1], W[b, :, 0], W[b, :, 1], margin, n_outer,
                                               weights=weights, last_as_mid=hook)
            out.append((r[3], np.r_[r[4], np.zeros(8 - len(r[4]))]))
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def xy(self, inp, W, margin, lon, n_outer, hook):
        out = []
        for b in range(len(W)):
            with orc.global_last_as_mid(hook):
                r = orc.global_mincurv_xy(inp.t, inp.cx, inp.cy, inp.k, W.shape[1], W[b, :, 0], W[b, :, 1], margin, lon, n_outer)
            out.append((r[3], r[4]))
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@contextlib.contextmanager
def hook(ctx, on=True):
    """with hook(ctx): ...  -- the calls inside run with the library's test hook "global_last_as_mid" set.  on=False touches
    nothing: a context that never had the option set stays one."""
    if not on:
        yield ctx
        return
    ctx.set_option("global_last_as_mid", 1)
    try:
        yield ctx
    finally:
        ctx.set_option("global_last_as_mid", 0)


class KernelSolver:
    """The kernels through ops.global_batch_host on one context (default: the process's cached one).  last_rs: the rl_stats of
    the last call (block_threads and lds_bytes tell which kernel ran)."""

    def __init__(self, ctx=None):
        from spline_trajectory_optimization_amd import _lib, ops
        self.lib, self.ops = _lib, ops
        self.ctx = ctx or _lib.Context.get(0)   # raises loudly when the HIP extension / device is missing
        self.tracks, self.last_rs = {}, None

    def track(self, inp, N):
        key = (id(inp), N)
        if key not in self.tracks:
            self.tracks[key] = self.lib.Track(self.ctx, inp.t, inp.cx, inp.cy, inp.k, N)
        return self.tracks[key]

    def one(self, inp, W, margin, n_outer, hook_on, weights=None):
        with hook(self.ctx, hook_on):
            _, _, a, st, self.last_rs = self.ops.global_batch_host(self.track(inp, W.shape[1]), W, margin, n_outer, weights=weights)
        return a, st

    def xy(self, inp, W, margin, lon, n_outer, hook_on):
        with hook(self.ctx, hook_on):
            _, _, z, st, self.last_rs = self.ops.global_batch_host(self.track(inp, W.shape[1]), W, margin, n_outer, dof=2, lon=lon)
        return z, st


def solve_case(solver, c):
    """The case's two calls -> (x_m, stats_m, x_{m-1}, stats_{m-1}); x_{m-1} from the (m-1)-call with the hook ON (zeros and
    None for m = 1).  `hooked` selects the hook of the second call: False is the old, wrong premise (kept callable so that a
    test can show it failing)."""
    return solve_case_with(solver, c, hooked=True)


def solve_case_with(solver, c, hooked):
    inp, W = inputs(c.track, c.N), widths_of(c)
    w = weights_of(c.weights, c.N)
    if c.kind == "one":
        call = lambda m, hook: solver.one(inp, W, c.margin, m, hook, weights=w)  # noqa: E731
        zero = np.zeros((len(W), inp.n_p))
    else:
        call = lambda m, hook: solver.xy(inp, W, c.margin, LON, m, hook)  # noqa: E731
        zero = np.zeros((len(W), inp.n_p, 2))
    x, st = call(c.n_outer, False)
    if c.n_outer == 1:
        return x, st, zero, None
    xp, stp = call(c.n_outer - 1, hooked)
    return x, st, xp, stp


# ------------------------------------------------------------------------------------------------- the certificate
def certify_case(c, x, st, xp, stp, report):
    """Every row of the case's batch on its own widths and its own x_{m-1}: certificate within kkt_certificate's bounds, the exact
    optimum a* of the same QP within POLISH_STAT of the stationarity bound, |x - a*|_inf <= DIST.  -> the figures, row by row."""
    inp, W = inputs(c.track, c.N), widths_of(c)
    w = weights_of(c.weights, c.N)
    ng = statement(c.kind, c.track, c.N)
    N, figures = c.N, []
    for b in range(len(W)):
        wl, wr = W[b, :, 0], W[b, :, 1]
        if c.kind == "one":
            P, q, A = weighted_qp_at(ng, xp[b], w)
            lo, hi = -(wr - c.margin), wl - c.margin
            sol, halved = x[b], 0
        else:
            halved = int(st[b, 7]) - (int(stp[b, 7]) if stp is not None else 0)
            assert halved in (0, 1)
            sol = (xp[b] + (x[b] - xp[b]) * (2.0 if halved else 1.0)).reshape(-1)     # the QP's own answer: the whole step
            P, q, A = ng.qp_at(xp[b])
            lo = np.concatenate([-(wr - c.margin), -LON * np.ones(N)]); hi = np.concatenate([wl - c.margin, LON * np.ones(N)])
        cert, bounds = kc.certify_qp(P, q, A, lo, hi, sol)
        star, nwork, passes = kc.polish_qp(P, q, A, lo, hi, sol)
        cstar, bstar = kc.certify_qp(P, q, A, lo, hi, star)
        dist = float(np.abs(sol - star).max())
        tag = f"{c.id} row {b} n_p={inp.n_p}" + (f" halved={halved}" if c.kind == "xy" else "")
        report(tag, cert, bounds)
        print(f"    ipm {int(st[b, 0])}" + (f" ({c.n_outer - 1}-run {int(stp[b, 0])})" if stp is not None else "") +
              f"  stat/bound {cert.stat / bounds[0]:.3f}  compl/bound {cert.compl / bounds[1]:.3f}  |x - a*| {dist:.2e} m  "
              f"a*: {nwork} working rows after {passes} passes, stat/bound {cstar.stat / bstar[0]:.1e} compl/bound "
              f"{cstar.compl / bstar[1]:.1e} viol {cstar.viol:.1e}")
        figures.append(types.SimpleNamespace(cert=cert, bounds=bounds, cstar=cstar, bstar=bstar, dist=dist, halved=halved,
                                             lo=lo, hi=hi, A=A))
    return figures


def assert_case(c, x, st, xp, stp, figures):
    for b, f in enumerate(figures):
        assert np.isfinite(x[b]).all() and st[b, 0] < 80 * c.n_outer                     # no linearisation ran into the cap
        assert f.cstar.stat <= POLISH_STAT * f.bstar[0] and f.cstar.compl <= f.bstar[1] and f.cstar.viol <= f.bstar[2]
        assert f.cert.viol <= f.bounds[2]
        assert f.cert.stat <= f.bounds[0] and f.cert.compl <= f.bounds[1]
        if c.kind == "one":
            assert f.cert.viol <= st[b, 3] + f.bounds[2]                                 # the solver's own figure does not under-report
        assert f.dist <= DIST
        if stp is not None:
            assert st[b, 0] > stp[b, 0]                                                  # the m-run went on from there
    if c.scale:                                                                          # rows 0 and 3 are the same instance
        assert c.scale[0] == c.scale[3]
        assert x[0].tobytes() == x[3].tobytes() and st[0].tobytes() == st[3].tobytes()
        assert xp[0].tobytes() == xp[3].tobytes() and stp[0].tobytes() == stp[3].tobytes()
        assert np.abs(x[0] - x[1]).max() > 1e-3                                          # and the other rows are not
