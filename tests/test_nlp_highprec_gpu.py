"""The device code under both min-time solvers (csrc/rl_dtrack.hpp: the double-track model, the forward-mode Dual arithmetic,
m_sincos / m_atan; csrc/rl_bicycle.hpp: the bicycle node functions) against a 50-digit reference -- fixture G16
(tests/golden/make_golden_nlp_highprec.py, tests/nlp_highprec.py), through the entry points rl_dt_eval_nodes, rl_dt_eval_jac and
rl_bicycle_eval_nodes.  The tests read the fixture only.

Tolerance.  Per family and output row, the yardstick is what honest double arithmetic achieves on those inputs,
    yard = max over the family's pairs of |double twin - reference|      (Python float / a float dual; from the fixture),
and a row passes when  |kernel - reference| <= FACTOR x max(yard, 2^-52 max|reference| of the row over the family).
FACTOR = 16: fma contraction, another association order, elementary functions of 1 ulp instead of libm's 1/2, all of it
compounding through three nested dynamics evaluations per defect.  A Jacobian row is one function's 21 derivatives.

Measured on an MI355X: allowance unit (the yardstick, floored at one ulp of the row's largest value) / worst kernel ratio, per
family and row group (the same table: DESIGN.md section 7).  No row needed a factor above 16; no kernel changed.

  family, output      defects          load transfer    pin              ellipses         power            bounds           rates            cost
  tame values         1.2e-14 / 1.00   2.2e-12 / 0.83   2.1e-17 / 0.00   3.1e-16 / 1.40   6.0e-11 / 0.11   5.5e-12 / 0.38   5.9e-11 / 0.23   9.1e-16 / 0.20
  tame Jacobian       2.1e-14 / 1.17   5.8e-11 / 0.81   2.2e-16 / 0.00   9.8e-15 / 1.96   1.1e-12 / 0.00   2.2e-16 / 0.00   1.5e-09 / 0.61   2.2e-16 / 0.15
  cornering values    1.2e-14 / 1.00   2.5e-12 / 0.73   3.0e-17 / 0.00   4.9e-16 / 1.00   6.0e-11 / 0.24   5.7e-12 / 0.32   4.2e-11 / 0.38   1.6e-15 / 1.00
  cornering Jacobian  7.6e-14 / 1.91   3.2e-11 / 1.00   2.2e-16 / 0.00   1.5e-14 / 1.30   1.3e-12 / 0.00   2.2e-16 / 0.00   1.2e-09 / 0.52   2.2e-16 / 0.53
  blend values        1.2e-14 / 1.34   1.8e-12 / 0.57   2.1e-17 / 0.00   4.2e-16 / 1.00   6.0e-11 / 0.48   4.4e-12 / 0.38   1.8e-12 / 0.73   4.9e-16 / 1.00
  blend Jacobian      1.6e-14 / 1.62   5.9e-11 / 1.00   2.2e-16 / 0.00   8.3e-15 / 2.13   5.2e-14 / 1.00   2.2e-16 / 0.00   3.8e-12 / 1.30   2.2e-16 / 0.12
  wraps values        1.1e-14 / 1.29   1.6e-12 / 0.92   1.6e-14 / 0.44   3.7e-16 / 1.36   6.0e-11 / 0.21   5.8e-12 / 0.37   1.1e-10 / 0.66   1.6e-15 / 0.38
  wraps Jacobian      7.0e-14 / 1.22   6.0e-11 / 0.61   2.2e-16 / 0.00   1.3e-14 / 1.18   1.3e-12 / 0.00   2.2e-16 / 0.00   2.7e-09 / 1.17   2.2e-16 / 0.12
  limits values       6.8e-14 / 1.16   1.6e-12 / 0.90   2.4e-17 / 0.00   8.4e-16 / 1.00   2.0e-10 / 0.22   7.8e-12 / 0.31   1.8e-10 / 0.42   1.3e-14 / 0.41
  limits Jacobian     6.0e-12 / 2.45   3.2e-11 / 0.99   2.2e-16 / 0.00   1.2e-14 / 1.01   3.3e-12 / 0.00   2.2e-16 / 0.00   4.5e-09 / 0.93   2.2e-16 / 0.53
  shape values        2.8e-14 / 1.63   1.6e-12 / 1.03   2.9e-17 / 0.00   8.0e-16 / 1.10   6.0e-11 / 0.06   5.7e-12 / 0.32   4.8e-11 / 0.41   -
  shape Jacobian      1.2e-14 / 1.31   1.9e-11 / 1.39   2.2e-16 / 0.00   3.5e-14 / 1.94   1.3e-12 / 0.00   2.2e-16 / 0.00   1.1e-09 / 0.59   2.2e-16 / 0.41

  bicycle family      defect x         defect y         defect theta     defect delta     defect v         longitudinal     lateral          traction
  bk_sweep            1.8e-15 / 1.00   3.6e-15 / 1.00   3.6e-15 / 1.00   0 / 0.00         0 / 0.00         0 / 0.00         0 / 0.00         0 / 0.00
  bk_general          7.1e-13 / 0.31   1.4e-12 / 0.33   1.8e-13 / 1.00   7.4e-16 / 0.65   7.9e-15 / 0.49   1.1e-15 / 0.55   8.0e-16 / 0.31   4.1e-14 / 0.72

On bk_sweep the kernel's m_sincos differs from libm at the same double angle by at most 1.5 (cos) / 1.0 (sin) ulp of T v."""
import math

import numpy as np
import pytest

import nlp_highprec as hp
from conftest import golden
from oracle import dt_checker as dt
from test_double_track import MODEL

pytestmark = pytest.mark.gpu

FACTOR = hp.MARGIN_BITS
RAISED = {}      # (family, "val" | "jac", row group) -> raised factor, with the reason next to it; none was needed


@pytest.fixture(scope="module")
def g16():
    g = golden("G16_nlp_highprec.npz")
    return {k: g[k] for k in g.files}


def _inputs(g16, name):
    """The nine arguments of ops.dt_eval_nodes / dt_eval_jac after the model."""
    scalars = (float(g16[f"{name}_margin"]), float(g16[f"{name}_L"]))
    return tuple(g16[f"{name}_{k}"] for k in ("s", "kappa", "left", "right")) + scalars + tuple(g16[f"{name}_{k}"] for k in ("X", "U", "T"))


def _judge(name, kind, r, allow):
    """Print the worst ratio and the yardstick per row group, then assert every row."""
    worst = hp.group_worst(r)
    yard = {k: float(max(allow[i] for i in v if i < len(allow))) for k, v in hp.ROW_GROUPS.items() if k in worst}
    print(f"[nlp_highprec {name} {kind}] " + "; ".join(f"{k}: ratio {worst[k]:.2f} (yard {yard[k]:.1e})" for k in worst))
    for k, rows in hp.ROW_GROUPS.items():
        for i in rows:
            if i < len(r):
                assert r[i] <= RAISED.get((name, kind, k), FACTOR), (name, kind, k, i, float(r[i]))


@pytest.mark.parametrize("name", hp.DT_FAMILIES)
def test_dt_eval_nodes_vs_50_digits(g16, name):
    from spline_trajectory_optimization_amd import ops
    eq, ineq, cost = ops.dt_eval_nodes(MODEL, *_inputs(g16, name))
    b, j = g16[f"{name}_pairs"].T
    got = np.concatenate([eq[b, j], ineq[b, j]], axis=1)
    ref, twin = g16[f"{name}_ref_val"], g16[f"{name}_twin_val"]
    assert np.isfinite(eq).all() and np.isfinite(ineq).all()
    _judge(name, "val", hp.ratios(got, ref[:, :22], twin[:, :22], 0), hp.allowance(ref[:, :22], twin[:, :22], 0))
    if name != "shape":            # every pair of the instance is stored: the objective is the sum of their terms, in node order
        parts = ref[:, 22].ravel().tolist()
        hi = math.fsum(parts)
        total = np.array([[[hi, math.fsum(parts + [-hi])]]])
        tw = 0.0
        for c in twin[:, 22]:
            tw += c
        tw = np.array([[tw]])
        r = hp.ratios(cost[None, :1], total, tw, 0)
        print(f"[nlp_highprec {name} val] cost: ratio {float(r[0]):.2f} (yard {float(hp.allowance(total, tw, 0)[0]):.1e})")
        assert r[0] <= FACTOR


@pytest.mark.parametrize("name", hp.DT_FAMILIES)
def test_dt_eval_jac_vs_50_digit_differences(g16, name):
    """All 21 variables of every stored pair: the seven blockIdx.z slices of k_dt_eval_jac."""
    from spline_trajectory_optimization_amd import ops
    args = _inputs(g16, name)
    je, ji, gc = ops.dt_eval_jac(MODEL, *args)
    b, j = g16[f"{name}_pairs"].T
    got = np.concatenate([je[b, j], ji[b, j], gc[b, j][:, None, :]], axis=1)
    ref, twin = g16[f"{name}_ref_jac"], g16[f"{name}_twin_jac"]
    assert np.isfinite(je).all() and np.isfinite(ji).all() and np.isfinite(gc).all()
    _judge(name, "jac", hp.ratios(got, ref, twin, (0, 2)), hp.allowance(ref, twin, (0, 2)))
    # structure, on every pair the kernel wrote: the abscissa pin and the simple bounds have constant unit derivatives
    assert np.all(je[:, :, 7, 0] == 1.0) and np.all(je[:, :, 7, 1:] == 0.0)
    for row, var, one in ((5, 5, -1.0), (6, 6, -1.0), (7, 6, 1.0), (8, 8, -1.0), (9, 8, 1.0), (12, 1, -1.0), (13, 1, 1.0)):
        rest = np.delete(ji[:, :, row, :], var, axis=-1)
        assert np.all(ji[:, :, row, var] == one) and np.all(rest == 0.0), row
    assert np.all(gc[:, :, 10] == 1.0)
    # the rate rows carry the derivative of the side the reference says is active: +-1/t with respect to the next node's control
    t = args[8][b, j]
    for row, var in ((10, 17), (11, 19)):
        side = np.sign(ref[:, 8 + row, var, 0])
        assert np.all(side != 0.0)
        assert np.all(np.abs(ji[b, j, row, var] - side / t) <= 2.0 ** -51 / t), row
        assert np.all(ji[b, j, row, var - 11] == -ji[b, j, row, var])


def test_shape_every_pair_vs_numpy_checker(g16):
    """B = 3, N = 130: two blocks of 128 threads per instance, the wrap pair in the second; all 390 pairs at the older 1e-10."""
    from spline_trajectory_optimization_amd import ops
    args = _inputs(g16, "shape")
    assert args[8].shape == (3, 130)
    eq, g, cost = ops.dt_eval_nodes(MODEL, *args)
    oeq, og, ocost = dt.eval_nodes(MODEL, *args)
    scale = lambda r: np.maximum(1.0, np.abs(r))  # noqa: E731
    assert (np.abs(eq - oeq) / scale(oeq)).max() <= 1e-10
    assert (np.abs(g - og) / scale(og)).max() <= 1e-10
    np.testing.assert_allclose(cost, ocost, rtol=1e-12)


BK_ROWS = ("defect x", "defect y", "defect theta", "defect delta", "defect v", "longitudinal", "lateral", "traction")


@pytest.mark.parametrize("name", ["bk_sweep", "bk_general"])
def test_bicycle_eval_nodes_vs_50_digits(g16, name):
    from bicycle_problem import MODEL as BK_MODEL
    from spline_trajectory_optimization_amd import ops
    X, U, T = (g16[f"{name}_{k}"] for k in ("X", "U", "T"))
    eq, ineq, cost = ops.bicycle_eval_nodes(BK_MODEL, g16[f"{name}_P0"], g16[f"{name}_yaw"], X[None], U[None], T[None])
    got = np.concatenate([eq[0], ineq[0]], axis=1)
    ref, twin = g16[f"{name}_ref"], g16[f"{name}_twin"]
    assert np.isfinite(got).all()
    r, allow = hp.ratios(got, ref, twin, 0), hp.allowance(ref, twin, 0)
    print(f"[nlp_highprec {name}] " + "; ".join(f"{k}: ratio {r[i]:.2f} (yard {allow[i]:.1e})" for i, k in enumerate(BK_ROWS)))
    assert np.all(r <= FACTOR), r
    assert cost[0] == pytest.approx(T.sum(), rel=1e-14)
    if name == "bk_sweep":
        # m_sincos itself: here rows 0 / 1 are T v cos(theta') and T v sin(theta') of the SAME double theta' in the kernel and in
        # the float twin (theta / 3.14 * 3.14 rounds alike), so the two differ by the functions' roundings and the sum's alone --
        # a few units in the last place of the amplitude T v = 2
        ulps = np.abs(got[:, :2] - twin[:, :2]).max(axis=0) / (2.0 ** -52 * 2.0)
        print(f"[nlp_highprec bk_sweep] m_sincos against libm over 512 angles up to 4 pi: cos {ulps[0]:.2f}, sin {ulps[1]:.2f} "
              f"ulp of the amplitude")
        assert np.all(ulps <= FACTOR)
