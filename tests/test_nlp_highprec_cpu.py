"""Fixture G16 (tests/golden/G16_nlp_highprec.npz) and the generic model code behind it (tests/nlp_highprec.py), without a GPU:
the float instantiation against the G8-pinned numpy checker, the mpmath instantiation against fixture G8, the float dual against
the 50-digit differences, the conditions the input families must meet (coverage of every m_atan interval and m_sincos quadrant,
distance from the kinks), the generator's reproducibility, and the sensitivity of the tolerance rule the GPU tests apply
(tests/test_nlp_highprec_gpu.py): a slightly wrong atan constant and a dropped chain-rule term pass on the old `tame` inputs
and fail on `cornering`."""
import math
import os
import sys

import numpy as np
import pytest

import nlp_highprec as hp
from conftest import golden
from oracle import dt_checker as dt
from test_double_track import MODEL

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


@pytest.fixture(scope="module")
def g16():
    g = golden("G16_nlp_highprec.npz")
    return {k: g[k] for k in g.files}


def family(g16, name):
    keys = ("s", "kappa", "left", "right", "L", "margin", "X", "U", "T", "pairs")
    return {k: g16[f"{name}_{k}"] for k in keys}


def twin_rows(g16, name, math_ns=None, dual_ns=None):
    """The float twin (or a variant of it) on the stored pairs of a family: values [P,23], Jacobian [P,23,21]."""
    fam = family(g16, name)
    vals, jacs = [], []
    for b, j in fam["pairs"]:
        z, trk = hp.pair_inputs(fam, int(b), int(j))
        vals.append(hp.dt_float(MODEL, trk, z, math_ns=math_ns))
        jacs.append(hp.dt_dual(MODEL, trk, z, math_ns=dual_ns)[1])
    return np.array(vals), np.array(jacs)


@pytest.mark.parametrize("name", hp.DT_FAMILIES)
def test_float_twin_equals_the_numpy_checker(g16, name):
    """1e-13 relative to the largest term of the row's last subtraction (the states for a defect, P_max for the power row, the
    value itself elsewhere): the checker sums the same terms in the same order, the libraries' sin / atan may differ by an ulp.
    A row that an exactly stated family value makes 0 is compared absolutely: both must be exactly 0."""
    fam = family(g16, name)
    eq, g, _ = dt.eval_nodes(MODEL, fam["s"], fam["kappa"], fam["left"], fam["right"], float(fam["margin"]), float(fam["L"]),
                             fam["X"], fam["U"], fam["T"])
    N = fam["T"].shape[1]
    worst = 0.0
    for p, (b, j) in enumerate(fam["pairs"]):
        mine = g16[f"{name}_twin_val"][p]
        ref = np.concatenate([eq[b, j], g[b, j]])
        scale = np.abs(ref)
        scale[:6] = np.maximum(scale[:6], np.maximum(np.abs(fam["X"][b, j]), np.abs(fam["X"][b, (j + 1) % N])))
        scale[6] = max(scale[6], abs(fam["U"][b, j, 3])); scale[12] = max(scale[12], MODEL["Pmax"])
        dev = np.abs(mine[:22] - ref)
        assert np.all(dev[ref == 0.0] == 0.0)
        worst = max(worst, float((dev[ref != 0.0] / scale[ref != 0.0]).max()))
        su = np.array([MODEL["Fd_max"], abs(MODEL["Fb_max"]), MODEL["delta_max"], MODEL["mass"] * 50.0])
        Us, Uns = fam["U"][b, j] / su, fam["U"][b, (j + 1) % N] / su
        cost = fam["T"][b, j] + 1e-4 * (Uns ** 2).sum() + 1e-1 * ((Uns - Us) ** 2).sum()       # test_double_track._pair_cost
        assert abs(mine[22] - cost) <= 1e-13 * abs(cost)
    print(f"[nlp_highprec {name}] float twin vs numpy checker: worst relative deviation {worst:.2e}")
    assert worst <= 1e-13


def test_limits_family_rows_are_exactly_zero(g16):
    fam, val = family(g16, "limits"), g16["limits_twin_val"]
    ref = g16["limits_ref_val"]
    U0, dl, v = fam["U"][0, :, 0], fam["U"][0, :, 2], fam["X"][0, :, 5]
    for row, at in ((8 + 6, U0 == MODEL["Fb_max"]), (8 + 7, U0 == MODEL["Fd_max"]), (8 + 8, dl == -MODEL["delta_max"]),
                    (8 + 9, dl == MODEL["delta_max"]), (8 + 5, v == 1.0)):
        assert at.sum() >= 3
        assert np.all(val[at, row] == 0.0) and np.all(ref[at, row] == 0.0)
    assert (np.abs(U0) == 15000.0).sum() >= 6 and all(math.tanh(u) == math.copysign(1.0, u) for u in U0)
    # the rate rows: the upper side is the active one on half of the pairs, the lower on the rest
    T = fam["T"][0]
    ru = (np.roll(U0, -1) - U0) / T; rd = (np.roll(dl, -1) - dl) / T
    upper_u = ru - MODEL["Fd_max"] / MODEL["Td"] > MODEL["Fb_max"] / MODEL["Tb"] - ru
    upper_d = rd - MODEL["delta_max"] / MODEL["Tdelta"] > -MODEL["delta_max"] / MODEL["Tdelta"] - rd
    assert upper_u.sum() == upper_d.sum() == len(T) // 2


def test_mpmath_instantiation_reproduces_g8():
    """The 50-digit instantiation on fixture G8's point (the reference's own functions on numbers), to the tolerances of
    test_double_track.test_dt_eval_nodes_vs_reference_fixture."""
    pytest.importorskip("mpmath")
    g = golden("G8_double_track.npz")
    m = dict(zip(g["model_keys"].tolist(), g["model_vals"].tolist()))
    fam = dict(s=g["nlp_s"], kappa=g["nlp_kappa"], left=g["nlp_left"], right=g["nlp_right"], margin=float(g["nlp_margin"]),
               L=float(g["nlp_length"]), X=g["nlp_X"][None], U=g["nlp_U"][None], T=g["nlp_T"][None])
    M = hp.MpMath()
    rows = []
    for j in range(fam["T"].shape[1]):
        z, trk = hp.pair_inputs(fam, 0, j)
        rows.append(hp.dt_reference(M, m, trk, z, jac=False)[0][:, 0])
    rows = np.array(rows)
    np.testing.assert_allclose(rows[:, :8], g["nlp_eq"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(rows[:, 8:22], g["nlp_ineq"], rtol=1e-11, atol=1e-10)
    assert abs(rows[:, 22].sum() - float(g["nlp_cost"])) < 1e-11 * abs(float(g["nlp_cost"]))


@pytest.mark.parametrize("name", hp.DT_FAMILIES)
def test_float_dual_against_the_50_digit_differences(g16, name):
    """Two derivative computations that share no code: forward-mode duals in double, central differences at 50 digits.  The
    figure printed is the yardstick of the GPU test; the assertion only guards the reference against a gross mismatch (a term
    missing from either side is 1e-6 of a row's largest entry or more; rounding amplified by the rows' cancellation is far less)."""
    ref, twin = g16[f"{name}_ref_jac"], g16[f"{name}_twin_jac"]
    dev = hp.deviation(twin, ref).max(axis=(0, 2))
    big = np.abs(ref[..., 0]).max(axis=(0, 2))
    rel = np.where(big > 0, dev / np.where(big > 0, big, 1.0), dev)
    print(f"[nlp_highprec {name}] float dual vs 50-digit differences: worst |dev| / max|row| {rel.max():.2e} "
          f"(row {int(rel.argmax())}), worst absolute {dev.max():.2e}")
    assert np.isfinite(ref).all() and rel.max() <= 1e-9


def test_coverage_of_atan_intervals_and_sincos_quadrants(g16):
    kin = np.concatenate([g16[f"{f}_atan_kin"] for f in hp.DT_FAMILIES])
    pac = np.concatenate([g16[f"{f}_atan_pac"] for f in hp.DT_FAMILIES])
    ck, cp = hp.atan_coverage(kin), hp.atan_coverage(pac)
    sc = hp.sincos_coverage(np.concatenate([g16[f"{f}_sincos"].ravel() for f in hp.DT_FAMILIES + ("bk_sweep", "bk_general")]))
    print(f"[nlp_highprec] pairs per m_atan interval: kinematic {ck.tolist()}, Pacejka {cp.tolist()}; "
          f"m_sincos arguments per quadrant and sign {sc.tolist()}")
    assert ck.min() >= 3 and cp.min() >= 3 and sc.min() >= 3
    # what the old inputs reach (the reason for the new families): one atan interval at the kinematic sites
    assert hp.atan_coverage(g16["tame_atan_kin"])[1:].sum() == 0
    # blend: the tanh blend where it is not saturated, and at 0 exactly; wraps: d near +-4 pi, the fmod branch at interior pairs
    U0 = g16["blend_U"][0, :, 0]
    assert (np.abs(np.tanh(U0)) < 1.0).sum() >= 8 and (U0 == 0.0).sum() >= 1 and (np.abs(U0) == 1e-3).sum() == 2
    xi, s = g16["wraps_X"][0, :, 2], g16["wraps_X"][0, :, 0]
    turns = np.rint((np.roll(xi, -1) - xi)[:-1] / (2 * math.pi))
    assert set(turns.tolist()) >= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert (np.abs((s - np.roll(s, -1))[:-1]) > float(g16["wraps_L"]) / 2).sum() >= 8
    th = g16["bk_sweep_X"][:, 2]
    assert abs(th).max() <= 4 * math.pi + 1e-14 and all(np.sum(th == q) >= 1 for q in (1e-300, -1e-300, 2.0 ** -27, -2.0 ** -27))
    assert np.sum(th == 0.0) >= 2 and np.sum(np.signbit(th) & (th == 0.0)) == 1


@pytest.mark.parametrize("name", hp.DT_FAMILIES)
def test_distance_from_the_kinks(g16, name):
    """Every stored pair, and on `shape` every pair the kernel evaluates; no pair is left out (the generator draws a failing
    pair again)."""
    least = np.array(hp.KINK_MIN)
    assert np.all(g16[f"{name}_kinks"] >= least)
    assert np.all(hp.family_kinks(MODEL, family(g16, name)) >= least)
    if name == "shape":
        assert sorted(set(g16["shape_pairs"][:, 1].tolist())) == list(hp.SHAPE_PAIRS) and len(g16["shape_pairs"]) == 18
    else:
        assert len(g16[f"{name}_pairs"]) == 24


def test_bicycle_families_keep_off_the_yaw_kink(g16):
    for name in ("bk_sweep", "bk_general"):
        assert g16[f"{name}_yawdist"].min() >= 1e-3
        F = hp.FloatMath(record=True)
        fam = {k: g16[f"{name}_{k}"] for k in ("P0", "yaw", "X", "U", "T")}
        from bicycle_problem import MODEL as BK_MODEL
        assert np.array_equal(np.array(hp.bk_eval(F, BK_MODEL, fam)), g16[f"{name}_twin"])
    assert len(g16["bk_sweep_T"]) == 512 and len(g16["bk_general_T"]) == 24


def test_bicycle_float_twin_equals_bicycle_twin(g16):
    import bicycle_twin as bt
    from bicycle_problem import MODEL as BK_MODEL
    for name in ("bk_sweep", "bk_general"):
        fam = {k: g16[f"{name}_{k}"] for k in ("P0", "yaw", "X", "U", "T")}
        prob = bt.Problem(BK_MODEL, fam["P0"], fam["yaw"], np.ones(len(fam["T"])), -np.ones(len(fam["T"])))
        c, d = prob.funcs(prob.to_w(fam["X"], fam["U"], fam["T"]))
        ref = np.concatenate([c, d], axis=1)
        scale = np.maximum(1.0, np.abs(fam["X"]).max())
        assert np.abs(g16[f"{name}_twin"] - ref).max() <= 1e-13 * max(scale, np.abs(ref).max())


def test_inputs_are_what_the_generator_draws(g16):
    for name in hp.DT_FAMILIES:
        fam = hp.draw_dt_family(name, MODEL, int(g16[f"{name}_seed"]))
        for k, v in fam.items():
            assert np.array_equal(np.asarray(v), g16[f"{name}_{k}"]), (name, k)
    for k, v in hp.bk_sweep_family().items():
        assert np.array_equal(v, g16[f"bk_sweep_{k}"])
    # tame is random_problem's draw, untouched
    from test_double_track import random_problem
    s, kappa, left, right, L, X, U, T = random_problem(1, 24, seed=int(g16["tame_seed"]))
    assert np.array_equal(X, g16["tame_X"]) and np.array_equal(U, g16["tame_U"]) and np.array_equal(T, g16["tame_T"])


def test_generator_reproduces_the_fixture_bits(g16):
    """Two pairs of every family (and eight nodes of each bicycle family) through the committed generator's own functions."""
    pytest.importorskip("mpmath")
    import make_golden_nlp_highprec as gen
    from bicycle_problem import MODEL as BK_MODEL
    M = hp.MpMath()
    for name in hp.DT_FAMILIES:
        sel = [0, len(g16[f"{name}_pairs"]) - 1]
        for k, v in gen.dt_family_arrays(name, MODEL, family(g16, name), M, pairs=sel).items():
            assert np.array_equal(v, g16[k][sel]), k
    for name in ("bk_sweep", "bk_general"):
        fam = {k: g16[f"{name}_{k}"] for k in ("P0", "yaw", "X", "U", "T")}
        sel = [0, 3, 7, 11, 15, 19, 22, 23] if name == "bk_general" else [0, 100, 231, 233, 235, 300, 510, 511]
        for k, v in gen.bk_family_arrays(name, BK_MODEL, fam, M, nodes=sel).items():
            assert np.array_equal(v, g16[k][sel]), k


# ---- sensitivity of the tolerance rule: variants of the float twin judged as the GPU tests judge the kernels
_ATAN_HI = (0.0, 4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
_ATAN_LO = (0.0, 2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
       9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
       4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)


def _atan_by_intervals(x, hi=_ATAN_HI):
    """atan the way the device computes it (csrc/rl_dtrack.hpp: m_atan; s_atan.c's reduction and polynomial), in float."""
    ax = abs(x)
    i = hp.atan_interval(ax)
    num = (ax, 2.0 * ax - 1.0, ax - 1.0, ax - 1.5, -1.0)[i]
    den = (1.0, 2.0 + ax, ax + 1.0, 1.5 * ax + 1.0, ax)[i]
    t = num / den
    z = t * t
    w = z * z
    s1 = z * (_AT[0] + w * (_AT[2] + w * (_AT[4] + w * (_AT[6] + w * (_AT[8] + w * _AT[10])))))
    s2 = w * (_AT[1] + w * (_AT[3] + w * (_AT[5] + w * (_AT[7] + w * _AT[9]))))
    res = hi[i] - ((t * (s1 + s2) - _ATAN_LO[i]) - t)
    return -res if x < 0.0 else res


class _IntervalAtan(hp.FloatMath):
    """atan by intervals with the constants `hi`; with kinematic_only, at the kinematic call sites alone (the call sites
    announce themselves by the note that precedes them)."""

    def __init__(self, hi, kinematic_only=False):
        hp.FloatMath.__init__(self)
        self.hi, self.kinematic_only, self.site = hi, kinematic_only, None

    def note(self, key, x):
        if key.startswith("atan_"):
            self.site = key

    def atan(self, x):
        if self.kinematic_only and self.site != "atan_kin":
            return math.atan(x)
        return _atan_by_intervals(x, self.hi)


class _DroppedChainTerm(hp.DualMath):
    """atan in its last interval is pi/2 - atan(1/x); its derivative by the chain rule is (1/x^2) * 1/(1 + 1/x^2).  This
    variant drops the second factor there."""
    @staticmethod
    def atan(x):
        outer = abs(x.v) >= hp.ATAN_BREAKS[3]
        return x.chain(math.atan(x.v), 1.0 / (x.v * x.v) if outer else 1.0 / (1.0 + x.v * x.v))


def _passes(g16, name, vals=None, jacs=None):
    ok = True
    if vals is not None:
        ok &= bool(np.all(hp.ratios(vals, g16[f"{name}_ref_val"], g16[f"{name}_twin_val"], 0) <= hp.MARGIN_BITS))
    if jacs is not None:
        ok &= bool(np.all(hp.ratios(jacs, g16[f"{name}_ref_jac"], g16[f"{name}_twin_jac"], (0, 2)) <= hp.MARGIN_BITS))
    return ok


def test_tolerance_rule_accepts_the_twin_and_a_sound_atan_by_intervals(g16):
    for name in hp.DT_FAMILIES:
        vals, jacs = twin_rows(g16, name)
        assert np.array_equal(vals, g16[f"{name}_twin_val"]) and np.array_equal(jacs, g16[f"{name}_twin_jac"])
        r = hp.ratios(twin_rows(g16, name, math_ns=_IntervalAtan(_ATAN_HI))[0], g16[f"{name}_ref_val"], g16[f"{name}_twin_val"], 0)
        print(f"[nlp_highprec {name}] atan by intervals (1 ulp) in the float twin: worst ratio per row group {hp.group_worst(r)}")
        assert r.max() <= hp.MARGIN_BITS


def test_a_wrong_atan_constant_in_the_third_interval_is_caught_on_cornering_only(g16):
    """hi of the third interval, atan(1) = 0.785398163397448279, with its last digits changed (+1e-12).  `tame` never enters
    that interval at a kinematic call site, so the constant wrong THERE goes unseen on it; random_problem's draw does reach it
    at the Pacejka sites in a few pairs (Bf * slip ~ 0.7), where the old tests' 1e-10 relative still hides the 1e-12.  On
    `cornering` the rule catches the constant at either kind of site."""
    bad = list(_ATAN_HI); bad[2] = 7.85398163398448e-01
    assert hp.atan_coverage(g16["tame_atan_kin"])[2] == 0 and hp.atan_coverage(g16["cornering_atan_kin"])[2] >= 3
    assert _passes(g16, "tame", vals=twin_rows(g16, "tame", math_ns=_IntervalAtan(bad, kinematic_only=True))[0])
    assert not _passes(g16, "cornering", vals=twin_rows(g16, "cornering", math_ns=_IntervalAtan(bad, kinematic_only=True))[0])
    assert not _passes(g16, "cornering", vals=twin_rows(g16, "cornering", math_ns=_IntervalAtan(bad))[0])
    # what the old test asks (1e-10 relative, the scale floored at 1) lets the wrong constant through on `tame` at every site
    vals, ref = twin_rows(g16, "tame", math_ns=_IntervalAtan(bad))[0], g16["tame_twin_val"]
    assert (np.abs(vals - ref)[:, :22] / np.maximum(1.0, np.abs(ref[:, :22]))).max() <= 1e-10


def test_a_dropped_chain_rule_term_is_caught_on_cornering_only(g16):
    assert hp.atan_coverage(np.concatenate([g16["tame_atan_kin"], g16["tame_atan_pac"]], axis=1))[4] == 0
    assert _passes(g16, "tame", jacs=twin_rows(g16, "tame", dual_ns=_DroppedChainTerm())[1])
    jac = twin_rows(g16, "cornering", dual_ns=_DroppedChainTerm())[1]
    assert not _passes(g16, "cornering", jacs=jac)
