"""The synthetic family of tests/global_shape_cases.py, without a GPU: the case list reaches every branch of the global-QP
dispatch, and the CPU twin is well enough conditioned on every case for the 1e-6 m kernel-versus-twin bound of
tests/test_global_shapes_gpu.py to mean something.

Measured here (margin 0.25, all 77 runnable cases, both width scalings of the GPU test's batch): the twin leaves every
linearisation by its exit rule, 11 to 76 interior-point iterations in all per case; its strict and FMA-contracted builds agree
to <= 1e-11 m (offsets and line) on every case."""
import functools

import numpy as np
import pytest

import global_shape_cases as gc
import kkt_certificate as kc
import weighted_global_twin as tw
from oracle import oracle as orc
from test_global_qp import NumpyGlobal

SCALES = (1.0, 0.8)          # the width rows of the GPU test's batch


def test_the_case_list_reaches_every_branch():
    """Case by case the mirror gives the branch the case is there for; together they give all of BRANCHES_160K and nothing
    else: per degree the five fast instantiations (R5G1, R6G1, R10G1, R5G3, R6G3) and the three generic templates -- sixteen
    kernels, each weighted and unweighted in the GPU test -- the generic ones by each of the reasons that lead there (R = 10 with
    three groups, chunks beyond seven row waves, LDS overflow of the fast layout, forced), and the two refusals."""
    got = set()
    for c in gc.CASES:
        d = c.dispatch()
        assert d.branch == c.expect, (c.id, d)
        got.add((c.k, d.branch))
    assert got == gc.BRANCHES_160K, (got - gc.BRANCHES_160K, gc.BRANCHES_160K - got)
    kernels = {(k, b.split()[1]) for k, b in got if not b.startswith("refused")}
    assert len(kernels) == 16, sorted(kernels)
    reasons = {b.split()[2] for _, b in got if b.startswith("qp <")}
    assert reasons == {"r10_g3", "chunks", "lds", "forced"}
    assert len({c.id for c in gc.CASES}) == len(gc.CASES)
    assert set(gc.WEIGHTED_VS_TWIN) <= set(gc.BY_ID) and set(gc.CERTIFIED) <= set(gc.BY_ID)
    # the weighted comparison runs once per kernel, the certificate on every small single-linearisation case
    assert {(gc.BY_ID[i].k, gc.BY_ID[i].expect.split()[1]) for i in gc.WEIGHTED_VS_TWIN} == kernels
    assert all(gc.BY_ID[i].n_p <= 66 for i in gc.CERTIFIED) and len(gc.CERTIFIED) == 14


def test_the_switch_points_are_where_the_cases_put_them():
    D = {c.id: c.dispatch() for c in gc.CASES}
    for k in (3, 5):
        assert D[f"k{k}-np64_N2239"].n_chunks == 448 and D[f"k{k}-np64_N2241"].n_chunks < 448      # 449 chunks of 5 -> R = 6
        t = gc.closed_spline(k, 64)[0]
        assert gc.n_chunks(gc.rows_per_span(t, k, 2241), 5) == 449
        assert gc.n_chunks(gc.rows_per_span(t, k, 2700), 6) > 448                                   # -> R = 10
        assert D[f"k{k}-np64_N500"].G == 1 and D[f"k{k}-np65_N500"].G == 3
        assert D[f"k{k}-np192_N2000"].family == "qp2" and D[f"k{k}-np193_N2000"].family == "refused"
        fronts = lambda n_p: (n_p - 4 * k) // 2 if n_p > 4 * k else 0          # noqa: E731  (rl_global2.hpp: TwoFront<2k>::fronts)
        assert [fronts(gc.BY_ID[f"k{k}-{name}"].n_p) for name in ("np_min_N100", "np_4k_N201", "np_4k1_N333", "np_4k2_N333")] == [0, 0, 0, 1]
        for n_p, N in ((40, 97), (64, 131), (90, 181)):
            d = D[f"k{k}-uneven_np{n_p}_N{N}"]
            assert 2 <= d.empty_spans <= 5 and d.short_tails > 0, d
            rows = gc.rows_per_span(gc.BY_ID[f"k{k}-uneven_np{n_p}_N{N}"].spline()[0], k, N)
            assert rows.max() > 10 and rows.max() % 5 != 0           # the fat span: full chunks and a short tail
    # K = 5, n_p = 192, N = 2303: the fast layout is the one that overflows, by 416 B
    t = gc.closed_spline(5, 192)[0]
    assert 8 * gc.global2_layout_doubles(5, 197, 192, 2303, 3, 384) == 164256 == gc.LDS_160K + 416
    assert gc.dispatch(t, 5, 2303, max_lds=164256).branch == "qp2 R6G3"
    rows64 = gc.rows_per_span(gc.BY_ID["k5-uneven_np64_N131"].spline()[0], 5, 131)
    assert ((rows64[:-1] == 0) & (rows64[1:] == 0)).any()           # two empty spans in a row


def test_the_spline_is_closed_and_periodic():
    from scipy.interpolate import BSpline
    for k, n_p, seed in ((3, 8, None), (5, 21, None), (5, 64, 12), (3, 90, 13)):
        t, cx, cy = gc.closed_spline(k, n_p, seed)
        assert len(t) == n_p + 2 * k + 1 and len(cx) == n_p + k
        assert np.array_equal(cx[n_p:], cx[:k]) and np.array_equal(cy[n_p:], cy[:k])
        assert t[k] == 0.0 and t[k + n_p] == 1.0
        assert np.allclose(np.diff(t)[:k], np.diff(t)[n_p:n_p + k], rtol=0, atol=1e-15)
        for der in range(k):                                         # C^(k-1) across the seam
            for c in (cx, cy):
                s = BSpline(t, c, k)
                assert s(0.0, der) == pytest.approx(s(1.0 - 1e-13, der), rel=1e-6, abs=1e-6 * 100.0 * (2 * np.pi * n_p) ** der)


@functools.lru_cache(maxsize=None)
def twin(problem, scale, fma=False):
    k, n_p, N, n_outer, seed = problem
    t, cx, cy = gc.closed_spline(k, n_p, seed)
    wl, wr = gc.half_widths(N, scale)
    if fma:
        with orc.fma_variant():
            return orc.global_mincurv(t, cx, cy, k, N, wl, wr, gc.MARGIN, n_outer)
    return orc.global_mincurv(t, cx, cy, k, N, wl, wr, gc.MARGIN, n_outer)


def iterations_per_linearisation(problem, scale):
    """The twin reports the total; the runs with 1 .. n_outer linearisations are prefixes of one another."""
    k, n_p, N, n_outer, seed = problem
    tot = [0] + [int(twin((k, n_p, N, m, seed), scale)[4][0]) for m in range(1, n_outer + 1)]
    return np.diff(tot)


@pytest.mark.parametrize("case", [c for c in gc.RUNNABLE if not c.force_v1], ids=lambda c: c.id)
def test_twin_is_well_conditioned_on_the_case(case):
    for scale in SCALES:
        cx, cy, xy, a, st = twin(case.problem, scale)
        assert np.isfinite(cx).all() and np.isfinite(cy).all() and np.isfinite(xy).all() and np.isfinite(a).all() and np.isfinite(st).all()
        it = iterations_per_linearisation(case.problem, scale)
        assert it.sum() == int(st[0]) and (it > 0).all() and (it < 80).all(), it
        assert st[3] <= 1e-9 and st[2] < st[1]
        fcx, fcy, fxy, fa, fst = twin(case.problem, scale, fma=True)
        da, dxy = np.abs(a - fa).max(), np.abs(xy - fxy).max()
        print(f"[global shapes twin {case.id} x{scale}] ipm {it.tolist()}  strict-vs-FMA |da| {da:.1e} |dxy| {dxy:.1e} m  "
              f"k2 {st[1]:.5f}->{st[2]:.5f}  active {int(st[5])}")
        assert da <= 1e-9 and dxy <= 1e-9
        assert abs(int(st[0]) - int(fst[0])) <= 1


@pytest.mark.parametrize("cid", [i for i in gc.WEIGHTED_VS_TWIN if not gc.BY_ID[i].force_v1])
def test_weighted_twin_is_the_oracle_at_unit_weights(cid):
    """The numpy twin the weighted GPU cases are held to, pinned to the oracle on these shapes: 1e-8 m, the bound of
    tests/test_weighted_global_cpu.py (measured: <= 2.3e-11 m, equal iteration counts)."""
    c = gc.BY_ID[cid]
    t, cx, cy = c.spline()
    wl, wr = gc.half_widths(c.N)
    _, _, xy, a, st = tw.global_mincurv_weighted(t, cx, cy, c.k, c.N, wl, wr, gc.MARGIN, c.n_outer)
    _, _, oxy, oa, ost = twin(c.problem, 1.0)
    print(f"[global shapes weighted twin {cid}] |da| {np.abs(a - oa).max():.1e} |dxy| {np.abs(xy - oxy).max():.1e} m  "
          f"ipm {int(st[0])}/{int(ost[0])}")
    assert np.abs(a - oa).max() <= 1e-8 and np.abs(xy - oxy).max() <= 1e-8 and int(st[0]) == int(ost[0])


@pytest.mark.parametrize("cid", gc.CERTIFIED)
def test_twin_is_a_kkt_point_of_the_dense_statement(cid):
    """What the GPU test asks of the kernel on these cases, asked of the twin: the certificate's bounds can be met here."""
    c = gc.BY_ID[cid]
    t, cx, cy = c.spline()
    wl, wr = gc.half_widths(c.N)
    a = twin(c.problem, 1.0)[3]
    ng = NumpyGlobal(t, cx, cy, c.k, np.arange(c.N) * (1.0 / c.N))
    P, q, A = ng.qp_at(np.zeros(ng.np))
    cert, bounds = kc.certify_qp(P, q, A, -(wr - gc.MARGIN), wl - gc.MARGIN, a)
    print(f"[global shapes kkt twin {cid}] stat {cert.stat:.2e} (<= {bounds[0]:.2e})  compl {cert.compl:.2e} (<= {bounds[1]:.2e})  "
          f"viol {cert.viol:.1e}")
    assert cert.viol <= 1e-9 and cert.stat <= 1e-6 * np.abs(q).max() and cert.compl <= bounds[1]
