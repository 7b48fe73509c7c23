"""Every branch of the global-QP dispatch (rl_mincurv_global_batch_host, rl_mincurv_global_weighted_batch_host) on the synthetic
closed splines of tests/global_shape_cases.py, against the CPU twin.  Needs a real MI355X:  pytest -m gpu -k global_shapes

Per case, as a batch of three width rows (x 1.0, x 0.8, x 1.0):
  * rl_stats.block_threads / lds_bytes are what the dispatch mirror predicts for the device's LDS size -- only then is the
    branch in the report the branch that ran;
  * offsets, line and control points within 1e-6 m of oracle.global_mincurv (the bound of
    test_global_qp.py::test_global_kernel_vs_twin; the twin's own strict-versus-FMA spread on these cases is <= 1e-11 m,
    tests/test_global_shapes_cpu.py), bound violation <= 1e-9 m, interior-point iterations within one of the twin's, sum kappa^2
    before / after to rel 1e-9 / 1e-7 -- instance 0 against the twin at x 1.0, instance 1 against the twin at x 0.8;
  * instances 0 and 2 are the same bits;
  * the weighted entry with w = 1 returns the unweighted bits.
Cases past a limit of the library are refused with its message, before anything runs.  n_p = 193 and 200 are such cases: both
kernels hold three rows of the triangular solves per lane, global_tables refuses n_p > 192, and the three generic templates
are reached by n_p <= 192 instead (np192_N3000 / N3500 / N5000; K = 5: N = 4736, the largest N whose 704-thread generic layout
fits 160 KiB -- N = 5000 is refused for LDS, and is a case too).

Then, once per kernel and degree, the weighted cost with w_i = 1 + 0.5 sin(0.05 i) against tests/weighted_global_twin.py at the
tolerances of tests/test_weighted_global_gpu.py; and the single-linearisation cases (n_p <= 66) through the certificate of
tests/kkt_certificate.py on the dense numpy statement of the QP (test_global_qp.py: NumpyGlobal), which shares no code with the
twin: 1e-9 m feasibility, 1e-6 |q|_inf stationarity, the bounds of test_twin_solves_the_qp_kkt."""
import functools
import os

import numpy as np
import pytest

import global_shape_cases as gc
import kkt_certificate as kc
import weighted_global_twin as tw
from oracle import oracle as orc
from test_global_qp import NumpyGlobal

pytestmark = pytest.mark.gpu
SCALES = (1.0, 0.8, 1.0)
OUT = ("ctrl", "xy", "a", "stats")


@pytest.fixture(scope="module")
def rl():
    import torch
    from spline_trajectory_optimization_amd import _lib, ops
    ctx = _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing
    old = os.environ.get("RL_GLOBAL_V1")
    os.environ["RL_GLOBAL_V1"] = "1"       # read once, in rl_ctx_create: a context of its own keeps the generic kernel
    try:
        v1 = _lib.Context(0)
    finally:
        if old is None:
            del os.environ["RL_GLOBAL_V1"]
        else:
            os.environ["RL_GLOBAL_V1"] = old
    p = torch.cuda.get_device_properties(0)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.ctx, ns.v1 = _lib, ops, ctx, v1
    # rl_ctx_create: the larger of sharedMemPerBlock and the opt-in maximum
    ns.max_lds = max(int(p.shared_memory_per_block), int(getattr(p, "shared_memory_per_block_optin", 0)))
    return ns


@functools.lru_cache(maxsize=None)
def twin(problem, scale):
    k, n_p, N, n_outer, seed = problem
    t, cx, cy = gc.closed_spline(k, n_p, seed)
    wl, wr = gc.half_widths(N, scale)
    return orc.global_mincurv(t, cx, cy, k, N, wl, wr, gc.MARGIN, n_outer)


def width_rows(N, scales):
    return np.ascontiguousarray(np.stack([np.stack(gc.half_widths(N, s), 1) for s in scales]))


def track(rl, case):
    t, cx, cy = case.spline()
    return rl.lib.Track(rl.v1 if case.force_v1 else rl.ctx, t, cx, cy, case.k, case.N)


def ran_as_predicted(rl, case, rs):
    d = case.dispatch(rl.max_lds)
    assert (rs.block_threads, rs.lds_bytes) == (d.block_threads, d.lds_bytes), (case.id, d, rs.block_threads, rs.lds_bytes)
    return d


def against_twin(tag, out, b, ref):
    """Instance b of out = (ctrl, xy, a, st, rs) against ref = (cx, cy, xy, a, stats) of a twin."""
    ctrl, xy, a, st, _ = out
    tcx, tcy, txy, ta, tst = ref
    da, dxy = np.abs(a[b] - ta).max(), np.abs(xy[b] - txy).max()
    dc = np.abs(ctrl[b] - np.stack([tcx, tcy], 1)).max()
    print(f"[global shapes {tag} #{b}] |da| {da:.2e} |dxy| {dxy:.2e} |dctrl| {dc:.2e} m  ipm {int(st[b, 0])}/{int(tst[0])}  "
          f"k2 {st[b, 1]:.6f}->{st[b, 2]:.6f}  viol {st[b, 3]:.1e}")
    assert np.isfinite(a[b]).all() and np.isfinite(xy[b]).all() and np.isfinite(ctrl[b]).all()
    assert da <= 1e-6 and dxy <= 1e-6 and dc <= 1e-6
    assert st[b, 3] <= 1e-9
    assert abs(int(st[b, 0]) - int(tst[0])) <= 1
    assert st[b, 1] == pytest.approx(tst[1], rel=1e-9) and st[b, 2] == pytest.approx(tst[2], rel=1e-7)


def test_the_device_has_the_lds_the_case_list_assumes(rl):
    """The branches named in the case list are those at 160 KiB; with another size the LDS-overflow cases move."""
    assert rl.max_lds == gc.LDS_160K


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_case_vs_twin(rl, case):
    d = case.dispatch(rl.max_lds)
    W = width_rows(case.N, SCALES)
    trk = track(rl, case)
    if d.family == "refused":
        for kw in (dict(), dict(weights=np.ones(case.N))):
            with pytest.raises(rl.lib.RlError, match=d.why):
                rl.ops.global_batch_host(trk, W, gc.MARGIN, case.n_outer, **kw)
        print(f"[global shapes {case.id}] n_p {case.n_p} N {case.N}: {d.branch}")
        return
    out = rl.ops.global_batch_host(trk, W, gc.MARGIN, case.n_outer)
    ran_as_predicted(rl, case, out[4])
    print(f"[global shapes {case.id}] n_p {case.n_p} N {case.N} outer {case.n_outer}: {d.branch}  block {d.block_threads} lds "
          f"{d.lds_bytes}  chunks {d.n_chunks} ({d.short_tails} spans with a short tail, {d.empty_spans} empty)  "
          f"{out[4].kernel_ms:.2f} ms")
    if rl.max_lds == gc.LDS_160K:
        assert d.branch == case.expect
    against_twin(case.id, out, 0, twin(case.problem, 1.0))
    against_twin(case.id, out, 1, twin(case.problem, 0.8))
    for q, name in enumerate(OUT):
        assert out[q][0].tobytes() == out[q][2].tobytes(), name              # the neighbour in the batch leaves no trace
    assert np.abs(out[2][1] - out[2][0]).max() > 1e-3                         # and instance 1 is another problem
    ones = rl.ops.global_batch_host(trk, W, gc.MARGIN, case.n_outer, weights=np.ones((3, case.N)))
    ran_as_predicted(rl, case, ones[4])
    for q, name in enumerate(OUT):
        assert ones[q].tobytes() == out[q].tobytes(), name


@pytest.mark.parametrize("cid", gc.WEIGHTED_VS_TWIN)
def test_weighted_case_vs_twin(rl, cid):
    case = gc.BY_ID[cid]
    t, cx, cy = case.spline()
    wl, wr = gc.half_widths(case.N)
    w = gc.weights_sine(case.N)
    out = rl.ops.global_batch_host(track(rl, case), width_rows(case.N, (1.0,)), gc.MARGIN, case.n_outer, weights=w)
    d = ran_as_predicted(rl, case, out[4])
    ref = tw.global_mincurv_weighted(t, cx, cy, case.k, case.N, wl, wr, gc.MARGIN, case.n_outer, weights=w)
    against_twin(f"weighted {cid} {d.branch}", out, 0, ref)
    assert out[3][0, 6] == 0.0 and out[3][0, 7] == 0.0
    assert np.abs(out[2][0] - twin(case.problem, 1.0)[3]).max() > 1e-3       # the weight did something


@pytest.mark.parametrize("cid", gc.CERTIFIED)
def test_single_linearisation_is_a_kkt_point_of_the_dense_statement(rl, cid):
    case = gc.BY_ID[cid]
    t, cx, cy = case.spline()
    wl, wr = gc.half_widths(case.N)
    _, _, a, st, rs = rl.ops.global_batch_host(track(rl, case), width_rows(case.N, (1.0,)), gc.MARGIN, 1)
    d = ran_as_predicted(rl, case, rs)
    ng = NumpyGlobal(t, cx, cy, case.k, np.arange(case.N) * (1.0 / case.N))
    P, q, A = ng.qp_at(np.zeros(ng.np))
    cert, bounds = kc.certify_qp(P, q, A, -(wr - gc.MARGIN), wl - gc.MARGIN, a[0])
    print(f"[global shapes kkt {cid} {d.branch}] stat {cert.stat:.2e} (<= {bounds[0]:.2e})  compl {cert.compl:.2e} "
          f"(<= {bounds[1]:.2e})  viol {cert.viol:.1e}  ipm {int(st[0, 0])}")
    assert cert.viol <= 1e-9 and cert.stat <= 1e-6 * np.abs(q).max() and cert.compl <= bounds[1]
    assert cert.viol <= st[0, 3] + 1e-9                                      # the kernel's own figure does not under-report
