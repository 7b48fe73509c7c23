"""rl_tables_batch_* / rl_table_summary_* / batch.lap_times_* on the device against the CPU twin (tests/tables_twin.py: the
oracle's sample_along + fill_bounds, pinned to the reference's fixtures in tests/test_tables_cpu.py).

Tolerances are those of the single-instance kernels (tests/test_hip_parity.py::test_sample_along_golden, ::test_fill_bounds):
X, Y and the bound columns 1e-10 m, YAW 1e-13, DIST 1e-9 m against the oracle (GK21 like the kernel); IDX, ITERATION_FLAG, BANK
and the zero columns exactly.  CURVATURE (the turn radius) 1e-10 relative on the unperturbed centre-line fit.  On solved (and
on perturbed) lines that rule is not reachable by construction -- near-straight stretches and inflections have radii of 1e5 m
and more, where the oracle's own strict and FMA-contracted builds differ by 9e-11 relative -- so there the column is compared as
curvature 1 / radius, absolute, with tolerance 100 x max(spread of the oracle's two builds on the same control points,
1.14e-15 1/m)."""
import numpy as np
import pytest
from scipy.interpolate import CubicSpline

import tables_twin as tw
from conftest import golden, spline
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KAPPA_FLOOR = 1.14e-15   # 1/m: strict vs FMA build of the oracle on the benchmarked batch's first 16 instances


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    ctx = _lib.Context.get(0)
    ctx.set_arith(_lib.ARITH_DEFAULT)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch, ns.ctx = _lib, ops, batch, ctx
    yield ns
    ctx.set_option("tables_search", _lib.SEARCH_WINDOWED)
    ctx.set_option("tables_rings", 0)


def vehicle():
    g = golden("G6_simulator.npz")
    acc = CubicSpline(g["acc_lookup"][:, 0], g["acc_lookup"][:, 1])
    dcc = CubicSpline(g["dcc_lookup"][:, 0], g["dcc_lookup"][:, 1])
    return (acc.x, acc.c, dcc.x, dcc.c, g["params"])


def kappa_tolerance(strict, fma):
    spread = float(np.abs(1.0 / strict[..., tw.CURV] - 1.0 / fma[..., tw.CURV]).max())
    return 100.0 * max(spread, KAPPA_FLOOR), spread


def check(tag, pts, ref, kappa_tol=None, dist_atol=1e-9):
    """Every column of pts [.., N, 19] against the twin; prints each figure before it asserts."""
    d = lambda cols: float(np.abs(pts[..., cols] - ref[..., cols]).max())  # noqa: E731
    rel = float(np.abs(pts[..., tw.CURV] / ref[..., tw.CURV] - 1.0).max())
    kap = float(np.abs(1.0 / pts[..., tw.CURV] - 1.0 / ref[..., tw.CURV]).max())
    print(f"[tables {tag}] xy {d([0, 1]):.2e} m  yaw {d([3]):.2e}  radius rel {rel:.2e}  kappa {kap:.2e} 1/m"
          f" (tol {kappa_tol if kappa_tol is not None else 'rel 1e-10'})  dist {d([6, 7]):.2e} m  bounds {d(tw.BOUND_COLS):.2e} m")
    assert d([0, 1]) <= 1e-10 and d([3]) <= 1e-13
    if kappa_tol is None:
        assert rel <= 1e-10
    else:
        assert kap <= kappa_tol
    assert d([6, 7]) <= dist_atol
    assert d(tw.BOUND_COLS) <= 1e-10
    for c in (tw.IDX, tw.FLAG, tw.BANK) + tuple(tw.ZERO_COLS):
        np.testing.assert_array_equal(pts[..., c], ref[..., c])
    return kap


@pytest.mark.parametrize("N", [500, 2000])
def test_shared_rings_every_column(rl, fits, rings, N):
    t, cx, cy, k, length = spline(fits, "c100")
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    trk.set_rings(*rings)
    scx, scy, _, _, _ = rl.ops.mincurv_sweep(trk, cx, cy, rl.batch.default_i_start(len(cx), k, 2, seed=0), want_points=False)
    rng = np.random.default_rng(7)
    ctrl = np.stack([np.stack([cx, cy], 1), np.stack([scx, scy], 1),
                     np.stack([cx, cy], 1) + rng.uniform(-0.5, 0.5, size=(len(cx), 2))])
    ctrl[2, -k:] = ctrl[2, :k]                      # the periodic wrap of the reference's splines
    ctrl = np.ascontiguousarray(ctrl)
    pts = rl.ops.tables_host(trk, ctrl, rl.lib.BOUNDS_SHARED_RINGS, None, length)
    ref = tw.tables(t, k, N, ctrl, rings, length)
    with orc.fma_variant():
        fma = tw.tables(t, k, N, ctrl, rings, length)
    check(f"shared N={N} fit", pts[0], ref[0])
    for b, name in ((1, "solved"), (2, "perturbed")):
        tol, spread = kappa_tolerance(ref[b], fma[b])
        check(f"shared N={N} {name} (spread {spread:.2e})", pts[b], ref[b], kappa_tol=tol)
    # the unperturbed instance against the reference's own fixtures
    g = golden("G2_sample_along.npz")[f"N{N}_cols"]
    np.testing.assert_allclose(pts[0][:, [0, 1]], g[:, :2], rtol=0, atol=1e-10)
    np.testing.assert_allclose(pts[0][:, 3], g[:, 2], rtol=0, atol=1e-13)
    np.testing.assert_allclose(pts[0][:, 5], g[:, 3], rtol=1e-10)
    atol = 1e-9 if N >= 2000 else 1e-7
    np.testing.assert_allclose(pts[0][:, 6], g[:, 4], rtol=0, atol=atol)
    np.testing.assert_allclose(pts[0][:, 7], g[:, 5], rtol=0, atol=atol)
    if N == 500:
        np.testing.assert_allclose(pts[0][:, 9:13], golden("G4_track_constraint.npz")["c100_N500_bounds"], rtol=0, atol=1e-10)


def test_shared_rings_degree_3(rl, fits, rings):
    """k = 3: the left-boundary fit sampled every 2 m is the ring fixture itself (test_sample_along_k3_interval).  A boundary
    fit is not the centre-line fit the 1e-10 relative radius rule was made on (a cubic's second derivative is piecewise linear
    and crosses zero on the straights, where the radius is unbounded): the column is held to the curvature rule of the module
    docstring, from the oracle's own two builds.  Measured: 6.6e-15 1/m (1.2e-10 relative on the radius)."""
    t, cx, cy, k, length = spline(fits, "l10")
    N = int(length // 2.0)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    trk.set_rings(*rings)
    ctrl = np.ascontiguousarray(np.stack([cx, cy], 1)[None])
    pts = rl.ops.tables_host(trk, ctrl, rl.lib.BOUNDS_SHARED_RINGS, None, length)
    assert pts.shape[1] == rings[0].shape[0]
    np.testing.assert_allclose(pts[0][:, :2], rings[0], rtol=0, atol=1e-10)
    ref = tw.tables(t, k, N, ctrl, rings, length)
    with orc.fma_variant():
        tol, spread = kappa_tolerance(ref, tw.tables(t, k, N, ctrl, rings, length))
    check(f"shared k=3 (spread {spread:.2e})", pts, ref, kappa_tol=tol)


@pytest.fixture(scope="module")
def monza16(rl, fits, rings):
    """The first 16 instances of the benchmarked batch (Monza, N = 2000, widths of batch.width_batch(seed=1234)), solved with
    the default arithmetic; their tables on the device and from the twin's two builds."""
    t, cx, cy, k, length = spline(fits, "c100")
    N = 2000
    base = tw.table(t, cx, cy, k, length, N, rings[0], rings[1])
    wl, wr = rl.batch.half_widths_from_bounds(base)
    widths = np.ascontiguousarray(rl.batch.width_batch(wl, wr, 1024, seed=1234)[:16])
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    ctrl, _, _, _, _ = rl.ops.solve_batch_host(trk, rl.lib.BOUNDS_WIDTHS, widths, rl.batch.default_i_start(len(cx), 5, 5, seed=0))
    ctrl = np.ascontiguousarray(ctrl)
    ring_list = [tw.width_rings(t, cx, cy, k, N, widths[b]) for b in range(16)]
    ref = tw.tables(t, k, N, ctrl, ring_list, length)
    with orc.fma_variant():
        fma = tw.tables(t, k, N, ctrl, [tw.width_rings(t, cx, cy, k, N, widths[b]) for b in range(16)], length)
    pts = rl.ops.tables_host(trk, ctrl, rl.lib.BOUNDS_WIDTHS, widths, length)
    return dict(t=t, cx=cx, cy=cy, k=k, length=length, N=N, widths=widths, trk=trk, ctrl=ctrl, ref=ref, fma=fma, pts=pts)


def test_widths_benchmarked_batch_every_column(rl, monza16):
    m = monza16
    cond = float(np.abs(m["ref"][..., tw.BOUND_COLS] - m["fma"][..., tw.BOUND_COLS]).max())
    print(f"[tables widths] twin strict vs FMA on the bound columns: {cond:.2e} m")
    assert cond <= 1e-11, "the input is ill-conditioned for fill_bounds (closest-crossing tie): not a kernel finding"
    tol, spread = kappa_tolerance(m["ref"], m["fma"])
    kap = check(f"widths B=16 N=2000 (spread {spread:.2e})", m["pts"], m["ref"], kappa_tol=tol)
    print(f"[tables widths] kappa deviation / spread = {kap / max(spread, KAPPA_FLOOR):.1f}")


def test_points_form_is_bit_identical(rl, monza16):
    """The rings the width form builds, passed as points.  The default arithmetic builds them as the oracle's build with the
    correctly rounded cos / sin does (the reference-order sweep's rings)."""
    m = monza16
    with orc.cr_variant():
        rg = [tw.width_rings(m["t"], m["cx"], m["cy"], m["k"], m["N"], m["widths"][b]) for b in range(16)]
    bounds = np.ascontiguousarray(np.stack([np.concatenate([rl_, rr_], 1) for rl_, rr_ in rg]))
    pts = rl.ops.tables_host(m["trk"], m["ctrl"], rl.lib.BOUNDS_POINTS, bounds, m["length"])
    np.testing.assert_array_equal(pts, m["pts"])


def test_invariances_bitwise(rl, monza16):
    import torch
    m = monza16
    lib, ops, trk = rl.lib, rl.ops, m["trk"]
    W = lib.BOUNDS_WIDTHS
    for b in (0, 7, 15):   # instance b of the batch == the same instance alone
        one = ops.tables_host(trk, m["ctrl"][b:b + 1].copy(), W, m["widths"][b:b + 1].copy(), m["length"])
        np.testing.assert_array_equal(one[0], m["pts"][b])
    try:
        for mode in (lib.SEARCH_BRUTE, lib.SEARCH_CULLED):
            rl.ctx.set_option("tables_search", mode)
            np.testing.assert_array_equal(ops.tables_host(trk, m["ctrl"], W, m["widths"], m["length"]), m["pts"])
        rl.ctx.set_option("tables_search", lib.SEARCH_WINDOWED)
        rl.ctx.set_option("tables_rings", 1)      # ring vertices in the arena instead of LDS
        np.testing.assert_array_equal(ops.tables_host(trk, m["ctrl"], W, m["widths"], m["length"]), m["pts"])
    finally:
        rl.ctx.set_option("tables_search", lib.SEARCH_WINDOWED)
        rl.ctx.set_option("tables_rings", 0)
    dev = torch.device("cuda", 0)
    ctrl_d, w_d = torch.from_numpy(m["ctrl"]).to(dev), torch.from_numpy(m["widths"]).to(dev)
    out = torch.empty((16, m["N"], 19), dtype=torch.float64, device=dev)
    ops.tables_torch(trk, ctrl_d, W, w_d, m["length"], out=out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), m["pts"])
    # a repeated call of the same shape allocates nothing: free device memory (hipMemGetInfo) before and after.  The figure is
    # device wide, so another process may move it: an allocation of ours would show on every attempt.
    seen = []
    for _ in range(3):
        free0 = torch.cuda.mem_get_info(dev)[0]
        ops.tables_torch(trk, ctrl_d, W, w_d, m["length"], out=out)
        ops.tables_host(trk, m["ctrl"], W, m["widths"], m["length"])
        torch.cuda.synchronize()
        seen.append(free0 - torch.cuda.mem_get_info(dev)[0])
    print(f"[tables] free-memory change over a repeated call: {seen} B")
    assert min(seen) <= 0


def test_edge_cases(rl, fits, rings):
    lib, ops = rl.lib, rl.ops
    t, cx, cy, k, length = spline(fits, "c100")
    c0 = np.stack([cx, cy], 1)
    # length <= 0 leaves the DIST columns 0; bank [N] and [B,N]; B = 1 and B = 5; N = 58 (a sparse sampling, tests/sparse_cases.py)
    N = 58
    trk = lib.Track(rl.ctx, t, cx, cy, k, N)
    base = tw.table(t, cx, cy, k, length, N, rings[0], rings[1])
    wl, wr = rl.batch.half_widths_from_bounds(base)
    rng = np.random.default_rng(11)
    for B in (1, 5):
        widths = np.ascontiguousarray(rl.batch.width_batch(wl, wr, B, seed=5))
        ctrl = np.repeat(c0[None], B, 0) + rng.uniform(-0.05, 0.05, size=(B, len(cx), 2))
        ctrl[:, -k:] = ctrl[:, :k]
        ctrl = np.ascontiguousarray(ctrl)
        ring_list = [tw.width_rings(t, cx, cy, k, N, widths[b]) for b in range(B)]
        bank1 = np.linspace(-0.1, 0.2, N)
        bankB = np.ascontiguousarray(rng.uniform(-0.2, 0.2, size=(B, N)))
        with orc.fma_variant():
            fma = tw.tables(t, k, N, ctrl, [tw.width_rings(t, cx, cy, k, N, widths[b]) for b in range(B)], length)
        for bank, L in ((None, length), (bank1, 0.0), (bankB, -1.0), (bankB, length)):
            pts = ops.tables_host(trk, ctrl, lib.BOUNDS_WIDTHS, widths, L, bank=bank)
            ref = tw.tables(t, k, N, ctrl, ring_list, L, bank=bank)
            tol, _ = kappa_tolerance(ref, fma)
            check(f"N=58 B={B} length={L:g} bank={'none' if bank is None else bank.shape}", pts, ref, kappa_tol=tol)
            if not L > 0:
                assert not pts[..., [6, 7]].any()
    # a ring the normals miss keeps the point itself as bound: test_fill_bounds_no_hit_and_far_ring's square, moved onto the
    # first sample so that some normals hit it and most are more than 100 m away
    N = 500
    trk = lib.Track(rl.ctx, t, cx, cy, k, N)
    sq = np.array([[-10.0, -3.0], [10.0, -3.0], [10.0, 4.0], [-10.0, 4.0]]) + base[0, :2]
    trk.set_rings(sq, sq)
    ctrl = np.ascontiguousarray(np.stack([c0, c0 + 0.01]))
    pts = ops.tables_host(trk, ctrl, lib.BOUNDS_SHARED_RINGS, None, length)
    ref = tw.tables(t, k, N, ctrl, (sq, sq), length)
    with orc.fma_variant():
        tol, _ = kappa_tolerance(ref, tw.tables(t, k, N, ctrl, (sq, sq), length))
    check("square ring, fit", pts[0], ref[0])
    check("square ring, shifted", pts[1], ref[1], kappa_tol=tol)
    miss = np.all(ref[..., 9:13] == ref[..., [0, 1, 0, 1]], axis=-1)
    assert miss.sum() > N and (~miss).sum() > 0
    np.testing.assert_array_equal(pts[..., 9:13][miss], pts[..., [0, 1, 0, 1]][miss])
    # argument errors
    with pytest.raises(lib.RlError):
        ops.tables_host(lib.Track(rl.ctx, t, cx, cy, k, N), ctrl, lib.BOUNDS_SHARED_RINGS, None, length)   # no rings attached


def test_chain_lap_times(rl, monza16):
    import torch
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    from spline_trajectory_optimization_amd.simulator.simulator import Simulator
    m = monza16
    veh = vehicle()
    dev = torch.device("cuda", 0)
    ctrl_d, w_d = torch.from_numpy(m["ctrl"]).to(dev), torch.from_numpy(m["widths"]).to(dev)
    out = rl.batch.lap_times_torch(m["trk"], ctrl_d, rl.lib.BOUNDS_WIDTHS, w_d, m["length"], veh)
    torch.cuda.synchronize()
    pts, iters, summ = out["points"].cpu().numpy(), out["iters"].cpu().numpy(), out["summary"].cpu().numpy()
    assert np.all(iters > 0)
    for b in range(16):
        ref, oit = orc.qss_sim(m["pts"][b], *veh)        # the simulator's checker on the table the GPU built
        assert iters[b] == oit
        np.testing.assert_array_equal(pts[b][:, 18], ref[:, 18])
        dv = np.abs(pts[b][:, [4, 14, 15, 16]] - ref[:, [4, 14, 15, 16]]).max(axis=0)
        if b == 0:
            print(f"[tables chain] instance 0: |d| speed {dv[0]:.2e} lon {dv[1]:.2e} lat {dv[2]:.2e} time {dv[3]:.2e}")
        np.testing.assert_allclose(pts[b][:, [4, 14, 15, 16]], ref[:, [4, 14, 15, 16]], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(summ[b], tw.summary(pts[b]))   # ordered sum and extrema: bitwise
        assert summ[b, 0] == np.cumsum(pts[b][:, 16])[-1]
    print(f"[tables chain] lap times of the 16 instances: {summ[:, 0].min():.3f} .. {summ[:, 0].max():.3f} s")
    host = rl.batch.lap_times_host(m["trk"], m["ctrl"], rl.lib.BOUNDS_WIDTHS, m["widths"], m["length"], veh)
    np.testing.assert_array_equal(host["summary"], summ)
    np.testing.assert_array_equal(rl.ops.table_summary(pts, iters), summ)
    # an instance the reference would have raised on: a zero turn radius makes a seed speed zero
    bad = m["pts"][:3].copy()
    bad[1, 100, 5] = 0.0
    sim = Simulator(Vehicle(VehicleParams(golden("G6_simulator.npz")["acc_lookup"], golden("G6_simulator.npz")["dcc_lookup"],
                                          *[float(v) for v in veh[4]])))
    sp, it = rl.ops.qss_sim(bad, *veh)
    assert it[1] < 0 and it[0] > 0 and it[2] > 0
    s3 = rl.ops.table_summary(sp, it)
    assert np.isnan(s3[1]).all() and np.isfinite(s3[[0, 2]]).all()
    with pytest.raises(FloatingPointError, match="instance 1"):
        sim.run_simulation_batch(bad)
    res = sim.run_simulation_batch(np.ascontiguousarray(m["pts"][:2]))
    assert len(res) == 2 and res[0].total_time == summ[0, 1] and res[1].max_speed == summ[1, 3]
