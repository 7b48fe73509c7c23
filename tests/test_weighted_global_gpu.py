"""The speed-weighted global min-curvature QP on the device: rl_mincurv_global_weighted_batch_* through ops.global_batch_*(weights=)
and the chain batch.vehicle_lines_*.  Need a real MI355X:  pytest -m gpu

Against the CPU twin tests/weighted_global_twin.py (pinned to the oracle at w = 1 by tests/test_weighted_global_cpu.py, 1e-8 m):
offsets and line to 1e-6 m -- the kernel-vs-twin bound of tests/test_global_qp.py::test_global_kernel_vs_twin -- violation
<= 1e-9 m, iteration counts within one (DESIGN a15 records one-apart cases between kernel and twin), the weighted cost to
rel 1e-7.  Once per instantiation of the dispatch: R = 5 / 6 with one group (c100 N = 500), R = 10 without register-resident
rows (c100 N = 4000), three groups (c30, n_p = 73), degree 3 (l10), and the generic kernel (a context created under
RL_GLOBAL_V1=1).  Everything else bit for bit: None / ones / the unweighted entry, a power-of-two weight, the position in the
batch, the refusal of one instance on the device entry, the chain against its steps issued one by one."""
import os

import numpy as np
import pytest

import vehicle_sweep_cases as vc
import weighted_global_twin as tw
from conftest import spline
from test_global_qp import MARGIN, monza_widths

pytestmark = pytest.mark.gpu
N = 500


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    ctx = _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch, ns.ctx = _lib, ops, batch, ctx
    return ns


@pytest.fixture(scope="module")
def monza(rl, fits):
    t, cx, cy, k, u, wl, wr = monza_widths(fits, "c100", N)
    m = dict(t=t, cx=cx, cy=cy, k=k, wl=wl, wr=wr, length=spline(fits, "c100")[4])
    m["trk"] = rl.lib.Track(rl.ctx, t, cx, cy, k, N)
    m["W1"] = np.ascontiguousarray(np.stack([wl, wr], 1)[None])
    m["w"] = 1.0 / np.linspace(20.0, 80.0, N)
    m["tab"] = tw.Tables(t, cx, cy, k, N)
    return m


def against_twin(tag, out, twin):
    """out = (ctrl, xy, a, st, rs) of one instance's call, twin = weighted_global_twin's result."""
    ctrl, xy, a, st, rs = out
    tcx, tcy, txy, ta, tst = twin
    da, dxy = np.abs(a[0] - ta).max(), np.abs(xy[0] - txy).max()
    print(f"[weighted global {tag}] |da| {da:.2e} m |dxy| {dxy:.2e} m  ipm {int(st[0, 0])}/{int(tst[0])}  "
          f"w k2 {st[0, 1]:.6f}->{st[0, 2]:.6f} (twin {tst[2]:.6f})  viol {st[0, 3]:.1e}  refused {st[0, 6]:.0f}  "
          f"block {rs.block_threads} lds {rs.lds_bytes}  {rs.kernel_ms:.2f} ms")
    assert da <= 1e-6 and dxy <= 1e-6
    assert np.abs(ctrl[0] - np.stack([tcx, tcy], 1)).max() <= 1e-6
    assert st[0, 3] <= 1e-9
    assert abs(int(st[0, 0]) - int(tst[0])) <= 1
    assert st[0, 1] == pytest.approx(tst[1], rel=1e-9) and st[0, 2] == pytest.approx(tst[2], rel=1e-7)
    assert st[0, 6] == 0.0 and st[0, 7] == 0.0


@pytest.mark.parametrize("n_outer", [1, 6])
def test_weighted_kernel_vs_twin(rl, monza, n_outer):
    """Fails without the feature: the entry does not exist."""
    m = monza
    out = rl.ops.global_batch_host(m["trk"], m["W1"], MARGIN, n_outer, weights=m["w"])
    twin = tw.global_mincurv_weighted(m["t"], m["cx"], m["cy"], m["k"], N, m["wl"], m["wr"], MARGIN, n_outer, weights=m["w"],
                                      tables=m["tab"])
    against_twin(f"c100 N={N} outer={n_outer}", out, twin)
    assert out[4].block_threads > 64 and out[4].block_threads % 64 == 0      # the wave-specialised kernel ran
    # and the weight did something: the unweighted line is elsewhere
    plain = rl.ops.global_batch_host(m["trk"], m["W1"], MARGIN, n_outer)
    assert np.hypot(*(plain[1][0] - out[1][0]).T).max() > 1e-3


def _case(fits, tag, n):
    if tag == "l10":  # degree-3 spline (the track boundary fit) with synthetic widths, as tests/test_global_qp.py
        t, cx, cy, k, _ = spline(fits, tag)
        wl = np.full(n, 4.0) + np.sin(np.arange(n) * 0.05)
        wr = np.full(n, 3.0) + np.cos(np.arange(n) * 0.03)
    else:
        t, cx, cy, k, _, wl, wr = monza_widths(fits, tag, n)
    return t, cx, cy, k, wl, wr


@pytest.mark.parametrize("tag,n,n_outer", [("c100", 4000, 6), ("c30", 2000, 3), ("l10", 1000, 2)],
                         ids=["rows10_l2_rows", "three_groups", "degree3"])
def test_weighted_kernel_vs_twin_other_instantiations(rl, fits, tag, n, n_outer):
    t, cx, cy, k, wl, wr = _case(fits, tag, n)
    w = 1.0 / np.linspace(20.0, 80.0, n)
    trk = rl.lib.Track(rl.ctx, t, cx, cy, k, n)
    out = rl.ops.global_batch_host(trk, np.stack([wl, wr], 1)[None], MARGIN, n_outer, weights=w)
    against_twin(f"{tag} N={n} outer={n_outer} n_p={len(cx) - k}", out,
                 tw.global_mincurv_weighted(t, cx, cy, k, n, wl, wr, MARGIN, n_outer, weights=w))
    assert out[4].block_threads > 64 and out[4].block_threads % 64 == 0


def test_weighted_generic_kernel_vs_twin(rl, monza):
    """RL_GLOBAL_V1 is read once, in rl_ctx_create: a context of its own (Context(...), not the cached Context.get) created
    under RL_GLOBAL_V1=1 keeps the generic kernel, in this process.  Same bounds; and, at w = 1, the unweighted generic bits."""
    m = monza
    old = os.environ.get("RL_GLOBAL_V1")
    os.environ["RL_GLOBAL_V1"] = "1"
    try:
        ctx = rl.lib.Context(0)
    finally:
        if old is None:
            del os.environ["RL_GLOBAL_V1"]
        else:
            os.environ["RL_GLOBAL_V1"] = old
    trk = rl.lib.Track(ctx, m["t"], m["cx"], m["cy"], m["k"], N)
    out = rl.ops.global_batch_host(trk, m["W1"], MARGIN, 6, weights=m["w"])
    fast = rl.ops.global_batch_host(m["trk"], m["W1"], MARGIN, 6, weights=m["w"])
    print(f"[weighted global generic] block {out[4].block_threads} lds {out[4].lds_bytes}; fast path block "
          f"{fast[4].block_threads} lds {fast[4].lds_bytes}")
    assert (out[4].block_threads, out[4].lds_bytes) != (fast[4].block_threads, fast[4].lds_bytes)   # another kernel ran
    against_twin(f"generic c100 N={N} outer=6", out,
                 tw.global_mincurv_weighted(m["t"], m["cx"], m["cy"], m["k"], N, m["wl"], m["wr"], MARGIN, 6, weights=m["w"],
                                            tables=m["tab"]))
    plain = rl.ops.global_batch_host(trk, m["W1"], MARGIN, 6)
    ones = rl.ops.global_batch_host(trk, m["W1"], MARGIN, 6, weights=np.ones(N))
    quarter = rl.ops.global_batch_host(trk, m["W1"], MARGIN, 6, weights=np.full(N, 0.25))
    for q in range(4):
        assert ones[q].tobytes() == plain[q].tobytes(), q
    for q in range(3):
        assert quarter[q].tobytes() == plain[q].tobytes(), q
    assert np.array_equal(quarter[3][:, 1:3], 0.25 * plain[3][:, 1:3])
    bad = np.ones(N); bad[3] = np.nan; bad[499] = 2.0 ** 31
    import torch
    dev = torch.device("cuda", 0)
    ref = rl.ops.global_batch_torch(trk, torch.from_numpy(m["W1"]).to(dev), MARGIN, 6, weights=torch.from_numpy(bad).to(dev))
    torch.cuda.synchronize()
    assert ref["stats"][0, 6].item() == 2.0 and ref["stats"][0, 0].item() == 0.0
    assert np.array_equal(ref["ctrl"][0].cpu().numpy(), np.stack([m["cx"], m["cy"]], 1))


def test_none_ones_and_the_unweighted_entry_are_the_same_bits(rl, monza):
    m = monza
    W = rl.batch.width_batch(m["wl"], m["wr"], 4, seed=3)
    plain = rl.ops.global_batch_host(m["trk"], W, MARGIN, 6)
    none = rl.ops.global_batch_host(m["trk"], W, MARGIN, 6, weights=None)
    ones = rl.ops.global_batch_host(m["trk"], W, MARGIN, 6, weights=np.ones((4, N)))
    quarter = rl.ops.global_batch_host(m["trk"], W, MARGIN, 6, weights=np.full(N, 0.25))
    for q, name in enumerate(("ctrl", "xy", "a", "stats")):
        assert none[q].tobytes() == plain[q].tobytes(), name
        assert ones[q].tobytes() == plain[q].tobytes(), name
    for q, name in enumerate(("ctrl", "xy", "a")):
        assert quarter[q].tobytes() == plain[q].tobytes(), name
    assert np.array_equal(quarter[3][:, 1:3], 0.25 * plain[3][:, 1:3])            # exactly: a power of two
    assert np.array_equal(quarter[3][:, [0, 3, 4, 5, 6, 7]], plain[3][:, [0, 3, 4, 5, 6, 7]])
    # the C entry with weights == NULL is the unweighted launch
    import ctypes
    lib, dp = rl.lib.load(), ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    ctrl, xy, a, st = np.zeros((4, m["trk"].n, 2)), np.zeros((4, N, 2)), np.zeros((4, m["trk"].n - m["k"])), np.zeros((4, 8))
    rc = lib.rl_mincurv_global_weighted_batch_host(rl.ctx.h, m["trk"].h, p(W), None, 4, MARGIN, 6, p(ctrl), p(xy), p(a), p(st),
                                                   None)
    assert rc == 0
    for got, want in zip((ctrl, xy, a, st), plain):
        assert got.tobytes() == want.tobytes()
    # the host entry refuses a bad weight itself, naming the instance
    wb = np.ones((4, N)); wb[2, 17] = 0.0
    rc = lib.rl_mincurv_global_weighted_batch_host(rl.ctx.h, m["trk"].h, p(W), p(wb), 4, MARGIN, 6, p(ctrl), p(xy), p(a), p(st),
                                                   None)
    assert rc == -1 and b"instance 2" in lib.rl_last_error()      # RL_ERR_ARG


def test_position_independence_and_broadcast(rl, monza):
    m = monza
    B = 8
    W = rl.batch.width_batch(m["wl"], m["wr"], B, seed=5)
    rng = np.random.default_rng(11)
    wts = np.ascontiguousarray(1.0 / rng.uniform(15.0, 90.0, size=(B, N)))
    out = rl.ops.global_batch_host(m["trk"], W, MARGIN, 3, weights=wts)
    again = rl.ops.global_batch_host(m["trk"], W, MARGIN, 3, weights=wts)
    perm = rng.permutation(B)
    moved = rl.ops.global_batch_host(m["trk"], np.ascontiguousarray(W[perm]), MARGIN, 3, weights=np.ascontiguousarray(wts[perm]))
    for q in range(4):
        assert again[q].tobytes() == out[q].tobytes(), q
        assert moved[q].tobytes() == np.ascontiguousarray(out[q][perm]).tobytes(), q
    assert len({out[2][b].tobytes() for b in range(B)}) == B
    one = rl.ops.global_batch_host(m["trk"], W, MARGIN, 3, weights=wts[0])
    rows = rl.ops.global_batch_host(m["trk"], W, MARGIN, 3, weights=np.ascontiguousarray(np.tile(wts[0], (B, 1))))
    for q in range(4):
        assert one[q].tobytes() == rows[q].tobytes(), q
    assert one[2][0].tobytes() == out[2][0].tobytes()


def test_device_entry_refuses_one_instance_and_leaves_the_rest(rl, monza):
    """A validated input, not a fault: instance 2 carries one NaN and one 2^31; the kernel reports it and runs it as
    n_outer = 0, the other three return what they return in a clean batch, the call returns RL_OK."""
    import torch
    m = monza
    dev = torch.device("cuda", 0)
    W = rl.batch.width_batch(m["wl"], m["wr"], 4, seed=9)
    wts = np.ascontiguousarray(np.tile(m["w"], (4, 1)))
    clean = rl.ops.global_batch_torch(m["trk"], torch.from_numpy(W).to(dev), MARGIN, 6, weights=torch.from_numpy(wts).to(dev))
    bad = wts.copy(); bad[2, 100] = np.nan; bad[2, 401] = 2.0 ** 31
    got = rl.ops.global_batch_torch(m["trk"], torch.from_numpy(W).to(dev), MARGIN, 6, weights=torch.from_numpy(bad).to(dev))
    torch.cuda.synchronize()
    c = {k_: v.cpu().numpy() for k_, v in clean.items() if k_ != "rl_stats"}
    g = {k_: v.cpu().numpy() for k_, v in got.items() if k_ != "rl_stats"}
    assert np.array_equal(c["stats"][:, 6], np.zeros(4))
    assert g["stats"][2, 6] == 2.0 and g["stats"][2, 0] == 0.0
    assert np.array_equal(g["ctrl"][2], np.stack([m["cx"], m["cy"]], 1))           # the input line
    assert not g["a"][2].any()
    for b in (0, 1, 3):
        for name in ("ctrl", "xy", "a", "stats"):
            assert g[name][b].tobytes() == c[name][b].tobytes(), (name, b)
    # the host form of the same call refuses before anything is enqueued
    with pytest.raises(ValueError, match="weights"):
        rl.ops.global_batch_host(m["trk"], W, MARGIN, 6, weights=bad)
    with pytest.raises(ValueError, match="dof=1"):
        rl.ops.global_batch_torch(m["trk"], torch.from_numpy(W).to(dev), MARGIN, 6, dof=2, weights=torch.from_numpy(wts).to(dev))


def test_vehicle_lines_chain(rl, monza):
    import torch
    m = monza
    dev, Wf = torch.device("cuda", 0), rl.lib.BOUNDS_WIDTHS
    pick = (0, 5, 2, 0)                                     # four of the grid's vehicles; the first and the last are equal
    vehs = [vc.vehicle("2p", v) for v in pick]
    w1 = torch.from_numpy(m["W1"]).to(dev)
    out = rl.batch.vehicle_lines_torch(m["trk"], w1, m["length"], vehs, rounds=2, margin=MARGIN, n_outer=6)
    torch.cuda.synchronize()
    o = {k_: v.cpu().numpy() for k_, v in out.items()}
    assert o["ctrl"].shape == (4, m["trk"].n, 2) and o["summary"].shape == (3, 4, 8) and o["stats"].shape == (3, 4, 8)
    assert o["weights"].shape == (4, N) and o["points"].shape == (4, N, 19)
    assert not o["stats"][:, :, 6].any() and np.all(o["stats"][:, :, 3] <= 1e-9)
    print(f"[vehicle lines] lap time per round [round, vehicle]: {np.round(o['summary'][:, :, 0], 3).tolist()} s")
    # the same steps issued one by one through ops
    w4 = w1.expand(4, N, 2).contiguous()
    stacked = tuple(torch.from_numpy(a).to(dev) for a in rl.batch.vehicle_tables_batch(vehs))
    sol = rl.ops.global_batch_torch(m["trk"], w4, MARGIN, 6)
    assert sol["stats"].cpu().numpy().tobytes() == o["stats"][0].tobytes()      # round 0 = the unweighted entry
    wts = None
    for r in range(3):
        pts = rl.ops.tables_torch(m["trk"], sol["ctrl"], Wf, w4, m["length"])
        it = rl.ops.qss_sim_vehicles_torch(pts, *stacked)
        summ = rl.ops.table_summary_torch(pts, it)
        assert summ.cpu().numpy().tobytes() == o["summary"][r].tobytes(), r
        assert sol["stats"].cpu().numpy().tobytes() == o["stats"][r].tobytes(), r
        if r < 2:
            wts = (1.0 / pts[:, :, 4]).contiguous()
            sol = rl.ops.global_batch_torch(m["trk"], w4, MARGIN, 6, weights=wts)
    assert sol["ctrl"].cpu().numpy().tobytes() == o["ctrl"].tobytes() and pts.cpu().numpy().tobytes() == o["points"].tobytes()
    assert wts.cpu().numpy().tobytes() == o["weights"].tobytes()
    zero = rl.batch.vehicle_lines_torch(m["trk"], w1, m["length"], vehs, rounds=0, margin=MARGIN, n_outer=6)
    plain = rl.ops.global_batch_torch(m["trk"], w4, MARGIN, 6)
    assert zero["ctrl"].cpu().numpy().tobytes() == plain["ctrl"].cpu().numpy().tobytes()
    # equal vehicles, equal bits; different vehicles, different lines
    assert o["ctrl"][0].tobytes() == o["ctrl"][3].tobytes() and o["summary"][:, 0].tobytes() == o["summary"][:, 3].tobytes()
    for b in (1, 2):
        d = np.abs(o["ctrl"][b] - o["ctrl"][0]).max()
        print(f"[vehicle lines] vehicle {pick[b]} against vehicle {pick[0]}: control points {d:.3f} m apart")
        assert d > 1e-3
    # a permutation of the vehicles permutes the result
    perm = [2, 0, 3, 1]
    moved = rl.batch.vehicle_lines_torch(m["trk"], w1, m["length"], [vehs[p] for p in perm], rounds=2, margin=MARGIN, n_outer=6)
    assert moved["ctrl"].cpu().numpy().tobytes() == np.ascontiguousarray(o["ctrl"][perm]).tobytes()
    assert moved["summary"].cpu().numpy().tobytes() == np.ascontiguousarray(o["summary"][:, perm]).tobytes()
    # the host twin of the call
    host = rl.batch.vehicle_lines_host(m["trk"], m["W1"], m["length"], vehs, rounds=2, margin=MARGIN, n_outer=6)
    for name in ("ctrl", "summary", "stats", "weights", "points"):
        assert host[name].tobytes() == o[name].tobytes(), name
