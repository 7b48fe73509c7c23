"""Vehicle sweeps on the device: rl_qss_sim_vehicles_* (one vehicle per instance) through ops.qss_sim_vehicles[_torch],
batch.lap_times_*(vehicles=...), batch.lap_times_grid_torch and Simulator.run_simulation_batch(vehicles=...).
Need a real MI355X:  pytest -m gpu

Inputs (tests/vehicle_sweep_cases.py): three synthetic tables (sawtooth N = 256, loguniform N = 319, seam4 N = 320), each as a
batch of six under six vehicles derived from each of the two lookups of tests/qss_cases.py; a mixed batch of three tables x three
vehicles at N = 320; the 16-instance Monza fixture of tests/test_tables_gpu.py for the chain.  Every (table, vehicle) pair has
passed the oracle and tests/qss_schedule_model.py first (the `modelled` fixture; pinned in tests/test_vehicle_sweep_cpu.py).

Against the oracle called with the instance's own vehicle: iteration counts and owner flags exactly, value columns to 1e-10
(the tolerance of tests/test_qss_gpu.py).  Everything else bit for bit: the kernel variants among each other, an instance
against ops.qss_sim of its table with its vehicle alone, permutations, the chain against its single-vehicle form.  With the
hook "qss_df_redo" = 0 no instance may come back from the dataflow kernel."""
import contextlib

import numpy as np
import pytest

import qss_cases as qc
import vehicle_sweep_cases as vc
from oracle import oracle as orc
from test_tables_gpu import monza16  # noqa: F401  (the fixture: first 16 instances of the benchmarked batch, solved)

pytestmark = pytest.mark.gpu

KERNELS = [("list", dict(qss_kernel=0))] + [(f"flow{w}", dict(qss_kernel=1, qss_df_waves=w)) for w in (1, 2, 4)] + \
          [("flow4-noredo", dict(qss_kernel=1, qss_df_waves=4, qss_df_redo=0))]
CASES = [(prof, N, tag) for tag in vc.TAGS for prof, N in vc.INPUTS]
IDS = [f"{prof}-N{N}-{tag}" for prof, N, tag in CASES]
WRITTEN = [4, 14, 15, 16, 18]
UNTOUCHED = [c for c in range(19) if c not in WRITTEN]


@pytest.fixture(scope="module")
def rl():
    from spline_trajectory_optimization_amd import _lib, batch, ops
    ctx = _lib.Context.get(0)  # raises loudly when the HIP extension / device is missing
    ctx.set_arith(_lib.ARITH_DEFAULT)

    class NS:
        pass
    ns = NS()
    ns.lib, ns.ops, ns.batch, ns.ctx = _lib, ops, batch, ctx
    return ns


@pytest.fixture(scope="module")
def modelled():
    """A (table, vehicle) pair that has not passed the schedule model is not given to the GPU: label -> (iterations, result)."""
    return vc.model_all()


@contextlib.contextmanager
def qss_options(rl, qss_kernel=-1, qss_df_waves=4, qss_df_bail_at=0, qss_df_redo=1):
    try:
        for k_, v_ in (("qss_kernel", qss_kernel), ("qss_df_waves", qss_df_waves), ("qss_df_bail_at", qss_df_bail_at),
                       ("qss_df_redo", qss_df_redo)):
            rl.ctx.set_option(k_, v_)
        yield rl.ctx
    finally:
        for k_, v_ in (("qss_kernel", -1), ("qss_df_waves", 4), ("qss_df_bail_at", 0), ("qss_df_redo", 1)):
            rl.ctx.set_option(k_, v_)


def run_vehicles(rl, pts, vehs, **opt):
    """One rl_qss_sim_vehicles_host call: pts [B,N,19], vehs = B 5-tuples."""
    with qss_options(rl, **opt):
        out, it = rl.ops.qss_sim_vehicles(np.ascontiguousarray(pts), *rl.batch.vehicle_tables_batch(vehs))
    return out, it.astype(np.int64)


def run_single(rl, pts, veh, **opt):
    with qss_options(rl, **opt):
        out, it = rl.ops.qss_sim(pts, *veh)
    return out, int(np.atleast_1d(it)[0])


def six(prof, N):
    return np.ascontiguousarray(np.repeat(vc.table(prof, N)[None], vc.NV, axis=0))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_parity_per_vehicle(rl, modelled, case):
    """1. The same table under the six vehicles, one batch, on every kernel variant, each instance against the oracle called
    with that instance's vehicle; with redo off no instance is handed back."""
    prof, N, tag = case
    pts, vehs = six(prof, N), vc.vehicles(tag)
    for v in range(vc.NV):
        assert vc.label(prof, N, tag, v) in modelled, "not through the schedule model"
    res = {name: run_vehicles(rl, pts, vehs, **opt) for name, opt in KERNELS}
    lout, lit = res["list"]
    for v in range(vc.NV):
        ref, oit = orc.qss_sim(pts[v], *vehs[v])
        assert oit == modelled[vc.label(prof, N, tag, v)][0]
        for name, (out, it) in res.items():
            assert it[v] == oit, (prof, N, tag, name, v, it.tolist(), oit)
        np.testing.assert_array_equal(lout[v][:, UNTOUCHED], pts[v][:, UNTOUCHED])
        if oit < 0:
            continue     # (what the profile holds when the reference raises depends on the order the steps ran in)
        np.testing.assert_array_equal(lout[v][:, 18], ref[:, 18])
        dev = np.abs(lout[v][:, [4, 14, 15, 16]] - ref[:, [4, 14, 15, 16]]).max(axis=0)
        print(f"{prof}-N{N}-{tag} vehicle {v}: iterations {oit}, max |kernel - oracle| speed {dev[0]:.2e} lon {dev[1]:.2e} "
              f"lat {dev[2]:.2e} time {dev[3]:.2e}")
        np.testing.assert_allclose(lout[v][:, [4, 14, 15, 16]], ref[:, [4, 14, 15, 16]], rtol=0, atol=1e-10)
    qc.assert_not_handed_back(res["flow4-noredo"][1], f"{prof}-N{N}-{tag}, flow4-noredo")
    for name, (out, it) in res.items():
        np.testing.assert_array_equal(it, lit)
        np.testing.assert_array_equal(out, lout, err_msg=f"{prof}-N{N}-{tag}: {name} against the list order")
    lap = lout[:, :, 16].sum(axis=1)
    assert len({float(x) for x, i in zip(lap, lit) if i >= 0}) >= 4, "the vehicles must matter to the result"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_single_call_parity(rl, case):
    """2. Every instance's rows are bit-identical to ops.qss_sim of that table with that vehicle alone: on the list order, the
    dataflow kernel, and with the kernel each call picks for itself."""
    prof, N, tag = case
    pts, vehs = six(prof, N), vc.vehicles(tag)
    for name, opt in (("list", dict(qss_kernel=0)), ("flow4", dict(qss_kernel=1)), ("default", dict())):
        out, it = run_vehicles(rl, pts, vehs, **opt)
        for v in range(vc.NV):
            one, it1 = run_single(rl, pts[v], vehs[v], **opt)
            assert it1 == it[v], (name, v, it1, it.tolist())
            assert out[v].tobytes() == one.tobytes(), (name, v)


@pytest.mark.parametrize("tag", vc.TAGS)
def test_permutation_and_copies(rl, tag):
    """3. Reversing the order of the vehicles reverses the results bit for bit; six copies of vehicle 2 equal the shared-vehicle
    call with vehicle 2 bit for bit."""
    prof, N = "loguniform", 319
    pts, vehs = six(prof, N), vc.vehicles(tag)
    for name, opt in (("list", dict(qss_kernel=0)), ("flow4", dict(qss_kernel=1))):
        out, it = run_vehicles(rl, pts, vehs, **opt)
        rout, rit = run_vehicles(rl, pts, vehs[::-1], **opt)
        np.testing.assert_array_equal(rit, it[::-1])
        assert rout[::-1].tobytes() == out.tobytes(), name
        assert not np.array_equal(out[0], out[5])
        cout, cit = run_vehicles(rl, pts, [vehs[2]] * vc.NV, **opt)
        with qss_options(rl, **opt):
            sout, sit = rl.ops.qss_sim(pts, *vehs[2])
        np.testing.assert_array_equal(cit, sit)
        assert cout.tobytes() == sout.tobytes(), name
        assert cout[0].tobytes() == out[2].tobytes()


@pytest.mark.parametrize("tag", vc.TAGS)
def test_failure_is_per_instance(rl, tag):
    """4. seam4: -1 on exactly instances 1 and 4, the other four with the bits of their single runs, the failed ones with
    their input columns intact; run_simulation_batch(vehicles=...) raises and names instance 1."""
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    from spline_trajectory_optimization_amd.simulator.simulator import Simulator
    pts, vehs = six("seam4", 320), vc.vehicles(tag)
    for name, opt in (("list", dict(qss_kernel=0)), ("flow4", dict(qss_kernel=1)), ("flow4-noredo", dict(qss_kernel=1, qss_df_redo=0)),
                      ("default", dict())):
        out, it = run_vehicles(rl, pts, vehs, **opt)
        qc.assert_not_handed_back(it, f"seam4-N320-{tag}, {name}")
        assert (it == -1).tolist() == [v in (1, 4) for v in range(vc.NV)], (name, it.tolist())
        for v in range(vc.NV):
            if v in (1, 4):     # (what the written columns hold when the reference raises depends on the order the steps ran in)
                np.testing.assert_array_equal(out[v][:, UNTOUCHED], pts[v][:, UNTOUCHED])
                continue
            one, it1 = run_single(rl, pts[v], vehs[v], **opt)
            assert it1 == it[v] and out[v].tobytes() == one.tobytes(), (name, v)
    lx, lv, dx, dv = qc.LOOKUPS[tag]
    sim = Simulator(Vehicle(VehicleParams(np.column_stack([lx, lv]), np.column_stack([dx, dv]), *qc.PARAMS)))
    with pytest.raises(FloatingPointError, match=r"instance 1 \(and 1 more: \[4\]\)"):
        sim.run_simulation_batch(pts, vehicles=vehs)
    good = [0, 2, 3, 5]
    res = sim.run_simulation_batch(np.ascontiguousarray(pts[good]), vehicles=[vehs[v] for v in good])
    out, it = run_vehicles(rl, pts, vehs)
    assert len(res) == 4
    for r, v in zip(res, good):
        assert r.trajectory.points.tobytes() == out[v].tobytes()
    # without `vehicles` the simulator's own vehicle runs, as before: vehicle 0 of the grid on every instance
    own = sim.run_simulation_batch(np.ascontiguousarray(pts[:2]))
    assert own[0].trajectory.points.tobytes() == own[1].trajectory.points.tobytes() == out[0].tobytes()


@pytest.mark.parametrize("tag", vc.TAGS)
def test_mixed_tables_and_vehicles(rl, modelled, tag):
    """5. Three different tables under three different vehicles in one batch, against three single calls."""
    pts = np.ascontiguousarray(np.stack([vc.table(prof, vc.MIXED_N) for prof, v in vc.MIXED]))
    vehs = [vc.vehicle(tag, v) for prof, v in vc.MIXED]
    for prof, v in vc.MIXED:
        assert modelled[vc.label(prof, vc.MIXED_N, tag, v)][0] >= 0
    for name, opt in KERNELS + [("default", dict())]:
        out, it = run_vehicles(rl, pts, vehs, **opt)
        if name.endswith("-noredo"):
            qc.assert_not_handed_back(it, f"mixed-{tag}, {name}")
        for b, (prof, v) in enumerate(vc.MIXED):
            one, it1 = run_single(rl, pts[b], vehs[b], **opt)
            assert it1 == it[b] == modelled[vc.label(prof, vc.MIXED_N, tag, v)][0], (name, b, it1, it.tolist())
            assert out[b].tobytes() == one.tobytes(), (name, b)
    with qss_options(rl):      # the torch form, device tensors throughout, on the current stream
        import torch
        dev = torch.device("cuda", 0)
        dpts = torch.from_numpy(pts).to(dev)
        dveh = [torch.from_numpy(a).to(dev) for a in rl.batch.vehicle_tables_batch(vehs)]
        dit = rl.ops.qss_sim_vehicles_torch(dpts, *dveh)
        torch.cuda.synchronize()
    out, it = run_vehicles(rl, pts, vehs)
    np.testing.assert_array_equal(dit.cpu().numpy(), it)
    assert dpts.cpu().numpy().tobytes() == out.tobytes()


def test_argument_errors(rl):
    pts, st = six("sawtooth", 256), rl.batch.vehicle_tables_batch(vc.vehicles("2p"))
    lib = rl.lib.load()
    rc = lib.rl_qss_sim_vehicles_host(rl.ctx.h, None, 6, 256, *[None] * 2, 2, *[None] * 2, 2, None, None)
    assert rc == -1      # RL_ERR_ARG: null argument
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    it = np.zeros(6, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    rc = lib.rl_qss_sim_vehicles_host(rl.ctx.h, p(pts), 6, 256, p(st[0]), p(st[1]), 0, p(st[2]), p(st[3]), 2, p(st[4]),
                                      it.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == -1      # RL_ERR_ARG: a table without pieces


def _grid_vehicles(count):
    return [vc.vehicle("2p", v % vc.NV) for v in range(count)]


def test_chain_lap_times_with_vehicles(rl, monza16):  # noqa: F811
    """6. lap_times_torch(vehicles=[v0..v5, v0, ...]) on the 16 Monza instances equals per-instance lap_times_torch(vehicle=...)
    bit for bit; the stacked forms (numpy, cuda) and the host form give the same."""
    import torch
    m = monza16
    W, dev = rl.lib.BOUNDS_WIDTHS, torch.device("cuda", 0)
    ctrl_d, w_d = torch.from_numpy(m["ctrl"]).to(dev), torch.from_numpy(m["widths"]).to(dev)
    vehs = _grid_vehicles(16)
    out = rl.batch.lap_times_torch(m["trk"], ctrl_d, W, w_d, m["length"], vehicles=vehs)
    torch.cuda.synchronize()
    pts, iters, summ = out["points"].cpu().numpy(), out["iters"].cpu().numpy(), out["summary"].cpu().numpy()
    assert np.all(iters > 0)
    for b in range(16):
        one = rl.batch.lap_times_torch(m["trk"], ctrl_d[b:b + 1].contiguous(), W, w_d[b:b + 1].contiguous(), m["length"],
                                       vehicle=vehs[b])
        assert int(one["iters"][0]) == iters[b]
        assert one["points"][0].cpu().numpy().tobytes() == pts[b].tobytes(), b
        assert one["summary"][0].cpu().numpy().tobytes() == summ[b].tobytes(), b
    print(f"[vehicle sweep chain] lap times of the 16 instances: {np.round(summ[:, 0], 3).tolist()} s")
    assert len(set(summ[:6, 0].tolist())) == 6
    stacked = rl.batch.vehicle_tables_batch(vehs)
    for form in (stacked, tuple(torch.from_numpy(a).to(dev) for a in stacked)):
        again = rl.batch.lap_times_torch(m["trk"], ctrl_d, W, w_d, m["length"], vehicles=form)
        assert again["points"].cpu().numpy().tobytes() == pts.tobytes()
    host = rl.batch.lap_times_host(m["trk"], m["ctrl"], W, m["widths"], m["length"], vehicles=vehs)
    assert host["points"].tobytes() == pts.tobytes() and host["summary"].tobytes() == summ.tobytes()
    np.testing.assert_array_equal(host["iters"], iters)
    with pytest.raises(ValueError, match="15 vehicles for 16"):
        rl.batch.lap_times_torch(m["trk"], ctrl_d, W, w_d, m["length"], vehicles=vehs[:15])


def test_grid_lines_times_vehicles(rl, monza16):  # noqa: F811
    """7. lap_times_grid_torch with L = 4 lines x V = 3 vehicles equals the twelve single-vehicle results."""
    import torch
    m = monza16
    W, dev = rl.lib.BOUNDS_WIDTHS, torch.device("cuda", 0)
    L, vehs = 4, [vc.vehicle("2p", v) for v in (0, 5, 2)]
    ctrl_d = torch.from_numpy(np.ascontiguousarray(m["ctrl"][:L])).to(dev)
    w_d = torch.from_numpy(np.ascontiguousarray(m["widths"][:L])).to(dev)
    grid = rl.batch.lap_times_grid_torch(m["trk"], ctrl_d, W, w_d, m["length"], vehs)
    torch.cuda.synchronize()
    assert tuple(grid["summary"].shape) == (L, 3, 8) and tuple(grid["iters"].shape) == (L, 3)
    assert tuple(grid["points"].shape) == (L, 3, m["N"], 19)
    summ, iters, pts = grid["summary"].cpu().numpy(), grid["iters"].cpu().numpy(), grid["points"].cpu().numpy()
    for v, veh in enumerate(vehs):
        one = rl.batch.lap_times_torch(m["trk"], ctrl_d, W, w_d, m["length"], vehicle=veh)
        np.testing.assert_array_equal(one["iters"].cpu().numpy(), iters[:, v])
        assert one["summary"].cpu().numpy().tobytes() == np.ascontiguousarray(summ[:, v]).tobytes(), v
        assert one["points"].cpu().numpy().tobytes() == np.ascontiguousarray(pts[:, v]).tobytes(), v
    print(f"[vehicle sweep grid] lap times [line, vehicle]: {np.round(summ[:, :, 0], 3).tolist()} s")
    assert np.all(iters > 0) and np.all(summ[:, 1, 0] > summ[:, 0, 0])       # vehicle 5 is slower than vehicle 0 on every line
