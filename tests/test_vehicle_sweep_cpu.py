"""Vehicle sweeps (rl_qss_sim_vehicles_*: one vehicle per instance), the part that needs no GPU: what the strict oracle and the
schedule model (tests/qss_schedule_model.py, window 24 = kDfR) say about every (table, vehicle) pair tests/test_vehicle_sweep_gpu.py
gives to the kernels, batch.vehicle_tables_batch, the keyword rules of batch.lap_times_*, and the declarations."""
import os
import re

import numpy as np
import pytest

import qss_cases as qc
import vehicle_sweep_cases as vc
from conftest import ROOT
from oracle import oracle as orc

WINDOW = 24        # kDfR of csrc/rl_qss_df.hpp


@pytest.fixture(scope="module")
def modelled():
    return vc.model_all(WINDOW)


def test_vehicle_0_is_the_base_vehicle():
    for tag in vc.TAGS:
        for a, b in zip(vc.vehicle(tag, 0), qc.vehicle(tag)):
            np.testing.assert_array_equal(a, b)
        ax, ac, dx, dc, pr = vc.vehicle(tag, 5)
        np.testing.assert_array_equal(pr, [6.0, -12.0, 9.0, -9.0, 45.0, 50.0])
        assert ac.shape == qc.vehicle(tag)[1].shape and dc.shape == qc.vehicle(tag)[3].shape


def test_oracle_facts(modelled):
    """Iteration counts of the six vehicles with the "2p" lookups as pinned; with either lookup the reference raises on exactly
    vehicles 1 and 4 of seam4; every finished run passed the schedule model (vc.model_all asserts run() and the iteration
    count); the loguniform lap times span what they were chosen for."""
    for tag in vc.TAGS:
        for prof, N in vc.INPUTS:
            its = [modelled[vc.label(prof, N, tag, v)][0] for v in range(vc.NV)]
            print(f"{prof} N={N} {tag}: iterations {its}")
            assert [it == -1 for it in its] == [(prof, v) in vc.RAISES for v in range(vc.NV)], (tag, prof, its)
            if tag == "2p":
                assert tuple(its) == vc.ITERS_2P[prof]
            for v in range(vc.NV):
                out, it = orc.qss_sim(vc.table(prof, N), *vc.vehicle(tag, v))
                assert it == its[v]
        for prof, v in vc.MIXED:
            assert modelled[vc.label(prof, vc.MIXED_N, tag, v)][0] >= 0
    for lab, (it, r) in modelled.items():
        assert (r is None) == (it == -1), lab
        if r is not None:
            assert r["iterations"] == it and r["rules"]["ready"] == r["steps"], lab
    assert set(modelled) == {c[0] for c in vc.single_runs()}
    laps = [orc.qss_sim(vc.table("loguniform", 319), *vc.vehicle("2p", v))[0][:, 16].sum() for v in range(vc.NV)]
    print("loguniform N=319 2p lap times [s]:", np.round(laps, 3).tolist())
    assert (round(min(laps), 1), round(max(laps), 1)) == vc.LOGUNIFORM_LAP_TIMES_2P


def test_vehicle_tables_batch_shapes_and_errors():
    from spline_trajectory_optimization_amd import batch
    from spline_trajectory_optimization_amd.models.vehicle import Vehicle, VehicleParams
    for tag, (ma, md) in (("2p", (2, 2)), ("43p", (4, 3))):
        ax, ac, dx, dc, pr = batch.vehicle_tables_batch(vc.vehicles(tag))
        assert ax.shape == (6, ma + 1) and ac.shape == (6, 4, ma) and dx.shape == (6, md + 1) and dc.shape == (6, 4, md)
        assert pr.shape == (6, 6)
        for a in (ax, ac, dx, dc, pr):
            assert a.dtype == np.float64 and a.flags.c_contiguous
        for v in range(vc.NV):
            for a, one in zip((ax, ac, dx, dc, pr), vc.vehicle(tag, v)):
                np.testing.assert_array_equal(a[v], one)
    # Vehicle objects and 5-tuples mix; a Vehicle gives what its 5-tuple gives
    lx, lv, dx_, dv = qc.LOOKUPS["2p"]
    veh = Vehicle(VehicleParams(np.column_stack([lx, lv]), np.column_stack([dx_, dv]), *qc.PARAMS))
    both = batch.vehicle_tables_batch([veh, qc.vehicle("2p")])
    for a in both:
        np.testing.assert_array_equal(a[0], a[1])
    # unequal piece counts: the first odd instance is named
    mixed = [vc.vehicle("2p", 0), vc.vehicle("2p", 1), vc.vehicle("43p", 2), vc.vehicle("43p", 3)]
    with pytest.raises(ValueError, match=r"vehicles\[2\]"):
        batch.vehicle_tables_batch(mixed)
    with pytest.raises(ValueError):
        batch.vehicle_tables_batch([])
    with pytest.raises(ValueError):
        batch.vehicle_tables_batch([vc.vehicle("2p", 0)[:4]])


def test_lap_times_take_exactly_one_of_vehicle_and_vehicles():
    """Checked before anything touches the track or the device."""
    from spline_trajectory_optimization_amd import batch
    veh = vc.vehicle("2p", 0)
    for fn in (batch.lap_times_torch, batch.lap_times_host):
        with pytest.raises(ValueError, match="exactly one"):
            fn(None, None, 0, None, 1.0)
        with pytest.raises(ValueError, match="exactly one"):
            fn(None, None, 0, None, 1.0, veh, vehicles=[veh])
        with pytest.raises(ValueError, match="exactly one"):
            fn(None, None, 0, None, 1.0, vehicle=veh, bank=None, vehicles=batch.vehicle_tables_batch([veh]))


def test_ops_check_the_stacked_arrays_before_the_device():
    from spline_trajectory_optimization_amd import batch, ops
    pts = np.stack([vc.table("sawtooth", 256)] * 6)
    st = batch.vehicle_tables_batch(vc.vehicles("2p"))
    with pytest.raises(ValueError, match="points"):
        ops.qss_sim_vehicles(pts[:5].copy(), *st)                                  # five tables, six vehicles
    with pytest.raises(ValueError, match="points"):
        ops.qss_sim_vehicles(pts[0].copy(), *st)                                   # one table, not a batch
    with pytest.raises(ValueError, match="acc_c"):
        ops.qss_sim_vehicles(pts, st[0], st[1][:, :, :1].copy(), *st[2:])          # piece count of acc_c differs from acc_x
    with pytest.raises(ValueError, match="params"):
        ops.qss_sim_vehicles(pts, *st[:4], st[4].astype(np.float32))
    with pytest.raises(ValueError, match="dcc_x"):
        ops.qss_sim_vehicles(pts, st[0], st[1], st[2][::-1], st[3], st[4])         # not C-contiguous
    with pytest.raises(ValueError):
        ops.qss_sim_vehicles(pts[:1].copy(), *vc.vehicle("2p", 0))                 # one vehicle, not a stack


def test_declarations():
    """The header declares both entry points with rl_qss_sim's twelve arguments, _lib lists them, the library exports them, and
    the version stays 103."""
    from spline_trajectory_optimization_amd import _lib
    header = open(os.path.join(ROOT, "include", "rl_mincurv.h")).read()
    for name in ("rl_qss_sim_vehicles_dev", "rl_qss_sim_vehicles_host"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._SIGNATURES[name][1]) == decl.group(1).count(",") + 1 == 12 == len(_lib._SIGNATURES["rl_qss_sim"][1])
        assert getattr(_lib.load(), name) is not None
    assert re.search(r"#define\s+RL_VERSION\s+103\b", header)
