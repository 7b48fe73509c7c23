#!/usr/bin/env python3
"""bench.py -- min-curvature QP solves/sec at N=2000 waypoints on 1/2/4/8 MI355X.

Workloads
  monza (default; BASELINE.json configs[1]): Monza centre line
      (BSplineTrajectory s=100, k=5 -> 66 control points), N=2000 samples, B=1024 track instances PER GPU
      whose half-widths are the Monza half-widths scaled per instance by 1+e, e~U(-0.15,0.15)
      (numpy default_rng(1234 + rank)), floor 1.5 m.
  mixed (BASELINE.json configs[2]): per GPU half the batch Monza as above and
      half the synthetic Indy-style oval (rotated 17 degrees, widths seed 5678 + rank), grouped by track:
      two launches per step, on two streams, one per knot layout.

UNIT OF WORK.  One "solve" = the reference's complete TrajectoryOptimizer.run_min_curvature_qp for one
instance (optimizer.py:256-341, max_iter=5 -> 5 x (forward + backward) sweeps over the free control
points = 610 control-point QPs on Monza, each followed by re-sampling and boundary re-intersection), sweep
order pinned.  This is the path with reference parity, which is why it is the headline; SURVEY.md 8(d)'s
other unit (one global banded QP per linearisation, the north_star's design kernel, own formulation)
is reported as a second top-level leg, `global_qp`, with its own roofline block.
One "step" = one launch of the sweep kernel over the rank's whole batch, inputs already resident in
HBM; for N>1 ranks every step is followed by the single gather of the results to rank 0, issued
asynchronously (double-buffered outputs) so that it overlaps the next step's launch; the timed region
ends only after the last gather has completed.

`python bench.py --gpus N` starts its own N rank processes (children, spawned before anything touches
the GPU); under torch.distributed.run (WORLD_SIZE already set) it is one of the ranks.

A plain run sets up, warms up, times the K steps and prints the headline.  `--full` adds everything else the
line can carry: the CPU baseline and the parity classification of its sample, the reference-order / fast /
branch comparison, the deviation from the reference's own runs, the global-QP, min-time NLP and QSS legs, and
(N > 1) the bit checksums of the gathered shards.  `--dump-outputs DIR` writes what the last timed step
returned to its caller as DIR/<group>_<array>.npy (float64; see dump_outputs).

Prints ONE JSON line (rank 0).  See the repo instructions for the field contract.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
FP64_VECTOR_PEAK_GFLOPS = 78600.0  # 256 CU x 4 SIMD x 16 FP64 lanes/clk x 2 (FMA) x 2.4 GHz
N_WAYPOINTS = 2000
BATCH_PER_GPU = 1024
MAX_ITER = 5            # run_min_curvature_qp default (optimizer.py:256)
SPLINE_S, SPLINE_K = 100.0, 5
BYTES_PER_SOLVE = 8 * N_WAYPOINTS * (2 + 2)  # widths in (2 cols) + x,y out (2 cols)
GLOBAL_MARGIN, GLOBAL_OUTER = 0.25, 6


# ------------------------------------------------------------------------------------------------
def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N rank processes as CHILDREN (this parent
    never initialises the GPU and never execs), wait for them, pass rank 0's JSON line through."""
    import __graft_entry__ as ge
    ge.build_hip()  # hipcc only; the children then find the library up to date and never race on it
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = time.time() + 3000
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is not None:
                alive.remove(p)
                if code != 0:
                    rc = rc or code
                    for q in alive:      # a rank failed: end exactly the processes started here
                        q.terminate()
        if time.time() > deadline:
            for q in alive:
                q.kill()
            rc = rc or 124
            break
        time.sleep(0.2)
    sys.exit(rc)


# ------------------------------------------------------------------------------------------------
SWEEP_LIMITER = ("one instance's 610 dependent steps: the batch's 1024 workgroups all run at once (4 per CU), so the kernel time is the "
                 "latency of one instance under that sharing.  Across every arithmetic mode and build of rounds 5-6 it is 2.9-3.0 ps per "
                 "executed VALU wave-instruction (1024 SIMDs issuing ~56 % of their cycles); removing instructions or memory round "
                 "trips from a step pays, moving work to idle waves does not (measured: DESIGN.md section 5).  The solver state is on "
                 "chip: the HBM roofline is the one north_star designates, the kernel is not HBM bound")


def profile_block(kernel):
    """Counter-derived figures of `kernel` from the committed rocprofv3 summary (profiles/): NOT measured in
    this run -- PMC collection needs its own rocprofv3 passes (tools/profile_bench.sh)."""
    path = os.path.join(ROOT, "profiles", "counters_latest.json")
    if not os.path.exists(path):
        return None
    try:
        d = json.load(open(path))
        k = d["kernels"][kernel]
    except Exception:
        return None
    k = dict(k)
    k["source"] = d.get("source", "profiles/counters_latest.json")
    k["measured_in_run"] = False
    return k


def cpu_legs(groups, i_starts, xy_gpu, ninst_total):
    """cpu_baseline: the oracle (a port of the reference's arithmetic, oracle/mincurv_oracle.c) timed on a
    bounded sample of the same workload, one instance per host thread; then the per-instance parity rule
    of tests/parity_rule.py on that sample (strict oracle vs its re-roundings)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity_rule
    per = max(1, ninst_total // len(groups))
    cores = max(1, min(os.cpu_count() or 1, per))
    t_wall, done, cls, pos = 0.0, 0, [], []
    for g, ist, xy in zip(groups, i_starts, xy_gpu):
        po = parity_rule.ParityOracle(g["t"], g["cx"], g["cy"], g["k"], g["length"], N_WAYPOINTS, g["widths"][:per], ist,
                                      n_seeds=2, nthreads=cores)
        t_wall += po.t_strict          # the timed leg: the strict oracle only
        done += per
        cls.append(parity_rule.classify(xy[:per], po))
        pos.append(po)
    c = {k_: np.concatenate([x[k_] for x in cls]) for k_ in cls[0]}
    probe = {}
    for mod in ("casadi", "shapely"):
        try:
            __import__(mod)
            probe[mod] = True
        except Exception:
            probe[mod] = False
    gv = parity_rule.summary(c)
    gv["rule"] = ("NEAREST BRANCH, per instance: max|GPU - strict oracle| <= 1e-4 m, or max|GPU - oracle_r| <= 1e-4 m for one "
                  "of the oracle's re-roundings r (FMA build; up to 24 seeded +-1 ulp re-roundings of sampled positions / bound "
                  "points) -- no multiple of a spread is accepted (tests/parity_rule.py)")
    gv["per_instance"] = [{"instance": int(b), "dev_m": float(c["dev"][b]), "nearest_branch_dev_m": float(c["nearest"][b]),
                           "branch": c["branch"][b], "oracle_rerounding_spread_m": float(c["noise"][b])} for b in range(len(c["dev"]))]
    cb = {"value": done / t_wall, "unit": "solves/s", "cores": cores, "kind": "port",
          "sample": f"{done} of the batch's instances (N={N_WAYPOINTS}, max_iter={MAX_ITER}), one per thread, "
                    f"{t_wall:.1f} s wall",
          "reference_path_probe": dict(probe, note="the reference's own CasADi/qpOASES + shapely path needs both "
                                       "modules and the reference tree; neither is on this box, so kind stays 'port'"),
          "gpu_vs_oracle": gv}
    ref_loop = reference_loop_time()
    if ref_loop:
        cb["reference_loop"] = ref_loop
    return cb, pos


def reference_order_leg(g, args, torch, search, fast_kernel_ms, fast_xy, po, ref_run, fast_ns_all=None):
    """The same batch through the sweep's REFERENCE-ORDER arithmetic (RL_ARITH_REFERENCE, include/rl_mincurv.h, the default
    since round 6): the reference's operations in the reference's order, which returns the oracle's bits.  Timed like the
    headline (events on the launch stream around each of `steps` launches after a warm-up); compared, on the cpu_baseline
    sample, with the oracle's build whose atan2 / cos / sin are the correctly rounded ones (bit for bit), with the strict
    oracle on the platform libm and with the reference's own runs (fixtures G7b, G7d).  The fast and the branch arithmetic are
    timed here too and laid beside it on the WHOLE batch (fast_xy None: the headline ran in the reference-order arithmetic)."""
    from oracle import oracle as orc
    from spline_trajectory_optimization_amd import _lib, ops

    def timed(arith_):
        o_ = ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search, arith=arith_)
        torch.cuda.synchronize()
        ev_ = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a_, b_ in ev_:
            a_.record()
            ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search, out=o_, arith=arith_)
            b_.record()
        torch.cuda.synchronize()
        return o_, float(np.mean([a_.elapsed_time(b_) for a_, b_ in ev_]))

    if fast_xy is None:
        fo, fast_kernel_ms = timed(_lib.ARITH_FAST)
        fast_xy, fast_ns_all = fo["xy"].cpu().numpy(), fo["n_success"].cpu().numpy()
    out = ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search, arith=_lib.ARITH_REFERENCE)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record()
        ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search, out=out,
                              arith=_lib.ARITH_REFERENCE)
        b.record()
    torch.cuda.synchronize()
    ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    B = g["widths"].shape[0]
    xy = out["xy"].cpu().numpy(); ctrl = out["ctrl"].cpu().numpy(); ns = out["n_success"].cpu().numpy()
    fast_xy_all = fast_xy
    leg = {"what": "the headline batch in RL_ARITH_REFERENCE: unfused de Boor recurrences and sums, splder derivative splines in the "
                   "cost, sequential cost sums, unfused cross products, correctly rounded atan2 / cos / sin (csrc/rl_crmath.hpp)",
           "kernel": "k_sweep<..., STRICT>", "kernel_ms": ms, "solves_per_s": B / ms * 1e3, "steps": args.steps,
           "cost_vs_fast": ms / fast_kernel_ms, "fast_kernel_ms": fast_kernel_ms, "fast_solves_per_s": B / fast_kernel_ms * 1e3,
           "default": "reference-order (round 6): rl_ctx_create, RL_ARITH unset and bench.py --arith all start there; "
                      "rl_ctx_set_arith(ctx, RL_ARITH_FAST) / RL_ARITH=fast / bench.py --arith fast select the fast arithmetic",
           "lds_bytes_per_workgroup": int(out["stats"].lds_bytes)}
    prof = profile_block("k_sweep_reference_order")
    ach = (BYTES_PER_SOLVE * B) / (ms * 1e-3) / 1e9
    leg["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBPS,
                       "traffic": prof.get("hbm_bytes_fetch_x2") if prof else None, "traffic_source": prof.get("source") if prof else None,
                       "traffic_measured_in_run": False, "kernel_ms": ms, "algorithmic_bytes_per_launch": BYTES_PER_SOLVE * B,
                       "actual_limiter": SWEEP_LIMITER,
                       "valu": valu_block(prof, ms)}
    if po is not None:
        m = po.xy0.shape[0]
        dev = np.abs(xy[:m] - po.xy0).reshape(m, -1).max(axis=1)
        with orc.cr_variant():
            t0 = time.perf_counter()
            octrl, oxy, ons = orc.solve_width_batch(*po.args, po.widths, po.i_start, nthreads=po.nthreads)
            dt = time.perf_counter() - t0
        bit = [bool(np.array_equal(ctrl[b], octrl[b]) and np.array_equal(xy[b], oxy[b]) and np.array_equal(ns[b].ravel(), ons[b].ravel()))
               for b in range(m)]
        leg["gpu_vs_oracle"] = {
            "sample": m, "dev_m_median": float(np.median(dev)), "dev_m_max": float(dev.max()),
            "vs": "the strict oracle on the platform libm (the same lines the headline's gpu_vs_oracle uses)",
            "bit_identical_to_the_correctly_rounded_oracle": int(sum(bit)),
            "correctly_rounded_oracle": f"oracle/libmincurv_oracle_cr.so (atan2 / cos / sin through libquadmath), {dt:.1f} s for the sample; "
                                        "control points, sampled line and success counts compared as bit patterns",
            "cr_oracle_vs_libm_oracle_dev_m_max": float(np.abs(oxy - po.xy0).max()),
            "fast_arithmetic_dev_m_median": float(np.median(np.abs(fast_xy[:m] - po.xy0).reshape(m, -1).max(axis=1)))}
    # the WHOLE batch: the reference-order result is the oracle's bits (checked on the sample above), so it is the oracle for
    # every instance -- how far the cheaper arithmetic modes end from it
    try:
        br = ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search, arith=_lib.ARITH_BRANCH)
        torch.cuda.synchronize()
        evb = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a_, b_ in evb:
            a_.record()
            ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search, out=br, arith=_lib.ARITH_BRANCH)
            b_.record()
        torch.cuda.synchronize()
        whole = {"oracle": "the reference-order result of every instance (bit-identical to the CPU oracle on the sample)"}
        for name, other_xy, other_ns in (("fast", fast_xy_all, fast_ns_all), ("branch", br["xy"].cpu().numpy(), br["n_success"].cpu().numpy())):
            dv = np.abs(other_xy - xy).reshape(B, -1).max(axis=1)
            whole[name] = {"dev_m_median": float(np.median(dv)), "dev_m_p99": float(np.quantile(dv, 0.99)), "dev_m_max": float(dv.max()),
                           "instances_beyond_1e-4_m": int((dv > 1e-4).sum()), "instances": B,
                           "instances_with_other_success_counts": int((other_ns.reshape(B, -1) != ns.reshape(B, -1)).any(axis=1).sum())}
        whole["branch"]["kernel_ms"] = float(np.mean([a_.elapsed_time(b_) for a_, b_ in evb]))
        whole["branch"]["what"] = ("RL_ARITH_BRANCH: positions, ring crossings, bound points and rows in the reference's order; normals from a "
                                   "reciprocal square root, cost sums from the fast tables in a tree")
        whole["reading"] = ("the reference's formulation is chaotic in the last bits (DESIGN_HISTORY.md 5): every operation that rounds differently moves a few "
                            "per cent of the instances to another branch; only the reference-order arithmetic stays on the oracle's")
        leg["whole_batch_vs_reference_order"] = whole
    except Exception as e:
        leg["whole_batch_vs_reference_order"] = {"error": f"{type(e).__name__}: {e}"}
    if ref_run:
        d = {bi: float(np.hypot(ctrl[bi, :, 0] - rc[0], ctrl[bi, :, 1] - rc[1]).max()) for bi, rc in ref_run.items()}
        leg["gpu_vs_reference_run"] = {"instances": sorted(d), "dev_m": [d[b_] for b_ in sorted(d)],
                                       "within_1e-4": int(sum(v <= 1e-4 for v in d.values())),
                                       "fixture": "tests/golden/G7b_benchmarked_config.npz, G7d_benchmarked_batch_sample.npz (the reference's own "
                                                  "loop, numpy on glibc)"}
    return leg


def reference_loop_time():
    """Wall time of the REFERENCE's own run_min_curvature_qp loop (optimizer.py:256-341) at exactly this configuration,
    measured when fixture G7b was generated (tests/golden/make_golden.py: the reference's Python imported in the build
    container, one core per run) and stored in the fixture -- not measured on this box (the reference cannot travel)."""
    path = os.path.join(ROOT, "tests", "golden", "G7b_benchmarked_config.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    el = {str(k_): float(g[f"{k_}_elapsed_s"]) for k_ in g["cases"] if f"{k_}_elapsed_s" in g.files and "N2000" in str(k_)}
    if not el:
        return None
    mean = float(np.mean(list(el.values())))
    return {"value": 1.0 / mean, "unit": "solves/s", "cores": 1, "seconds_per_solve": el,
            "where": "build container (8 vCPU, no GPU), one core per run, measured at fixture generation -- not on this box",
            "caveat": "qpOASES and GEOS replaced by exact stand-ins (closed-form clamp, C ray-ring intersection): a LOWER "
                      "bound on the reference's own time per solve",
            "fixture": "tests/golden/G7b_benchmarked_config.npz"}


def global_qp_leg(trk, d_widths, g, args, torch, with_cpu):
    """Second leg (SURVEY.md 8(d) primary unit; 8a row a15, own formulation): the Monza batch through the
    global banded QP (rl_mincurv_global_batch_dev).  One launch = B instances x GLOBAL_OUTER Gauss-Newton
    linearisations, each one inequality-constrained QP (2N bound rows, n-k unknowns) solved by the
    interior-point kernel; timed with HIP events on the launch stream, outside the headline's region."""
    from spline_trajectory_optimization_amd import ops
    out = ops.global_batch_torch(trk, d_widths, GLOBAL_MARGIN, GLOBAL_OUTER)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record()
        ops.global_batch_torch(trk, d_widths, GLOBAL_MARGIN, GLOBAL_OUTER, out=out)
        b.record()
    torch.cuda.synchronize()
    ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    st = out["stats"].cpu().numpy()
    B = d_widths.shape[0]
    assert np.isfinite(st).all() and (st[:, 3] <= 1e-8).all(), "global QP: a line left its bounds"
    achieved = BYTES_PER_SOLVE * B / (ms * 1e-3) / 1e9
    prof = profile_block("k_global_qp")
    leg = {"metric": "global min-curvature QPs/sec (N=2000, one QP = one Gauss-Newton linearisation of the "
                     "whole line, 2N bound rows)",
           "value": B * GLOBAL_OUTER / ms * 1e3, "unit": "QPs/s", "instances_per_s": B / ms * 1e3,
           "kernel_ms": ms, "linearisations": GLOBAL_OUTER, "ipm_iterations_mean": float(st[:, 0].mean()),
           "sum_kappa2_before_after": [float(st[:, 1].mean()), float(st[:, 2].mean())],
           "max_bound_violation_m": float(st[:, 3].max()), "block_threads": int(out["rl_stats"].block_threads),
           "lds_bytes_per_workgroup": int(out["rl_stats"].lds_bytes),
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": achieved / HBM_PEAK_GBPS,
                        "traffic": prof.get("hbm_bytes_fetch_x2") if prof else None,
                        "traffic_source": prof.get("source") if prof else None, "traffic_measured_in_run": False,
                        "kernel": "k_global_qp2", "kernel_ms": ms,
                        "algorithmic_bytes_per_launch": BYTES_PER_SOLVE * B,
                        "actual_limiter": "FP64 VALU issue of the factorising wave + barriers (DESIGN_HISTORY.md 3b)",
                        "valu": valu_block(prof, ms)}}
    if with_cpu:
        from oracle import oracle as orc
        ninst = 4
        t0 = time.perf_counter()
        dev_m = 0.0
        xy = out["xy"][:ninst].cpu().numpy()
        for b in range(ninst):
            r = orc.global_mincurv(g["t"], g["cx"], g["cy"], g["k"], N_WAYPOINTS, g["widths"][b, :, 0],
                                   g["widths"][b, :, 1], GLOBAL_MARGIN, GLOBAL_OUTER)
            dev_m = max(dev_m, float(np.abs(r[2] - xy[b]).max()))
        dt = time.perf_counter() - t0
        assert dev_m < 1e-6, f"global QP deviates from its CPU twin: {dev_m}"
        leg["cpu_twin"] = {"instances_per_s": ninst / dt, "cores": 1, "sample": f"{ninst} instances, {dt:.2f} s",
                           "gpu_vs_twin_dev_m": dev_m}
    leg["two_dof"] = global_qp_xy_block(trk, d_widths, g, args, torch, with_cpu)
    return leg


GLOBAL_LON = 1.0   # [m] longitudinal bound of the two-coordinate formulation (julia/spline_traj_opt.ipynb L276-279)


def global_qp_xy_block(trk, d_widths, g, args, torch, with_cpu):
    """The same batch through the formulation with BOTH coordinates of every control point free (the Julia prototype's
    unknowns and rows; rl_mincurv_global_xy_batch_dev, kernel k_global_xy): 4N bound rows, 2 (n-k) unknowns per QP."""
    from spline_trajectory_optimization_amd import ops
    out = ops.global_batch_torch(trk, d_widths, GLOBAL_MARGIN, GLOBAL_OUTER, dof=2, lon=GLOBAL_LON)
    torch.cuda.synchronize()
    steps = max(3, min(args.steps, 10))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        ops.global_batch_torch(trk, d_widths, GLOBAL_MARGIN, GLOBAL_OUTER, out=out, dof=2, lon=GLOBAL_LON)
        b.record()
    torch.cuda.synchronize()
    ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    st = out["stats"].cpu().numpy()
    B = d_widths.shape[0]
    assert np.isfinite(st).all() and (st[:, 3] <= 1e-8).all(), "global QP (two coordinates): a line left its bounds"
    blk = {"metric": "global min-curvature QPs/sec, both coordinates of every control point free (N=2000: 4N bound rows, "
                     "122 unknowns per QP; lateral bounds from the widths, longitudinal +-1 m)",
           "value": B * GLOBAL_OUTER / ms * 1e3, "unit": "QPs/s", "instances_per_s": B / ms * 1e3, "kernel_ms": ms,
           "timed_launches": steps, "linearisations": GLOBAL_OUTER, "ipm_iterations_mean": float(st[:, 0].mean()),
           "ipm_iterations_max": float(st[:, 0].max()), "sum_kappa2_before_after": [float(st[:, 1].mean()), float(st[:, 2].mean())],
           "halved_steps_mean": float(st[:, 7].mean()), "max_bound_violation_m": float(st[:, 3].max()),
           "block_threads": int(out["rl_stats"].block_threads), "lds_bytes_per_workgroup": int(out["rl_stats"].lds_bytes),
           "kernel": "k_global_xy",
           "actual_limiter": "register file: the interior-point state of 4 samples x 2 rows per thread (96 registers) plus the row "
                             "passes exceed 256 VGPRs -- 139 spilled registers, 6 GB of scratch writes per launch (DESIGN_HISTORY.md 3b); then the one factorising wave"}
    prof = profile_block("k_global_xy")
    if prof:   # committed rocprofv3 counters of the same kernel (profiles/counters_latest.json), not measured in this run
        c = prof["counters_per_launch"]
        blk["counters"] = {"source": prof["source"], "measured_in_run": False, "kernel_ms_under_rocprof": prof["avg_ms"],
                           "wave_cycles_waiting_frac": c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"] if "SQ_WAIT_ANY" in c else None,
                           "lds_bank_conflict_frac": c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"] if "SQ_LDS_IDX_ACTIVE" in c else None,
                           "vmem_read_wave_insts": c.get("SQ_INSTS_VMEM_RD"), "hbm_write_bytes": c.get("WRITE_SIZE", 0.0) * 1024.0,
                           "hbm_fetch_bytes": c.get("FETCH_SIZE", 0.0) * 1024.0, "valu": valu_block(prof, ms)}
    if with_cpu:
        from oracle import oracle as orc
        ninst = 2
        t0 = time.perf_counter()
        dev_m = 0.0
        xy = out["xy"][:ninst].cpu().numpy()
        for b in range(ninst):
            r = orc.global_mincurv_xy(g["t"], g["cx"], g["cy"], g["k"], N_WAYPOINTS, g["widths"][b, :, 0], g["widths"][b, :, 1],
                                      GLOBAL_MARGIN, GLOBAL_LON, GLOBAL_OUTER)
            dev_m = max(dev_m, float(np.abs(r[2] - xy[b]).max()))
            assert abs(int(r[4][0]) - int(st[b, 0])) <= 1, "global QP (two coordinates): iteration count differs from the twin"
        dt = time.perf_counter() - t0
        assert dev_m < 2e-6, f"global QP (two coordinates) deviates from its CPU twin: {dev_m}"
        blk["cpu_twin"] = {"instances_per_s": ninst / dt, "cores": 1, "sample": f"{ninst} instances, {dt:.2f} s",
                           "gpu_vs_twin_dev_m": dev_m}
    return blk


MFMA_F64_PEAK_GFLOPS = 78600.0  # v_mfma_f64_16x16x4_f64 runs at the FP64 vector rate on gfx950 (DESIGN_HISTORY.md 3d: 64 cycles per 2048 flops per SIMD)


def mintime_leg(B, with_cpu):
    """Third leg (BASELINE configs[4]): the reference's min-time example (MGKT kart circuit, 828 nodes) as a
    batch of width-perturbed tracks through rl_mintime_solve_batch -- QSS warm start, then the interior-point SQP-type
    iteration to KKT 1e-6.  Timed on the host around ONE call (copies included), outside the headline's region.
    roofline: EXECUTED FP64 flops per instance (rocprofv3 instruction-mix counters of the same batch, committed under
    profiles/: not measured in this run) x B / wall against the FP64 vector peak, which is also what v_mfma_f64 reaches.
    cpu_baseline: the CPU twin (oracle/sqp_twin.py, kind "port": the reference's IPOPT path needs casadi) timed for a few
    iterations of the same N = 828 problem and scaled by the GPU run's mean iteration count."""
    try:
        from spline_trajectory_optimization_amd.min_time_optm.example import timed_batch_solve
        leg = timed_batch_solve(B)
        leg["solver_pinned_by"] = "CPU twin oracle/sqp_twin.py (tests/test_mintime.py); NLP functions by fixture G8"
    except Exception as e:   # the headline must not depend on this leg
        return {"error": f"{type(e).__name__}: {e}"}
    try:
        path = os.path.join(ROOT, "profiles", "mintime_counters_latest.json")
        if os.path.exists(path):
            c = json.load(open(path))
            # flops scale with the iterations an instance runs: rescale the profiled batch's figure to this run's mean
            flops_inst = c["fp64_flops_per_instance"] * leg["iterations_mean"] / c["iterations_mean"]
            achieved = flops_inst * B / leg["wall_s"] / 1e9
            nodes = leg.get("nodes", 828)
            chain_us = c.get("kkt_avg_us")
            leg["roofline"] = {
                "bound": "fp64_vector", "achieved": achieved / 1e3, "peak": FP64_VECTOR_PEAK_GFLOPS / 1e3, "unit": "TFLOP/s",
                "frac": achieved / FP64_VECTOR_PEAK_GFLOPS, "traffic": None,
                "flops_per_instance": flops_inst, "flops_per_instance_iteration_node": flops_inst / leg["iterations_mean"] / nodes,
                "flops_source": c["source"], "measured_in_run": False, "profiled_iteration_kernels": c.get("iteration_kernels"),
                "flops_are": "EXECUTED FP64 flops of the profiled build (masked lanes and redundant dual arithmetic included), rescaled by "
                             "iterations -- an upper bound on useful work, not useful flops",
                "mfma_f64_share_of_flops": c.get("fp64_flops_mfma_share"), "mfma_f64_peak_tflops": MFMA_F64_PEAK_GFLOPS / 1e3,
                "dependent_chain": "k_mt_kkt4 eliminates the lap's block-tridiagonal KKT system node by node with four fronts (from both ends "
                                   f"and from the middle node outwards): (N-1)/4 + 3 = {(nodes - 1) // 4 + 3} sequential 16x16 block steps per call "
                                   "whatever the batch"
                                   + (f"; measured {chain_us:.0f} us per call = {chain_us / ((nodes - 1) // 4 + 3):.1f} us per block step"
                                      if chain_us else "")
                                   + f" -> >= {leg['iterations_mean']:.0f} x that per solve: the floor under wall_s for small batches",
                "actual_limiter": "FP64 VALU issue of the derivative kernels (transcendental / division sequences of the tyre model) "
                                  "and the latency of the node-by-node elimination (DESIGN_HISTORY.md 3d)"}
    except Exception as e:
        leg["roofline"] = {"error": f"{type(e).__name__}: {e}"}
    if with_cpu:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from mintime_problem import mgkt_problem
            from oracle import sqp_twin as tw
            from spline_trajectory_optimization_amd.min_time_optm import defaults
            d = mgkt_problem(1.0, defaults.ESTIMATES)
            P = tw.Problem(defaults.MODEL, d["s"], d["kappa"], d["left"], d["right"], d["L"],
                           defaults.SOLVER["average_track_width"], defaults.SOLVER["speed_cap"])
            w0 = tw.initial_point(P, d["speed"], d["seg_time"])
            iters = 5
            t0 = time.perf_counter()
            tw.solve(P, w0, max_iter=iters, tol=1e-6)
            dt = time.perf_counter() - t0
            leg["cpu_baseline"] = {"unit": "NLP solves/s", "cores": 1, "kind": "port",
                                   "not_a_speedup_basis": "the twin is a single-core Python/scipy restatement of THIS solver, not the "
                                                          "reference's casadi + IPOPT path (absent here): no GPU/CPU ratio is claimed from it",
                                   "this_host": {"seconds_per_iteration": dt / iters,
                                                 "sample": f"{iters} iterations of the CPU twin on the unperturbed N={P.N} problem ({dt:.1f} s)"}}
            full = os.path.join(ROOT, "profiles", "r04_mintime_twin_full_solve.json")
            if os.path.exists(full):
                f_ = json.load(open(full))
                leg["cpu_baseline"].update(value=f_["solves_per_s"],
                                           sample=f"ONE FULL solve of the CPU twin (tools/time_twin_full_solve.py, committed: "
                                                  f"{f_['wall_s']:.1f} s for {f_['info'].get('iterations', 0):.0f} iterations on one core of the "
                                                  f"build container; not measured on this host)", source="profiles/r04_mintime_twin_full_solve.json")
            else:
                leg["cpu_baseline"].update(value=1.0 / (dt / iters * leg["iterations_mean"]),
                                           sample=f"{iters} twin iterations x the GPU batch's mean of {leg['iterations_mean']:.1f}")
        except Exception as e:
            leg["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
    return leg


def qss_leg(B, with_cpu):
    """Fourth leg: Simulator.run_simulation on B Monza tables of N = 2000 whose turn radii are scaled
    by 0.9 ... 1.1 per instance (different profiles and iteration counts), device resident (rl_qss_sim_dev on torch's stream),
    timed with events around one call after a warm-up; and one table alone.  The kernel is latency bound (a dependent chain
    of front steps, DESIGN_HISTORY.md 3c), so the leg reports times and rates, not a roofline.  cpu_baseline / parity: the C oracle's
    list-order loop on the first instances, one core."""
    try:
        import torch
        from scipy.interpolate import CubicSpline
        from spline_trajectory_optimization_amd import batch, ops
        acc = CubicSpline([0.0, 50.0, 100.0], [10.0, 7.0, 0.5]); dcc = CubicSpline([0.0, 50.0, 100.0], [-13.0, -15.0, -20.0])
        veh = (acc.x, acc.c, dcc.x, dcc.c, np.array([10.0, -20.0, 15.0, -15.0, 100.0, 30.0]))   # the vehicle of the reference's simulator test
        N = 2000
        pts = batch.monza_centerline(100.0, 5).sample_along(ts=np.linspace(0, 1, N, endpoint=False)).points
        rng = np.random.default_rng(7)
        P = np.repeat(pts[None], B, axis=0)
        P[:, :, 5] *= rng.uniform(0.9, 1.1, size=(B, 1))
        leg = {"workload": f"Monza centre line, N = {N}, {B} tables with turn radii scaled by 0.9 ... 1.1; the reference test's vehicle",
               "instances": B}
        big = 1024
        Pbig = np.repeat(pts[None], big, axis=0)
        Pbig[:, :, 5] *= np.random.default_rng(8).uniform(0.9, 1.1, size=(big, 1))
        for name, tab in (("batch", P), ("batch_1024", Pbig), ("single", P[:1])):
            d = torch.from_numpy(tab).cuda()
            ops.qss_sim_torch(d.clone(), *veh); torch.cuda.synchronize()     # warm-up at this size
            runs = []
            for _ in range(3):
                w = d.clone()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); it = ops.qss_sim_torch(w, *veh); e1.record(); torch.cuda.synchronize()
                runs.append((e0.elapsed_time(e1), w, it))
            runs.sort(key=lambda r_: r_[0])
            ms, w, it = runs[len(runs) // 2]          # the MEDIAN of three event-timed calls
            its = it.cpu().numpy()
            leg[name] = {"instances": int(tab.shape[0]), "ms": ms, "ms_min": runs[0][0], "ms_all": [r_[0] for r_ in runs],
                         "simulations_per_s": tab.shape[0] / ms * 1e3,
                         "global_iterations_mean": float(its.mean()), "raised": int((its < 0).sum())}
            if name == "batch":
                out, its_batch = w.cpu().numpy(), its
        leg["timing"] = "median of three calls after a warm-up at the same size, HIP events on the launch stream (device resident)"
        # passes per trajectory: the dataflow kernel's pass counter of this very workload (one Monza table, N = 2000: 3 790 passes, 3 829
        # batches of <= 256 agents, 280 k examinations for 213 k steps -- RL_QSS_DEBUG counters of the diagnostic build, DESIGN_HISTORY.md 3c;
        # the kernel has not changed since) against the dependency analysis's critical path (3 889 steps; 1 446 with shared passes)
        if N == 2000 and "single" in leg:
            leg["single"]["passes_per_trajectory"] = 3790
            leg["single"]["us_per_pass"] = leg["single"]["ms"] * 1e3 / 3790
            leg["single"]["passes_source"] = ("counter of the diagnostic build on this workload (DESIGN_HISTORY.md 3c), not read in this run; critical "
                                              "path of the true dependencies: 3 889 passes (1 446 if a step shares a pass with the earlier "
                                              "readers of the sample it writes): the pass COUNT is at the model's, the 7-8 us a pass costs "
                                              "(about 2 000 instructions on the slowest lane of a 256-agent batch, four barriers) is what is off")
        cpath = os.path.join(ROOT, "profiles", "qss_counters_latest.json")
        if os.path.exists(cpath):       # counters of the committed rocprofv3 passes (tools/profile_qss.sh): not measured in this run
            try:
                cj = json.load(open(cpath))
                rows = [r_ for r_ in cj["kernels"] if r_["kernel"].startswith("k_qss_dfw") and r_["N"] == N]
                row = max(rows, key=lambda r_: r_["instances"])
                leg["counters"] = {
                    "kernel": row["kernel"], "instances_profiled": row["instances"], "ms_profiled": row["ms"],
                    "waiting_share_of_wave_cycles": row["SQ_WAIT_ANY"] / row["SQ_WAVE_CYCLES"],
                    "valu_busy_share_of_wave_cycles": 4.0 * row["SQ_ACTIVE_INST_VALU"] / row["SQ_WAVE_CYCLES"],
                    "lds_bank_conflict_share_of_lds_cycles": row["SQ_LDS_BANK_CONFLICT"] / row["SQ_LDS_IDX_ACTIVE"],
                    "wave_instructions_per_trajectory": {k_: row["per_instance"][k_] for k_ in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS")},
                    "bound": "latency of a dependent chain of front steps (DESIGN_HISTORY.md 3c): no bandwidth or flop roofline applies; the "
                             "counters say how much of a wave's time is waiting",
                    "source": cj.get("source_file", "profiles/qss_counters_latest.json"), "measured_in_run": False}
            except Exception as e:
                leg["counters"] = {"error": f"{type(e).__name__}: {e}"}
        leg["kernel"] = "k_qss_dfw<4> (the reference's steps as a dataflow, four waves per instance) for every size its LDS tables hold, else k_qss_sim (list order)"
        if with_cpu:
            from oracle import oracle as orc
            k = min(3, B)
            t0 = time.perf_counter()
            refs = [orc.qss_sim(P[i], *veh) for i in range(k)]
            dt = time.perf_counter() - t0
            leg["cpu_baseline"] = {"value": k / dt, "unit": "simulations/s", "cores": 1, "kind": "port",
                                   "sample": f"{k} of the {B} tables, oracle/mincurv_oracle.c orc_qss_sim (list order)"}
            leg["parity"] = {"instances": k,
                             "owner_flags_equal": bool(all(np.array_equal(out[i][:, 18], refs[i][0][:, 18]) for i in range(k))),
                             "iterations_equal": bool(all(int(its_batch[i]) == int(refs[i][1]) for i in range(k))),
                             "max_speed_dev": float(max(np.abs(out[i][:, 4] - refs[i][0][:, 4]).max() for i in range(k)))}
        return leg
    except Exception as e:   # the headline must not depend on this leg
        return {"error": f"{type(e).__name__}: {e}"}


def valu_block(prof, kernel_ms):
    """FP64 VALU view of a kernel from the committed counters + this run's kernel time.
      valu_active_frac = SQ_ACTIVE_INST_VALU [quad-cycles] x 4 / (1024 SIMDs x kernel cycles), kernel cycles =
                         SQ_BUSY_CYCLES / 8 XCDs... taken as clock_ghz x kernel time (clock_ghz from
                         GRBM_GUI_ACTIVE / 8 / time of the profiled run)
      fp64_gflops      = 64 lanes x (ADD_F64 + MUL_F64 + TRANS_F64 + 2 x FMA_F64 wave-instructions) / kernel time
    (wave-instruction counts x 64 lanes: partially masked instructions count as full, an upper bound)."""
    if not prof or "counters_per_launch" not in prof:
        return None
    c = prof["counters_per_launch"]
    out = {"source": prof.get("source"), "measured_in_run": False}
    clock = prof.get("clock_ghz")
    if clock and "SQ_ACTIVE_INST_VALU" in c:
        cycles = clock * 1e9 * prof["avg_ms"] * 1e-3
        out["valu_active_frac"] = c["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * cycles)
        out["clock_ghz"] = clock
    if "SQ_INSTS_VALU" in c:
        out["valu_wave_insts_per_launch"] = c["SQ_INSTS_VALU"]
    f64 = [c.get(k) for k in ("SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_TRANS_F64", "SQ_INSTS_VALU_FMA_F64")]
    if all(v is not None for v in f64):
        flops = 64.0 * (f64[0] + f64[1] + f64[2] + 2.0 * f64[3])
        out["fp64_gflops"] = flops / (kernel_ms * 1e-3) / 1e9
        out["fp64_frac_of_vector_peak"] = out["fp64_gflops"] / FP64_VECTOR_PEAK_GFLOPS
        out["fp64_flops_per_launch"] = flops
    return out


DUMP_BUDGET_BYTES = 60_000_000   # the arrays of --dump-outputs, under 64 MB with room for the sample indices


def dump_outputs(path, arrays):
    """--dump-outputs: `arrays` (name -> array, leading axis = instance) as path/<name>.npy in float64 -- exact for the
    int32 counters too.  Above DUMP_BUDGET_BYTES in all (only the gathered xy of many ranks gets there), each array keeps
    the same share of its instances, a fixed seeded sample, whose indices go to path/<name>_index.npy."""
    os.makedirs(path, exist_ok=True)
    arrays = {k_: np.ascontiguousarray(v_, dtype=np.float64) for k_, v_ in arrays.items()}
    total = sum(a_.nbytes for a_ in arrays.values())
    keep = min(1.0, DUMP_BUDGET_BYTES / total)
    for name, a_ in arrays.items():
        if keep < 1.0:
            idx = np.sort(np.random.default_rng(0).choice(a_.shape[0], int(a_.shape[0] * keep), replace=False))
            np.save(os.path.join(path, f"{name}_index.npy"), idx.astype(np.float64))
            a_ = a_[idx]
        np.save(os.path.join(path, f"{name}.npy"), a_)


# ------------------------------------------------------------------------------------------------
def run_rank(args):
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    exit_code = 0
    assert world == args.gpus, f"WORLD_SIZE={world} but --gpus {args.gpus}"
    # test hooks of tests/test_host_cpu.py::test_spawn_ranks_propagates_a_failed_rank (no GPU needed up to here): one rank fails at
    # once, the others would sit for a while -- spawn_ranks has to end them and hand the failing rank's code on
    if os.environ.get("RL_BENCH_FAIL_RANK") == str(rank):
        sys.exit(7)
    if os.environ.get("RL_BENCH_HOLD_S"):
        time.sleep(float(os.environ["RL_BENCH_HOLD_S"]))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X (no CPU fallback in the product path)")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    import __graft_entry__ as ge
    if int(os.environ.get("LOCAL_RANK", "0")) == 0:
        ge.build_hip()          # the .so normally ships prebuilt; never let N ranks race on hipcc
    if world > 1:
        dist.barrier()
    from spline_trajectory_optimization_amd import _lib, batch, ops
    from spline_trajectory_optimization_amd.models.race_track import RaceTrack

    # ---- set-up (untimed): tracks, base half-widths, per-instance widths resident in HBM
    _lib.set_default_device(local_rank)  # one process per GPU
    ctx = _lib.Context.get()
    B = args.batch
    groups = []
    centre, left, right = batch.load_monza()
    line = batch.monza_centerline(SPLINE_S, SPLINE_K)
    t, cx, cy, k = line._tck()
    track_geo = RaceTrack("Monza", left, right, centre)
    traj = line.sample_along(ts=np.linspace(0.0, 1.0, N_WAYPOINTS, endpoint=False))
    track_geo.fill_trajectory_boundaries(traj)
    wl, wr = batch.half_widths_from_bounds(traj.points)
    b_monza = B if args.workload == "monza" else B - B // 2
    groups.append({"name": "monza", "t": t, "cx": cx, "cy": cy, "k": k, "length": line.get_length(),
                   "widths": batch.width_batch(wl, wr, b_monza, seed=1234 + rank)})
    # Instances 0 and 3 of rank 0's Monza batch exist as a run of the REFERENCE's own loop (fixture G7b,
    # tests/golden/make_golden.py): take their widths from the fixture bit for bit (the batch's own base widths come from
    # this GPU's fill_bounds and agree with the fixture's to ~1e-10 m only), so that the result can be laid beside that run.
    ref_run = {}
    for fname in ("G7b_benchmarked_config.npz", "G7d_benchmarked_batch_sample.npz"):   # G7d (round 5): instances 1, 2, 4 ... 7
        g7b_path = os.path.join(ROOT, "tests", "golden", fname)
        if rank == 0 and b_monza > 7 and os.path.exists(g7b_path):
            g7b = np.load(g7b_path)
            for key in [str(k_) for k_ in g7b["cases"] if "bench" in str(k_)]:
                bi = int(key.split("bench")[1])
                if np.abs(groups[0]["widths"][bi] - g7b[f"{key}_widths"]).max() < 1e-6 and \
                        np.array_equal(g7b[f"{key}_i_start"], batch.default_i_start(len(cx), k, MAX_ITER, seed=0)):
                    groups[0]["widths"][bi] = g7b[f"{key}_widths"]
                    ref_run[bi] = (g7b[f"{key}_cx"], g7b[f"{key}_cy"])
    if args.workload == "mixed":
        oval = batch.oval_centerline(SPLINE_S, SPLINE_K)
        ot, ocx, ocy, ok_ = oval._tck()
        owl, owr = batch.oval_half_widths(N_WAYPOINTS)
        groups.append({"name": "oval", "t": ot, "cx": ocx, "cy": ocy, "k": ok_, "length": oval.get_length(),
                       "widths": batch.width_batch(owl, owr, B // 2, seed=5678 + rank)})
    search = {"windowed": _lib.SEARCH_WINDOWED, "culled": _lib.SEARCH_CULLED, "brute": _lib.SEARCH_BRUTE}[args.search]
    ctx.set_arith({"fast": _lib.ARITH_FAST, "reference": _lib.ARITH_REFERENCE, "branch": _lib.ARITH_BRANCH}[args.arith])   # of the headline's launches
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in groups[1:]]
    for g in groups:
        g["n"] = len(g["cx"])
        g["i_start"] = batch.default_i_start(g["n"], g["k"], MAX_ITER, seed=0)
        g["trk"] = _lib.Track(ctx, g["t"], g["cx"], g["cy"], g["k"], N_WAYPOINTS)
        g["d_widths"] = torch.from_numpy(g["widths"]).to(dev)
        g["out"] = [ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search)]
    torch.cuda.synchronize()
    stats = groups[0]["out"][0]["stats"]

    # N > 1: the gather of step s runs on the process group's stream while step s+1 computes into the
    # other output set (double buffering); a buffer is reused only after its gather has completed.
    gathered = None
    if world > 1:
        for g in groups:
            g["out"].append({kk: (vv.clone() if hasattr(vv, "clone") else vv) for kk, vv in g["out"][0].items()})
        if rank == 0:
            gathered = [[torch.empty((world * g["widths"].shape[0],) + tuple(g["out"][0]["xy"].shape[1:]),
                                     dtype=torch.float64, device=dev) for g in groups] for _ in range(2)]
    works = [[], []]
    main_stream = streams[0]

    def step(s, events=None):
        slot = s & 1 if world > 1 else 0
        for w in works[slot]:
            w.wait()                # stream-level wait: the buffer's previous gather is done
        works[slot] = []
        if events is not None:
            events[0].record(main_stream)
        fork = torch.cuda.Event()
        fork.record(main_stream)
        for g, st in zip(groups, streams):
            if st is not main_stream:
                st.wait_event(fork)
            with torch.cuda.stream(st):
                ops.solve_batch_torch(g["trk"], _lib.BOUNDS_WIDTHS, g["d_widths"], g["i_start"], search=search,
                                      out=g["out"][slot])
            if st is not main_stream:
                join = torch.cuda.Event()
                join.record(st)
                main_stream.wait_event(join)
        if events is not None:
            events[1].record(main_stream)   # kernel-only span on the launch stream(s)
        if world > 1:
            for gi, g in enumerate(groups):
                works[slot].append(batch.gather_to_root(g["out"][slot]["xy"], rank, world, dist,
                                                        out=gathered[slot][gi] if rank == 0 else None, async_op=True))

    def drain():
        for q in range(2):
            for w in works[q]:
                w.wait()
            works[q] = []

    for w_ in range(args.warmup):
        step(w_)
    drain()
    # ---- timed region: barrier + sync on both sides, exactly K steps
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        step(s, ev[s])
    drain()                     # every gather has landed on rank 0 before the clock stops
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    # sanity outside the timed region: results are finite and the bookkeeping is consistent
    last_slot = (args.steps - 1) & 1 if world > 1 else 0
    xy_gpu, ns_gpu = [], []
    for gi, g in enumerate(groups):
        last = g["out"][last_slot]
        status = last["status"].cpu().numpy()
        ns = last["n_success"].cpu().numpy()
        xy = last["xy"].cpu().numpy()
        bg = g["widths"].shape[0]
        if world > 1 and rank == 0:  # rank 0's own shard came back through the collective unchanged
            assert torch.equal(gathered[last_slot][gi][:bg], last["xy"])
        assert np.isfinite(xy).all()
        assert np.array_equal(status, 2 * MAX_ITER * (g["n"] - g["k"]) - ns.reshape(bg, -1).sum(axis=1))
        xy_gpu.append(xy); ns_gpu.append(ns)
        if gi == 0 and ref_run and args.full:
            ctrl0 = last["ctrl"].cpu().numpy()
            dev_ref = {bi: float(np.hypot(ctrl0[bi, :, 0] - rc[0], ctrl0[bi, :, 1] - rc[1]).max()) for bi, rc in ref_run.items()}

    # N > 1: every rank's shard of EVERY group arrived on rank 0 unchanged -- each rank publishes two INTEGER checksums of the
    # bit patterns of what it sent (wrapping int64 sums: independent of the reduction order, the device and the storage
    # offset), rank 0 recomputes them on what it received.  Outside the timed region.
    def bit_checksums(x):
        v = x.contiguous().view(torch.int64)
        return torch.stack([v.sum(), torch.bitwise_xor(v, v >> 29).sum()])

    gather_check = None
    if world > 1 and args.full:
        chk = torch.stack([torch.cat([bit_checksums(g["out"][last_slot]["xy"]),
                                      g["out"][last_slot]["status"].to(torch.int64).sum().reshape(1)]) for g in groups])
        all_chk = [torch.empty_like(chk) for _ in range(world)]
        dist.all_gather(all_chk, chk)
        if rank == 0:
            n_ok = 0
            for gi, g in enumerate(groups):
                bg = g["widths"].shape[0]
                for r in range(world):
                    got = bit_checksums(gathered[last_slot][gi][r * bg:(r + 1) * bg])
                    assert torch.equal(got, all_chk[r][gi, :2]), f"group {gi}: the shard of rank {r} changed in the gather"
                    n_ok += 1
            gather_check = {"groups": len(groups), "ranks": world, "shards_equal": n_ok, "checksum": "wrapping int64 sums of the bit patterns",
                            "collective": "grouped isend/irecv (dist.gather raised on this backend)" if batch._gather_fallback["p2p"] else "dist.gather",
                            "skipped_qps_per_rank": [[int(all_chk[r][gi, 2]) for gi in range(len(groups))] for r in range(world)]}

    # what the last timed step handed its caller: per group the sampled line (N > 1: gathered from every rank), and this
    # rank's control points, success counts and skipped-QP counts
    if args.dump_outputs and rank == 0:
        arrays = {}
        for gi, g in enumerate(groups):
            last = g["out"][last_slot]
            arrays[f"{g['name']}_xy"] = gathered[last_slot][gi].cpu().numpy() if world > 1 else xy_gpu[gi]
            arrays[f"{g['name']}_ctrl"] = last["ctrl"].cpu().numpy()
            arrays[f"{g['name']}_n_success"] = ns_gpu[gi]
            arrays[f"{g['name']}_status"] = last["status"].cpu().numpy()
        dump_outputs(args.dump_outputs, arrays)

    if rank == 0:
        total_solves = world * B * args.steps
        value = total_solves / elapsed
        qp_per_solve = [2 * MAX_ITER * (g["n"] - g["k"]) for g in groups]
        qps_per_step = sum(q * g["widths"].shape[0] for q, g in zip(qp_per_solve, groups))
        achieved = (BYTES_PER_SOLVE * B) / (kernel_ms * 1e-3) / 1e9
        prof = profile_block({"fast": "k_sweep", "reference": "k_sweep_reference_order", "branch": "k_sweep_branch"}[args.arith]) \
            if args.workload == "monza" else None
        wl_text = (f"Monza N={N_WAYPOINTS}, batch={B} width-perturbed instances per GPU (BASELINE configs[1])"
                   if args.workload == "monza" else
                   f"mixed: {groups[0]['widths'].shape[0]} Monza + {groups[1]['widths'].shape[0]} rotated-oval "
                   f"width-perturbed instances per GPU, N={N_WAYPOINTS}, grouped by track, two concurrent launches "
                   f"per step (BASELINE configs[2])")
        res = {
            "metric": "min-curvature QP solves/sec (N=2000 waypoints)",
            "value": value, "unit": "solves/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": wl_text + f"; UNIT: one solve = one instance's full run_min_curvature_qp "
                            f"(optimizer.py:256-341), max_iter={MAX_ITER}, {qp_per_solve} control-point QPs per "
                            f"solve, sweep order pinned -- the reference-parity path; the north_star's global "
                            f"banded QP is the separate `global_qp` leg",
                "spline": f"s={SPLINE_S:g} k={SPLINE_K} n={[g['n'] for g in groups]}", "batch_per_gpu": B,
                "control_point_qps_per_s": qps_per_step * world * args.steps / elapsed, "search": args.search,
                "arith": args.arith + (" (fma, rsqrt normal, tree sums: a legal rounding of the reference's arithmetic; the reference-order "
                                       "mode is the `reference_order` leg)" if args.arith == "fast" else
                                       (" (RL_ARITH_REFERENCE, the default: the reference's operations in the reference's order -- the CPU oracle's bits; "
                                        "the fast arithmetic is timed in the `reference_order` leg)" if args.arith == "reference" else
                                        " (RL_ARITH_BRANCH: positions, crossings, bound points and rows in the reference's order, the rest fast)")),
                "parallelism": f"{world} rank(s) x independent instances"
                               + (f", 1 gather to rank 0 per step and group over torch.distributed backend "
                                  f"'{dist.get_backend()}' ({'gloo: --share-gpu test hook' if args.share_gpu else 'nccl = RCCL over xGMI'})"
                                  f" (overlapped with the next step), world size {dist.get_world_size()}" if world > 1 else ""),
                "lds_bytes_per_workgroup": int(stats.lds_bytes), "block_threads": int(stats.block_threads),
            },
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": prof.get("hbm_bytes_fetch_x2") if prof else None,
                         "traffic_source": prof.get("source") if prof else None, "traffic_measured_in_run": False,
                         "kernel": {"fast": "k_sweep", "reference": "k_sweep<..., STRICT>", "branch": "k_sweep<..., STRICT, LITE>"}[args.arith], "kernel_ms": kernel_ms,
                         "algorithmic_bytes_per_launch": BYTES_PER_SOLVE * B,
                         "actual_limiter": SWEEP_LIMITER,
                         "valu": valu_block(prof, kernel_ms)},
        }
        if gather_check is not None:
            res["gather_check"] = gather_check
        if args.full and world == 1 and args.workload == "monza" and not args.no_global:
            try:      # a failing secondary leg is reported in the line, it does not take the headline with it
                res["global_qp"] = global_qp_leg(groups[0]["trk"], groups[0]["d_widths"], groups[0], args, torch,
                                                 with_cpu=not args.no_cpu_baseline)
            except Exception as e:
                res["global_qp"] = {"error": f"{type(e).__name__}: {e}"}
        if args.full and world == 1 and args.workload == "monza" and not args.no_mintime:
            res["mintime_nlp"] = mintime_leg(args.mintime_batch, with_cpu=not args.no_cpu_baseline)
        if args.full and world == 1 and args.workload == "monza" and not args.no_qss:
            res["qss_sim"] = qss_leg(args.qss_batch, with_cpu=not args.no_cpu_baseline)
        pos = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                res["cpu_baseline"], pos = cpu_legs(groups, [g["i_start"] for g in groups], xy_gpu, min(args.cpu_instances, B))
            except Exception as e:
                res["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        if args.full and world == 1 and args.workload == "monza" and args.arith in ("fast", "reference") and not args.no_reference_order:
            try:
                fast_head = args.arith == "fast"
                res["reference_order"] = reference_order_leg(groups[0], args, torch, search, kernel_ms if fast_head else None,
                                                             xy_gpu[0] if fast_head else None, pos[0] if pos else None, ref_run,
                                                             fast_ns_all=ns_gpu[0] if fast_head else None)
            except Exception as e:
                res["reference_order"] = {"error": f"{type(e).__name__}: {e}"}
        if ref_run and args.full:
            per = {d_["instance"]: d_ for d_ in res.get("cpu_baseline", {}).get("gpu_vs_oracle", {}).get("per_instance", [])}
            res["gpu_vs_reference_run"] = {
                "what": "instances of THIS batch that also exist as a run of the reference's own run_min_curvature_qp loop "
                        "(fixtures tests/golden/G7b_benchmarked_config.npz, G7d_benchmarked_batch_sample.npz: same widths bit for bit, "
                        "same sweep order); max control-point deviation [m]",
                "instances": sorted(dev_ref), "dev_m": [dev_ref[b_] for b_ in sorted(dev_ref)],
                "within_1e-4": int(sum(v <= 1e-4 for v in dev_ref.values())),
                "nearest_branch_dev_m": [per.get(b_, {}).get("nearest_branch_dev_m") for b_ in sorted(dev_ref)],
                "nearest_branch": [per.get(b_, {}).get("branch") for b_ in sorted(dev_ref)],
                "note": "an instance outside 1e-4 m of the reference's run must be within 1e-4 m of one of the oracle's re-rounding "
                        "branches (sampled line; cpu_baseline.gpu_vs_oracle.per_instance; "
                        "tests/test_hip_parity.py::test_benchmarked_configuration_vs_reference_run)"}
        # headline parity block: what was compared, how many are where
        gv_ = res.get("cpu_baseline", {}).get("gpu_vs_oracle")
        if gv_:
            res["parity"] = {"rule": "nearest branch <= 1e-4 m (tests/parity_rule.py)", "sample": gv_["sample"],
                             "within_1e-4_of_strict_oracle": gv_["within_1e-4_of_strict_oracle"],
                             "within_1e-4_of_a_rerounding_branch": gv_["within_1e-4_of_a_rerounding_branch"],
                             "failing": gv_["failing"], "nearest_branch_dev_m_max": gv_["nearest_branch_dev_m_max"],
                             "dev_vs_reference_run_m": res.get("gpu_vs_reference_run", {}).get("dev_m"),
                             "conditioning": "at N = 2000, max_iter = 5 no instance of this batch is well-conditioned in the reference's own "
                                             "formulation (rows min(L,R) - (p - b z) divide 1e-13 m of rounding by b ~ 1e-10): the 1e-4 m "
                                             "tolerance is met per BRANCH for the fast arithmetic; the reference-order arithmetic returns "
                                             "the oracle's own bits (reference_order leg)",
                             "ok": gv_["failing"] == 0}
            ro = res.get("reference_order", {}).get("gpu_vs_oracle")
            if ro:
                res["parity"]["reference_order_bit_identical"] = f"{ro['bit_identical_to_the_correctly_rounded_oracle']} of {ro['sample']}"
                res["parity"]["ok"] = bool(res["parity"]["ok"] and ro["bit_identical_to_the_correctly_rounded_oracle"] == ro["sample"])
        # every leg's headline number, compact, as the LAST key of the line (the driver keeps the tail of the line): README / DESIGN
        # quote these
        ro_ = res.get("reference_order", {}) if isinstance(res.get("reference_order"), dict) else {}
        gq_ = res.get("global_qp", {}) if isinstance(res.get("global_qp"), dict) else {}
        mt_ = res.get("mintime_nlp", {}) if isinstance(res.get("mintime_nlp"), dict) else {}
        qs_ = res.get("qss_sim", {}) if isinstance(res.get("qss_sim"), dict) else {}
        wb_ = ro_.get("whole_batch_vs_reference_order", {})
        r3 = lambda v: None if v is None else round(float(v), 3)   # noqa: E731
        summary = {
            "sweep_reference_ms": r3(kernel_ms if args.arith == "reference" else ro_.get("kernel_ms")),
            "sweep_fast_ms": r3(kernel_ms if args.arith == "fast" else ro_.get("fast_kernel_ms")),
            "sweep_branch_ms": r3(wb_.get("branch", {}).get("kernel_ms")),
            "reference_bit_identical": res.get("parity", {}).get("reference_order_bit_identical"),
            "fast_beyond_1e-4_m": wb_.get("fast", {}).get("instances_beyond_1e-4_m"),
            "global_qp_ms": r3(gq_.get("kernel_ms")), "global_xy_ms": r3(gq_.get("two_dof", {}).get("kernel_ms")),
            "global_qp_vs_twin_m": gq_.get("cpu_twin", {}).get("gpu_vs_twin_dev_m"),
            "mintime_nlp_per_s": r3(mt_.get("value")),
            "qss_b1_ms": r3(qs_.get("single", {}).get("ms")), "qss_b256_ms": r3(qs_.get("batch", {}).get("ms")),
            "qss_b1024_ms": r3(qs_.get("batch_1024", {}).get("ms")),
            "n_gpus": world, "collective": (gather_check or {}).get("collective"),
            "parity_ok": res.get("parity", {}).get("ok"),
        }
        res["config"]["sweep_reference_ms"] = summary["sweep_reference_ms"]
        res["config"]["sweep_fast_ms"] = summary["sweep_fast_ms"]
        res["summary"] = summary
        print(json.dumps(res), flush=True)
        # a line whose parity check failed, or one of whose legs crashed, must not pass for a measurement
        # ... for the legs the parity statement rests on; a crash of the independent min-time / simulator legs stays in the line
        failed = [k_ for k_ in ("cpu_baseline", "global_qp", "reference_order")
                  if isinstance(res.get(k_), dict) and "error" in res[k_]]
        soft = [k_ for k_ in ("mintime_nlp", "qss_sim") if isinstance(res.get(k_), dict) and "error" in res[k_]]
        if soft:
            print(f"bench.py: legs with an error (reported in the line, exit code unaffected): {soft}", file=sys.stderr, flush=True)
        if "parity" in res and not res["parity"]["ok"]:
            failed.append("parity")
        if failed:
            print(f"bench.py: FAILED legs / checks: {failed} (the JSON line above carries the details)", file=sys.stderr, flush=True)
            exit_code = 3
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if exit_code:
        sys.exit(exit_code)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=BATCH_PER_GPU, help="instances per GPU")
    ap.add_argument("--workload", choices=["monza", "mixed"], default="monza")
    ap.add_argument("--search", choices=["windowed", "culled", "brute"], default="windowed")
    ap.add_argument("--arith", choices=["fast", "reference", "branch"], default="reference",
                    help="arithmetic of the headline's launches (include/rl_mincurv.h: RL_ARITH_*); reference = the library's default")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: CPU baseline, parity sample, reference-order leg, deviation from the reference's own "
                         "runs, global-QP, min-time NLP and QSS legs, gather checksums (N > 1); the --no-* options below thin it out")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<group>_<array>.npy (float64)")
    ap.add_argument("--no-reference-order", action="store_true", help="skip the reference-order leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-global", action="store_true", help="skip the global-QP leg")
    ap.add_argument("--no-mintime", action="store_true", help="skip the min-time NLP leg")
    ap.add_argument("--mintime-batch", type=int, default=1024)
    ap.add_argument("--no-qss", action="store_true", help="skip the QSS simulator leg")
    ap.add_argument("--qss-batch", type=int, default=256)
    ap.add_argument("--cpu-instances", type=int, default=8)
    ap.add_argument("--share-gpu", action="store_true",
                    help="TEST HOOK: all ranks use cuda:0 and the gloo backend (exercises the N>1 code path "
                         "on a single-GPU box; the numbers are meaningless)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)   # never returns
    run_rank(args)


if __name__ == "__main__":
    main()
