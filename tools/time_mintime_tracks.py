#!/usr/bin/env python3
"""Timing of the min-time solve with one centre line per instance (include/rl_mincurv.h: rl_mintime_solve_tracks) on the
README's batch size: MGKT at 1 m (N = 828), B = 1024.  ONE run on one MI355X; host calls timed on the wall clock (copies of the
guess and of the solution included), one warm-up at the full batch size first, --repeats timed calls per leg, their median /
min / max.  Every leg records how many instances converged and the mean iteration count.
  (a) --compare-lib OTHER.so: the shared-model entry, the vehicles entry (B rows of MODEL) and the tracks entry (B equal
      tracks, as in (b)) on this build and on another build of the library (the parent commit's), in child processes that
      alternate, --rounds each; "not slower" = this build's median of rounds lies inside the range the other build's rounds
      show by themselves, which is stated, as is whether it lies below their largest plus that range;
  (b) B equal tracks and one model through the new entry (T = B, track_of = NULL) against the shared-model entry on the same
      width-perturbed batch: the same bits, the ratio of the medians;
  (c) B uniformly scaled copies of the circuit (0.8 x .. 1.25 x: s, L, the distances and average_track_width times f, kappa /
      f; guess: the QSS profile with speeds and times times sqrt f, a corner's lateral acceleration kept), one vehicle, in one
      call against the loop of single shared-model calls it replaces (--baseline of the B, scaled);
  (d) 4 tracks (0.8 x, 1 x, 1.25 x and the mirror image) x 256 vehicles (16 grip x 16 power levels) in one call against four
      vehicles calls of 256.
Prints one JSON line and writes it to --out.

    python tools/time_mintime_tracks.py [--out profiles/mintime_tracks/time_mintime_tracks.json] [--compare-lib PARENT.so]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
from time_mintime_vehicles import MAX_ITER, TOL, grid_models, load_package, report, timed  # noqa: E402


def scaled_track(prob, f):
    """The problem data of the circuit scaled by f about the origin, and the guess for it."""
    r = np.sqrt(f)
    X0 = prob.X0.copy(); X0[:, 0] = prob.s * f; X0[:, 5] = prob.X0[:, 5] * r
    return dict(s=prob.s * f, kappa=prob.kappa / f, track_length=prob.track_length * f, left=prob.left * f, right=prob.right * f,
                average_track_width=prob.average_track_width * f, speed_cap=prob.speed_cap, X0=X0, U0=prob.U0, T0=prob.T0 * r)


def mirrored_track(prob):
    return dict(s=prob.s, kappa=-prob.kappa, track_length=prob.track_length, left=-prob.right, right=-prob.left,
                average_track_width=prob.average_track_width, speed_cap=prob.speed_cap, X0=prob.X0, U0=prob.U0, T0=prob.T0)


def same_bits(a, b):
    return bool(all(np.array_equal(x, y) for x, y in zip(a, b)))


def compare(a, _lib, res):
    """(a) the existing entries, this build against another: child processes that alternate, a.rounds each."""
    rounds = {"this": [], "other": []}
    pair = (("other", a.compare_lib), ("this", _lib.LIB_PATH))
    for r in range(a.rounds):
        for who, lib in (pair if a.first == "other" else pair[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--existing-only", "--B", str(a.B),
                                  "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise RuntimeError(f"child on {lib} failed ({out.returncode}): {out.stderr[-800:]}")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("EXISTING ")][-1]
            rounds[who].append(json.loads(line[len("EXISTING "):]))
            print(f"round {r} {who}: {rounds[who][-1]}", file=sys.stderr, flush=True)
    order = "other, this, other, this, ..." if a.first == "other" else "this, other, this, other, ..."
    cmp = {"rounds": a.rounds, "order": order, "this": rounds["this"], "other": rounds["other"]}
    for entry in ("shared", "vehicles", "tracks"):
        mine = [r[entry]["median_s"] for r in rounds["this"]]; theirs = [r[entry]["median_s"] for r in rounds["other"]]
        cmp[entry] = {"this_median_of_rounds_s": float(np.median(mine)), "other_median_of_rounds_s": float(np.median(theirs)),
                      "other_min_s": float(min(theirs)), "other_max_s": float(max(theirs)),
                      "margin_s": float(max(theirs) - min(theirs)),
                      "this_within_other_range": bool(np.median(mine) <= max(theirs)),
                      "this_within_other_max_plus_margin": bool(np.median(mine) <= 2 * max(theirs) - min(theirs))}
    res["a_existing_entries_this_build_vs_other" + ("" if a.first == "other" else "_this_first")] = cmp
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mintime_tracks", "time_mintime_tracks.json"))
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", type=int, default=8)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--first", choices=["other", "this"], default="other", help="which build opens every round of (a)")
    ap.add_argument("--compare-only", action="store_true", help="leg (a) alone, added to the JSON that --out already holds")
    ap.add_argument("--lib", default=None, help="child mode: the two existing entries on this library, JSON on stdout")
    ap.add_argument("--existing-only", action="store_true")
    a = ap.parse_args()
    _lib = load_package(a.lib)
    if a.compare_only:
        res = json.load(open(a.out))
        compare(a, _lib, res)
        print(json.dumps(res))
        return
    import torch
    from spline_trajectory_optimization_amd import ops
    from spline_trajectory_optimization_amd.min_time_optm import example
    prob = example.mgkt_problem()
    B = a.B
    left, right = example.perturbed_widths(prob, B)
    kw = dict(max_iter=MAX_ITER, tol=TOL)
    prob.solve_batch(left[:2], right[:2], max_iter=8)          # module load, kernels resident
    shared_t, shared = timed(lambda: prob.solve_batch(left, right, **kw), a.repeats)
    if a.existing_only:
        veh_t, veh = timed(lambda: prob.solve_batch(left, right, models=[prob.model] * B, **kw), a.repeats)
        trk_t, trk = timed(lambda: prob.solve_batch(left, right, tracks=[prob] * B, **kw), a.repeats)   # T = B, track_of = NULL, as in (b)
        print("EXISTING " + json.dumps({"shared": dict(shared_t, **report(shared[3])), "vehicles": dict(veh_t, **report(veh[3])),
                                        "tracks": dict(trk_t, **report(trk[3]))}))
        return
    res = {"B": B, "N": int(prob.N), "repeats": a.repeats, "max_iter": MAX_ITER, "tol": TOL, "device": torch.cuda.get_device_name(0),
           "timed": "host calls on the wall clock, host<->device copies of guess and solution included; one warm-up per leg first"}

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:      # (kept if a later leg fails)
            json.dump(res, f, indent=1)
            f.write("\n")

    # (b) equal tracks and models through the new entry
    same_track = [prob] * B
    equal_t, equal = timed(lambda: prob.solve_batch(left, right, tracks=same_track, **kw), a.repeats)
    res["b_equal_tracks_against_the_shared_entry"] = {
        "batch": "B width-perturbed MGKT tracks (example.perturbed_widths), T = B copies of the centre line, one model, track_of = NULL",
        "shared_entry": shared_t, "tracks_entry": equal_t, "tracks_over_shared_median": equal_t["median_s"] / shared_t["median_s"],
        "bit_identical": same_bits(shared, equal), "result": report(equal[3])}
    dump()
    # (c) B scaled copies, one vehicle
    fs = np.linspace(0.8, 1.25, B)
    tr = [scaled_track(prob, f) for f in fs]
    stack = lambda k: np.stack([t[k] for t in tr])  # noqa: E731
    Lc, Rc, Xc, Uc, Tc = stack("left"), stack("right"), stack("X0"), stack("U0"), stack("T0")
    scal_t, scal = timed(lambda: prob.solve_batch(Lc, Rc, Xc, Uc, Tc, tracks=tr, **kw), a.repeats)
    nb = min(a.baseline, B)
    pick = np.linspace(0, B - 1, nb).astype(int)
    single = lambda b: ops.mintime_solve_batch(prob.model, tr[b]["s"], tr[b]["kappa"], tr[b]["left"], tr[b]["right"], prob.margin,  # noqa: E731
                                               tr[b]["track_length"], Xc[b][None], Uc[b][None], Tc[b][None],
                                               tr[b]["average_track_width"], tr[b]["speed_cap"], **kw)
    same = all(all(np.array_equal(x[0], y[b]) for x, y in zip(single(b), scal)) for b in pick)     # (also the warm-up)
    t0 = time.perf_counter()
    for b in pick:
        single(b)
    dt = time.perf_counter() - t0
    conv = scal[3][:, 5] == 1
    res["c_scaled_copies_one_vehicle"] = {
        "tracks": "B copies of the circuit scaled by f = 0.8 .. 1.25 (linspace): s, L, distances, average_track_width x f, kappa / f; "
                  "guess: the QSS profile with speeds and times x sqrt f",
        "one_call": scal_t, "result": report(scal[3]),
        "lap_s_at_f": {f"{fs[b]:.4f}": float(scal[3][b, 4]) for b in pick},
        "not_converged_f": [float(f) for f in fs[~conv]][:32],
        "single_calls": {"tracks_timed": nb, "wall_s_per_track": dt / nb, "wall_s_scaled_to_B": dt / nb * B,
                         "bit_identical_to_the_one_call": bool(same)},
        "one_call_speedup_over_the_loop": dt / nb * B / scal_t["median_s"], "solves_per_s": B / scal_t["median_s"]}
    dump()
    # (d) 4 tracks x B / 4 vehicles against four vehicles calls
    nv = B // 4
    side = int(round(np.sqrt(nv)))
    ms = grid_models(prob.model, side, side)[:nv]
    nv = len(ms)
    four = [scaled_track(prob, 0.8), scaled_track(prob, 1.0), scaled_track(prob, 1.25), mirrored_track(prob)]
    of = np.repeat(np.arange(4), nv)
    per = lambda k: np.stack([four[t][k] for t in of])  # noqa: E731
    Ld, Rd, Xd, Ud, Td = per("left"), per("right"), per("X0"), per("U0"), per("T0")
    tv_t, tv = timed(lambda: prob.solve_batch(Ld, Rd, Xd, Ud, Td, models=ms * 4, tracks=four, track_of=of, **kw), a.repeats)

    def four_calls():
        out = []
        for t, d in enumerate(four):
            sl = slice(t * nv, (t + 1) * nv)
            out.append(ops.mintime_solve_vehicles(ms, d["s"], d["kappa"], Ld[sl], Rd[sl], prob.margin, d["track_length"], Xd[sl], Ud[sl],
                                                  Td[sl], d["average_track_width"], d["speed_cap"], **kw))
        return [np.concatenate([o[i] for o in out]) for i in range(4)]
    fc_t, fc = timed(four_calls, a.repeats)
    res["d_four_tracks_times_vehicles"] = {
        "batch": f"tracks: the circuit x 0.8, x 1, x 1.25 and its mirror image; vehicles: {side} grip levels mu x 0.7 .. 1.1 by {side} "
                 f"power levels Pmax x 0.6 .. 1.2 of MODEL; {4 * nv} instances, track-major",
        "one_call": tv_t, "four_vehicles_calls": fc_t, "four_calls_over_one_call_median": fc_t["median_s"] / tv_t["median_s"],
        "bit_identical": same_bits(tv, fc), "result": report(tv[3]),
        "result_per_track": [report(tv[3][t * nv:(t + 1) * nv]) for t in range(4)], "solves_per_s": 4 * nv / tv_t["median_s"]}
    dump()
    if a.compare_lib:
        compare(a, _lib, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
