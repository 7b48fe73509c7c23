"""The MGKT kart circuit (fixture G14, tests/kart_cases.py) on the CPU: the oracle against the reference's own runs on it, the
assertion that these inputs ARE the regime tests/test_kart_track_gpu.py is about (hairpins, a ring search that loses its
certificate, failing steps), and the oracle's own invariances under ring orientation and start vertex."""
import numpy as np
import pytest

import kart_cases as kc
from oracle import oracle as orc

N_STEPS = lambda n: n - 5       # noqa: E731  free control points = steps per pass (optimizer.py:296-302)


def test_g14_reference_runs():
    """Fixture G14: the reference's own run_min_curvature_qp (N = 400) and run_joint_min_curvature_qp (N = 200) loops on the
    kart circuit, one outer iteration from a pinned start index.  The rule of test_g7_run_min_curvature_qp: equal success
    counts, the line within 1e-6 m.  Measured: 3.5e-11 m (sweep), 1.6e-11 m (sliding window)."""
    g = kc.fixture()
    t, cx, cy, k, length, ringL, ringR = kc.case("base")
    for line in g["meta"]:
        print("G14 meta:", line)
    ocx, ocy, pts, ns = orc.run_min_curvature_qp(t, cx, cy, k, length, 400, ringL, ringR, g["single_N400_i_start"])
    dev = float(np.hypot(ocx - g["single_N400_cx"], ocy - g["single_N400_cy"]).max())
    dxy = float(np.hypot(*(pts[:, :2] - g["single_N400_xy"]).T).max())
    print(f"G14 sweep N=400: oracle vs the reference's run, control points {dev:.2e} m, samples {dxy:.2e} m; successes {ns.tolist()}")
    np.testing.assert_array_equal(ns, g["single_N400_n_success"])
    assert dev < 1e-6 and dxy < 1e-6
    assert np.hypot(ocx - cx, ocy - cy).max() > 1.0      # the line really moved
    jcx, jcy, jpts, jns = orc.run_joint_min_curvature_qp(t, cx, cy, k, length, 200, ringL, ringR, g["joint_N200_i_start"])
    jdev = float(np.hypot(jcx - g["joint_N200_cx"], jcy - g["joint_N200_cy"]).max())
    jdxy = float(np.hypot(*(jpts[:, :2] - g["joint_N200_xy"]).T).max())
    print(f"G14 sliding window N=200: oracle vs the reference's run, control points {jdev:.2e} m, samples {jdxy:.2e} m; "
          f"windows {jns.tolist()}")
    assert int(g["joint_N200_n_other_exceptions"]) == 0
    assert int(jns.sum()) == int(g["joint_N200_n_ok"])
    assert jdev < 1e-6 and jdxy < 1e-6
    assert float(g["single_N400_oracle_fma_dev_m"]) < 1e-6 and float(g["joint_N200_oracle_fma_dev_m"]) < 1e-6


def test_the_inputs_are_the_regime():
    g = kc.fixture()
    t, cx, cy, k, length, ringL, ringR = kc.case("base")
    assert len(cx) == 68 and len(kc.case("driven_backwards")[1]) == 72
    assert (len(ringL), len(ringR)) == (426, 412) and len(ringL) % kc.CHUNK != 0 and len(ringR) % kc.CHUNK != 0
    pts = kc.centre_table("base", 400)
    print(f"min turn radius {pts[:, 5].min():.3f} m; track length {length:.1f} m")
    assert pts[:, 5].min() < 8.0
    for name, ring, cols in (("left", ringL, (9, 10)), ("right", ringR, (11, 12))):
        share, sep_min = kc.uncertified_share(pts, ring, cols)
        print(f"{name} ring: {share:.4f} of the N = 400 samples fail sep[ce] > 2 d; smallest sep {sep_min:.3f} m")
        assert share >= 0.05
    i_start = kc.i_start("base", 2)
    for N in (400, 1000):
        _, _, _, ns = orc.run_min_curvature_qp(t, cx, cy, k, length, N, ringL, ringR, i_start)
        share = ns.sum() / (ns.size * N_STEPS(len(cx)))
        print(f"N = {N}: successes {ns.ravel().tolist()}, share {share:.4f}")
        assert 0.9 <= share < 1.0
    # the scaled copy: every +-100 m normal spans the whole track
    ts = kc.case("small")
    assert np.ptp(ts[5], axis=0).max() < 100.0 and abs(ts[4] - 103.6) < 0.05
    # every case's pinned sweep order holds a failing step at N = 400 (what the GPU tests assert of their runs)
    for name in kc.NAMES:
        t, cx, cy, k, length, ringL, ringR = kc.case(name)
        _, _, _, ns = orc.run_min_curvature_qp(t, cx, cy, k, length, 400, ringL, ringR, kc.i_start(name, 2))
        assert 0.9 <= ns.sum() / (ns.size * N_STEPS(len(cx))) < 1.0, (name, ns.tolist())


@pytest.mark.parametrize("variant", ["strict", "cr"])
def test_ring_orientation_and_start_vertex(variant):
    """Rolling the rings' start vertex changes nothing an edge computes: the bits of `base`.  Reversing them takes every edge
    the other way, which rounds differently: the line of `base` within 1e-12 m (measured 2.9e-14 m)."""
    import contextlib
    with (orc.cr_variant() if variant == "cr" else contextlib.nullcontext()):
        runs = {}
        for name in ("base", "rings_rolled", "rings_reversed"):
            t, cx, cy, k, length, ringL, ringR = kc.case(name)
            runs[name] = orc.run_min_curvature_qp(t, cx, cy, k, length, 400, ringL, ringR, kc.i_start(name, 2))
    base = runs["base"]
    for q in range(4):
        np.testing.assert_array_equal(runs["rings_rolled"][q], base[q])
    rev = runs["rings_reversed"]
    dev = max(float(np.hypot(rev[0] - base[0], rev[1] - base[1]).max()), float(np.hypot(*(rev[2][:, :2] - base[2][:, :2]).T).max()))
    print(f"rings reversed vs base ({variant}): {dev:.2e} m; bit-equal: {np.array_equal(rev[0], base[0])}")
    np.testing.assert_array_equal(rev[3], base[3])
    assert dev <= 1e-12


def test_replay_noise_share_of_the_oracle_trajectory():
    """The MGKT row of tests/test_sweep_replay.py (N = 200, B = 8, two outer iterations, 4 recorded instances) holds the share of
    steps its noise-radius rule excuses to 5 %.  That the INPUTS allow it is checked here without a kernel: the oracle's own
    trajectory of the same instances, taken step by step through orc.replay_steps (which must end on orc.solve_width_batch's
    control points, bit for bit), is judged by the same rule."""
    from test_sweep_replay import MGKT_WIDTH_SEED, NOISE_SHARE_MAX, noisy_verdict
    N, B, max_iter, n_inst = 200, 8, 2, 4
    t, cx0, cy0, k, length, _, _ = kc.case("base")
    n = len(cx0)
    widths = kc.widths("base", N, B, MGKT_WIDTH_SEED)
    i_start = kc.i_start("base", max_iter)
    octrl, _, ons = orc.solve_width_batch(t, cx0, cy0, k, length, N, widths[:n_inst], i_start)
    order = []
    for it in range(max_iter):
        for p in range(2):
            for s in range(n - k):
                kk = (s if p == 0 else (n - k) - s) + int(i_start[it])
                order.append(kk - (n - 3) + 2 if kk >= n - 3 else kk)
    noisy = failed = 0
    for b in range(n_inst):
        ringL, ringR = orc.width_rings(t, cx0, cy0, k, N, widths[b])
        cx, cy = cx0.copy(), cy0.copy()
        for kk in order:
            rep = orc.replay_steps(t, k, N, ringL, ringR, np.array([kk], dtype=np.int32), cx[None], cy[None], nthreads=1)
            noisy += int(noisy_verdict(rep)[0])
            if int(rep[0, 0]) == 0:
                cx[kk], cy[kk] = rep[0, 9:11]
                cx[0], cy[0] = cx[n - 5], cy[n - 5]; cx[1], cy[1] = cx[n - 4], cy[n - 4]              # optimizer.py:281-285
                cx[n - 3], cy[n - 3] = cx[2], cy[2]; cx[n - 2], cy[n - 2] = cx[3], cy[3]; cx[n - 1], cy[n - 1] = cx[4], cy[4]
            else:
                failed += 1
        np.testing.assert_array_equal(cx, octrl[b, :, 0]); np.testing.assert_array_equal(cy, octrl[b, :, 1])
    steps = n_inst * len(order)
    print(f"oracle trajectory, MGKT widths seed {MGKT_WIDTH_SEED}: {noisy} of {steps} steps inside the noise radius "
          f"({noisy / steps:.4f}); {failed} failed steps")
    assert failed == steps - int(ons.sum()) and failed > 0
    assert noisy / steps <= NOISE_SHARE_MAX
