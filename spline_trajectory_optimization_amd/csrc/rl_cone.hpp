// rl_cone.hpp -- the direction cone of a search window (rl_device.hpp: scan_window's bracket path), one copy for k_sweep's
// prologue and the host check (tests/cone_check.cpp).  Part of rl_device.hpp; plain IEEE arithmetic, so that a host compiler
// can include this file on its own.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RL_CONE_FN __host__ __device__ __forceinline__
#else
#define RL_CONE_FN inline
#endif

namespace rl {

constexpr int kConeChunk = 8;    // == kChunk
constexpr int kConeEdges = 24;   // == kWinEdges: the edges of the three chunks of a window

// Two directions A, B (about unit length, rounded to float), or all zero: "invalid".  A VALID record of the window that starts
// at chunk cs of a ring -- the kConeEdges edges (8 cs + k) mod nr -> (8 cs + k + 1) mod nr, as window_start and scan_window
// address them -- guarantees: every edge vector w of the window is non-zero and finite, cross(A, B) > 0 (the cone from A
// counter-clockwise to B spans less than pi), and cross(A, w) > 0, cross(w, B) > 0: w lies strictly inside the open cone.
struct ConeRec { float ax, ay, bx, by; };

// How the guarantee is reached: it is CHECKED, not derived.  The extreme edge directions are found by cross products about
// the window's chord (every edge must point into the chord's open half plane, which makes "clockwise of" an order), turned
// outwards by 2^-18 rad and rounded to float (that moves a unit vector by less than 2^-23); then every edge is tested against
// the ROUNDED pair, in double:  cross(A, w) > 2^-30 |w|_1.  The float components are exact doubles, |A|_inf <= 1 + 2^-17, the
// edge vector is a rounded difference (relative error u = 2^-53 per component) and the cross product rounds three times: the
// computed value differs from the real one by less than 4 u |w|_1 -- 2^-30 |w|_1 away from zero, the real sign is the
// computed one.  1-norms of the edges outside [2^-500, 2^500] (a zero edge, an infinite or NaN vertex: every comparison is
// false for a NaN), an edge not in the chord's half plane (a window that turns by more than a quarter turn either way), a
// ring no longer than two windows (the windowed search does not take it): invalid.
template <typename RingPtr>
RL_CONE_FN ConeRec cone_record(RingPtr ring, int nr, int cs) {
  const ConeRec invalid{0.0f, 0.0f, 0.0f, 0.0f};
  const int j0 = cs * kConeChunk;
  if (nr <= 2 * kConeEdges || j0 < 0 || j0 >= nr) return invalid;
  auto vx = [&](int k) { const int t = j0 + k; return ring[t >= nr ? t - nr : t].x; };
  auto vy = [&](int k) { const int t = j0 + k; return ring[t >= nr ? t - nr : t].y; };
  const double rx = vx(kConeEdges) - vx(0), ry = vy(kConeEdges) - vy(0);
  double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
  bool ok = true;
  for (int k = 0; k < kConeEdges; ++k) {
    const double wx = vx(k + 1) - vx(k), wy = vy(k + 1) - vy(k);
    const double wl = fabs(wx) + fabs(wy);
    ok = ok && wl > 0x1p-500 && wl < 0x1p+500 && rx * wx + ry * wy > 0.0;
    if (k == 0) { ax = bx = wx; ay = by = wy; }
    if (ax * wy - ay * wx < 0.0) { ax = wx; ay = wy; }   // w clockwise of A
    if (bx * wy - by * wx > 0.0) { bx = wx; by = wy; }   // w counter-clockwise of B
  }
  if (!ok) return invalid;
  const double la = sqrt(ax * ax + ay * ay), lb = sqrt(bx * bx + by * by);
  ax /= la; ay /= la; bx /= lb; by /= lb;
  const double turn = 0x1p-18;
  const ConeRec r{(float)(ax + turn * ay), (float)(ay - turn * ax), (float)(bx - turn * by), (float)(by + turn * bx)};
  const double Ax = r.ax, Ay = r.ay, Bx = r.bx, By = r.by;
  ok = Ax * By - Ay * Bx > 0x1p-40;
  for (int k = 0; k < kConeEdges; ++k) {
    const double wx = vx(k + 1) - vx(k), wy = vy(k + 1) - vy(k);
    const double lim = 0x1p-30 * (fabs(wx) + fabs(wy));
    ok = ok && Ax * wy - Ay * wx > lim && wx * By - wy * Bx > lim;
  }
  return ok ? r : invalid;
}

// True only if cross(w, d) has ONE sign, and is not zero, for every w strictly inside the record's cone -- the side values
// e_k = cross(v_k - p, d) of the window's vertices are then strictly monotone, e_{k+1} - e_k = cross(v_{k+1} - v_k, d).
// With w = alpha A + beta B, alpha, beta > 0, it is enough that cross(A, d) and cross(B, d) have one sign.  Evaluated in
// float: d is rounded (relative 2^-24 per component), one product and the fma round (2^-24 each), |A|_inf, |B|_inf <= 1 +
// 2^-17 -- the computed value is within 2^-21 (|d_x| + |d_y|) of the real one, and the rounded 1-norm within 2^-22 of it; the
// margin 2^-12 (|d_x| + |d_y|) is 500 times that.  Its floor 2^-80 keeps a direction out whose components leave the normal
// range of float (there the relative bounds fail; absolute errors are below 2^-126); an overflowed or NaN direction
// fails every comparison, and so does the all-zero (invalid) record.  Only ever sufficient: false costs time, never a bit.
RL_CONE_FN bool cone_monotone(const ConeRec& r, double dx, double dy) {
  const float fx = (float)dx, fy = (float)dy;
  const float mg = fmaxf(0x1p-12f * (fabsf(fx) + fabsf(fy)), 0x1p-80f);
  const float ca = fmaf(r.ax, fy, -(r.ay * fx)), cb = fmaf(r.bx, fy, -(r.by * fx));
  return ((ca > mg) & (cb > mg)) | ((ca < -mg) & (cb < -mg));
}

}  // namespace rl
