// rl_sep.hpp -- the chunk separation of the windowed ring search (rl_device.hpp: search_ring_windowed, the certificate's
// `sep[ce] > 2 d_i`), one copy for k_sweep's prologue, the table kernels and the host check (tests/sep_check.cpp).
// Part of rl_device.hpp; plain IEEE double arithmetic, so that a host compiler can include this file on its own.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RL_SEP_FN __host__ __device__ __forceinline__
#else
#define RL_SEP_FN inline
#endif
// a wave whose lanes all skip a pair executes no square root; the host has one "lane"
#if defined(__HIP_DEVICE_COMPILE__)
#define RL_SEP_ANY(p) __any(p)
#else
#define RL_SEP_ANY(p) (p)
#endif

namespace rl {

// sep[c] of a ring of nc chunk circles circ[3q .. 3q+2] = (centre x, centre y, radius): the smallest gap
//   sqrt(|m_q - m_c|^2) - r_c - r_q
// to a chunk q further than `near` chunks from c in ring order, times (1 - 1e-9), minus 1e-9 -- the value of the plain loop
// over every q, bit for bit.  fmin over a set of values does not depend on the order (no value is -0: the root of a sum of
// squares is +0 or more, and x - x is +0; a NaN never replaces a number), so the chunks are walked by ring offset -- all
// lanes of a wave look at the same relative neighbour -- and a pair that cannot lower the gap is dropped on its squared
// distance alone:
//   rmax >= every radius of the ring.  With T = fl(fl(gap + r_c) + rmax) and d2 > T^2 (1 + 1e-12): s = fl(sqrt(d2)) exceeds
//   T by 5e-13 T, while everything rounding does to T and to fl(fl(s - r_c) - r_q) stays below 6 u (T + r_c + rmax),
//   u = 2^-53; for T >= (r_c + rmax) / 512 that is less than the margin, and the pair's value is >= gap.
// Whatever is outside that proof -- no gap yet, T small against the radii or not positive, a NaN or an infinity anywhere
// (every comparison below is false for a NaN) -- takes the exact path, today's expression unchanged.
template <typename CircPtr>
RL_SEP_FN double chunk_separation(CircPtr circ, int nc, int c, int near, double rmax) {
  const double mx = circ[3 * c], my = circ[3 * c + 1], r = circ[3 * c + 2];
  const double tmin = (r + rmax) * 0x1p-9;
  double gap = INFINITY;
  double thr = INFINITY;   // a pair with d2 > thr cannot lower the gap
  int q = c + near + 1;
  if (q >= nc) q -= nc;
  for (int off = near + 1; off < nc - near; ++off) {
    const double ex = circ[3 * q] - mx, ey = circ[3 * q + 1] - my;
    const double d2 = ex * ex + ey * ey;
    const bool exact = !(d2 > thr);
    if (RL_SEP_ANY(exact)) {
      if (exact) {
        gap = fmin(gap, sqrt(d2) - r - circ[3 * q + 2]);
        const double T = gap + r + rmax;
        thr = (T >= tmin && T > 0.0) ? T * T * (1.0 + 1e-12) : INFINITY;
      }
    }
    if (++q == nc) q = 0;
  }
  return gap * (1.0 - 1e-9) - 1e-9;
}

}  // namespace rl
