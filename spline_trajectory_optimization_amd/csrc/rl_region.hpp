// rl_region.hpp -- k_region_index: Trajectory.fill_region, the first region polygon that strictly contains each point.
//
// Semantics (models/trajectory.py: fill_region): a point is inside a polygon when it lies in its INTERIOR; a point on an edge
// or a vertex is not.  The closing edge (last vertex -> first) is implied; a repeated closing vertex only adds a zero-length
// edge, which changes nothing.  A polygon of zero area contains nothing, a point with a non-finite coordinate lies in no
// region, and so does every point for a region with a non-finite vertex (the host gives it an empty box).  Self-intersecting
// polygons are outside the contract; for them the kernel applies the even-odd rule.
//
// Method (own derivation).  Cast the ray from p = (px, py) towards +x and count the edges it crosses; p is inside when the
// count is odd.  Half-open rule on y: the edge (a, b) counts when exactly one of ay > py, by > py holds, so a ray through a
// vertex counts it once for the edge above and not for the one at or below, and horizontal edges never count.  For such an
// edge the crossing lies to the right of p exactly when p is on the left of the upward-directed edge, i.e. when the sign of
//     o(a, b, p) = (bx - ax)(py - ay) - (by - ay)(px - ax)
// is positive for an upward edge (ay <= py < by) and negative for a downward one.  p is ON the boundary exactly when some
// edge has o = 0 and p inside the edge's closed bounding box; every such case is examined before the crossing count matters.
//
// The sign of o is decided without rounding errors:
//   * filter: with t1 = fl(bx-ax) fl(py-ay), t2 = fl(by-ay) fl(px-ax) rounded and d = fl(t1 - t2), all five operations
//     correctly rounded (no contraction: `#pragma clang fp contract(off)` below), |d - o| <= (3 eps + 16 eps^2)(|t1| + |t2|)
//     with eps = 2^-53 (the standard bound for this expression, which holds as long as nothing under- or overflows).  The
//     filter accepts sign(d) when |d| exceeds that bound and |t1| + |t2| >= 2^-900 (far from the subnormal range).
//   * exact: otherwise o is expanded into the six coordinate products
//         o = ax by - ay bx + bx py - by px + px ay - py ax,
//     each split exactly by two_prod into a sum of two doubles (rl_crmath.hpp), and the twelve terms are summed into a
//     non-overlapping expansion with two_sum (each step exact).  The sign of o is that of the expansion's most significant
//     non-zero term.  Exact for every coordinate that is 0 or of magnitude in [2^-480, 2^500]: no product under- or
//     overflows (track coordinates in metres are far inside this range).
//
// Layout: one lane per point, the regions in list order.  A region whose bounding box does not hold a lane's point in its
// interior is rejected by that lane at once; when no lane of the workgroup needs the region, the workgroup skips it.
// Otherwise the region's vertices pass through LDS in tiles of kRegionTile + 1 (the first vertex of the next tile, or the
// polygon's first vertex, closes the tile's last edge), so every lane reads the same vertex at the same time (a broadcast)
// and any vertex count fits.  The workgroup stops as soon as every one of its points has found its region.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#include "rl_crmath.hpp"

namespace rl {

constexpr int kRegionBlock = 256;   // lanes (points) per workgroup
constexpr int kRegionTile = 512;    // edges per LDS tile: (512 + 1) x 16 B = 8.2 KB

struct RegionArgs {
  const double* xy;       // point i at xy[i * stride], xy[i * stride + 1]
  long long stride;       // doubles between consecutive points
  long long n;            // number of points (B * N)
  const double2* verts;   // [V]: the vertices of all regions, region after region
  const int* offsets;     // [R + 1]: region r owns verts[offsets[r] .. offsets[r+1])
  const double4* box;     // [R]: (min x, min y, max x, max y) of each region
  int R;
  int* out;               // [n] index of the first containing region or -1 (may be null)
  const int* codes;       // [R] (used with tag)
  double* tag;            // tag[i * tag_stride] = codes[index] where a region contains point i (may be null)
  long long tag_stride;
};

// sign of (bx - ax)(py - ay) - (by - ay)(px - ax): +1, -1 or 0, exactly
__device__ __forceinline__ int region_orient(double ax, double ay, double bx, double by, double px, double py) {
  RL_CR_STRICT
  const double t1 = (bx - ax) * (py - ay);
  const double t2 = (by - ay) * (px - ax);
  const double d = t1 - t2;
  const double mag = fabs(t1) + fabs(t2);
  const double eps = 0x1p-53;
  const double bound = (3.0 * eps + 16.0 * eps * eps) * mag;
  if (fabs(d) > bound && mag >= 0x1p-900) return d > 0.0 ? 1 : -1;
  // exact: twelve terms, summed into a non-overlapping expansion e[0..11] (increasing magnitude, zeros allowed)
  const cr::dd p[6] = {cr::two_prod(ax, by), cr::two_prod(-ay, bx), cr::two_prod(bx, py),
                       cr::two_prod(-by, px), cr::two_prod(px, ay), cr::two_prod(-py, ax)};
  double e[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {   // grow the expansion e[0..k) by one term: e[0..k] is again exact and non-overlapping
    double q = (k & 1) ? p[k >> 1].hi : p[k >> 1].lo;
#pragma unroll
    for (int j = 0; j < k; ++j) {
      const cr::dd s = cr::two_sum(q, e[j]);
      e[j] = s.lo;
      q = s.hi;
    }
    e[k] = q;
  }
  int sgn = 0;
#pragma unroll
  for (int j = 0; j < 12; ++j)
    if (e[j] != 0.0) sgn = e[j] > 0.0 ? 1 : -1;
  return sgn;
}

__global__ void __launch_bounds__(kRegionBlock) k_region_index(RegionArgs a) {
  __shared__ double2 tile[kRegionTile + 1];
  const long long i = (long long)blockIdx.x * kRegionBlock + threadIdx.x;
  const bool live = i < a.n;
  double px = 0.0, py = 0.0;
  if (live) { px = a.xy[i * a.stride]; py = a.xy[i * a.stride + 1]; }
  // a point with a non-finite coordinate is in no region: it never asks for one
  bool done = !live || !(isfinite(px) && isfinite(py));
  int found = -1;
  for (int r = 0; r < a.R; ++r) {
    if (!__syncthreads_or(!done)) break;
    const double4 bb = a.box[r];
    // interior points of the polygon lie in the OPEN box (this also rejects zero-width boxes and empty ones)
    const bool want = !done && bb.x < px && px < bb.z && bb.y < py && py < bb.w;
    if (!__syncthreads_or(want)) continue;
    const int v0 = a.offsets[r], nv = a.offsets[r + 1] - v0;
    bool odd = false, on_edge = false;
    for (int base = 0; base < nv; base += kRegionTile) {
      const int m = min(kRegionTile, nv - base);   // edges of this tile: vertex base+j -> base+j+1 (cyclic)
      for (int j = threadIdx.x; j <= m; j += kRegionBlock) {
        const int v = base + j;
        tile[j] = a.verts[v0 + (v < nv ? v : 0)];
      }
      __syncthreads();
      if (want && !on_edge) {
        for (int j = 0; j < m; ++j) {
          const double2 va = tile[j], vb = tile[j + 1];
          const bool up_a = va.y > py, up_b = vb.y > py;
          const double xlo = fmin(va.x, vb.x), xhi = fmax(va.x, vb.x);
          if (up_a != up_b) {
            if (px < xlo) {
              odd = !odd;                                  // the whole edge lies right of p
            } else if (px <= xhi) {
              const int s = region_orient(va.x, va.y, vb.x, vb.y, px, py);
              if (s == 0) { on_edge = true; break; }
              if ((s > 0) == up_b) odd = !odd;             // upward edge: p on its left; downward: on its right
            }
          } else if (fmin(va.y, vb.y) <= py && py <= fmax(va.y, vb.y) && xlo <= px && px <= xhi) {
            // no crossing, but p lies in the edge's closed box (py at the edge's upper end, or a horizontal edge at py)
            if (region_orient(va.x, va.y, vb.x, vb.y, px, py) == 0) { on_edge = true; break; }
          }
        }
      }
      __syncthreads();   // the tile is overwritten next
    }
    if (want && odd && !on_edge) { found = r; done = true; }
  }
  if (!live) return;
  if (a.out) a.out[i] = found;
  if (a.tag && found >= 0) a.tag[i * a.tag_stride] = (double)a.codes[found];
}

}  // namespace rl
