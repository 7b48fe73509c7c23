// rl_tables.hpp -- the 19-column Trajectory table of every instance of a solved batch, and its per-instance summary (gfx950).
//
//   k_tables         BSplineTrajectory.sample_along(ts = i/N) + Trajectory.fill_bounds for B instances, one workgroup each
//   k_table_summary  lap time (ordered sum of TIME) and the reference's result scalars, one wave per instance
//
// The arithmetic is that of the single-instance kernels (rl_kernels.hpp: k_sample_geometry, k_sample_cumsum, k_fill_bounds;
// rl_device.hpp: deboor, search_ring_*): what is new is the batched organisation.
//
// k_tables, one workgroup of kTablesThreads per instance:
//   prologue  knots and the instance's control points -> LDS; the instance's rings (shared: copied; widths / points: built as
//             the sweep builds them) -> LDS, or the instance's slice of the arena where they do not fit; chunk circles,
//             chunk separations and the coordinate bound for the windowed search
//   phase 1   the GK21 arc length of segment [u_{i-1}, u_i], one sample per thread (21 spline evaluations: the FP64 bulk)
//   phase 2   ONE lane of the instance adds the segments up in index order (the bits of the sequential sum); instances are the
//             parallel axis
//   phase 3   a wave owns a contiguous range of samples and takes it 64 at a time: geometry, both ring searches, the eleven
//             computed columns of its 64 rows into a wave-private LDS tile, then the 64 x 19 doubles of the tile to global
//             memory with consecutive lanes on consecutive addresses (the constant columns are made on the way out)
#pragma once
#include "rl_kernels.hpp"

namespace rl {

constexpr int kTablesThreads = 512;
constexpr int kTablesWaves = kTablesThreads / kWave;
constexpr int kTabCols = 11;   // staged per row: X, Y, YAW, CURVATURE, DIST_BWD, DIST_FWD, LBX, LBY, RBX, RBY, BANK

struct TablesArgs {
  TrackDev tr;
  const double* ctrl;     // [B,n,2]
  int B, form;            // RL_BOUNDS_*
  const double* in;       // widths [B,N,2] or bound points [B,N,4]
  const double2* ringL; const double2* ringR;   // shared rings
  int nL, nR;
  int strict_rings;       // widths: p0 + w (cos, sin)(yaw0 +- pi/2) from the reference-order tables (the sweep's default for k = 5)
  int search;             // RL_SEARCH_*
  double max_dist, length;
  const double* bank; int bank_per_instance;
  double* points;         // [B,N,19]
  double* gscratch;       // rings of the instances when they do not fit LDS
  size_t gscratch_stride; // doubles per instance
};

// LDS image of one instance, in doubles (every offset even: the rings are double2)
struct TablesLds {
  int ncL, ncR;
  size_t off_t, off_cx, off_cy, off_seg, off_cL, off_cR, off_pL, off_pR, off_cmax, off_stage, off_rL, off_rR, total;
};
__host__ __device__ inline TablesLds tables_lds_layout(int nt, int n, int N, int nL, int nR, bool rings_lds) {
  TablesLds L;
  auto even = [](size_t v) { return (v + 1) & ~(size_t)1; };
  L.ncL = (nL + kChunk - 1) / kChunk;
  L.ncR = (nR + kChunk - 1) / kChunk;
  size_t o = 0;
  L.off_t = o; o += even(nt);
  L.off_cx = o; o += even(n);
  L.off_cy = o; o += even(n);
  L.off_seg = o; o += even(N);
  L.off_cL = o; o += even((size_t)3 * L.ncL);
  L.off_cR = o; o += even((size_t)3 * L.ncR);
  L.off_pL = o; o += even(L.ncL);
  L.off_pR = o; o += even(L.ncR);
  L.off_cmax = o; o += 2;
  L.off_stage = o; o += (size_t)kTablesWaves * kWave * kTabCols;
  L.off_rL = o; if (rings_lds) o += (size_t)2 * (nL + kRingPad);
  L.off_rR = o; if (rings_lds) o += (size_t)2 * (nR + kRingPad);
  L.total = o;
  return L;
}
inline size_t tables_ring_scratch_doubles(int nL, int nR) { return (size_t)2 * (nL + kRingPad) + (size_t)2 * (nR + kRingPad); }

// GK21 length of the curve between parameters a and b: the panel of k_sample_geometry
template <int K>
__device__ __forceinline__ double gk21_segment(const double* __restrict__ t, int n, const double* __restrict__ cx,
                                               const double* __restrict__ cy, double a, double b) {
  const double centr = 0.5 * (a + b), hl = 0.5 * (b - a);
  double resk = c_wgk[10] * speed_at<K>(t, n, cx, cy, centr);
#pragma unroll 1
  for (int j = 0; j < 5; ++j) {
    const int jt = 2 * j + 1;
    const double ab = hl * c_xgk[jt];
    resk += c_wgk[jt] * (speed_at<K>(t, n, cx, cy, centr - ab) + speed_at<K>(t, n, cx, cy, centr + ab));
  }
#pragma unroll 1
  for (int j = 0; j < 5; ++j) {
    const int jt = 2 * j;
    const double ab = hl * c_xgk[jt];
    resk += c_wgk[jt] * (speed_at<K>(t, n, cx, cy, centr - ab) + speed_at<K>(t, n, cx, cy, centr + ab));
  }
  return resk * hl;
}

// staged column of table column c, -1: a constant column (IDX = i, ITERATION_FLAG = -1, the others 0)
__constant__ signed char c_tab_src[19] = {0, 1, -1, 2, -1, 3, 4, 5, -1, 6, 7, 8, 9, 10, -1, -1, -1, -1, -1};

__device__ __forceinline__ void wave_lds_sync() {   // the LDS writes of this wave's lanes are visible to its other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- what k_tables and k_pose_tables (rl_pose_tables.hpp) share: the prologue that makes an instance's rings searchable,
// the hint of the windowed search along a run of samples, and the way a tile of rows leaves for global memory.

// The instance's ring vertices into rL / rR (LDS or the arena), as k_sweep's prologue builds them, with the first kRingPad
// vertices repeated behind the last.  form = RL_BOUNDS_*: the widths / points forms make tr.N vertices per side from
// in[b] (strict_rings: from the reference-order tables), the shared form copies ringL / ringR.  Every thread of the
// block calls it; the rings are complete (block wide) on return.
template <int BLOCK>
__device__ __forceinline__ void tables_build_rings(const TrackDev& tr, int form, int strict_rings, const double* in, int b,
                                                   const double2* ringL, const double2* ringR, int nL, int nR, double2* rL,
                                                   double2* rR, int tid) {
  const int N = tr.N;
  if (form == 1) {   // widths: vertex i = p0_i + w_l n0_i  /  p0_i - w_r n0_i
    const double2* w = reinterpret_cast<const double2*>(in) + (size_t)b * N;
    for (int i = tid; i < N; i += BLOCK) {
      const double2 wi = w[i];
      if (strict_rings) {   // oracle: orc_width_rings -- p0 + w cos / sin(yaw0 +- pi/2), each normal on its own
        const double* bs = tr.base_s;
        const double px = bs[i], py = bs[(size_t)N + i];
        rL[i] = make_double2(uf_madd(px, wi.x, bs[(size_t)2 * N + i]), uf_madd(py, wi.x, bs[(size_t)3 * N + i]));
        rR[i] = make_double2(uf_madd(px, wi.y, bs[(size_t)4 * N + i]), uf_madd(py, wi.y, bs[(size_t)5 * N + i]));
      } else {
        const double px = tr.base[i], py = tr.base[(size_t)N + i];
        const double nx = tr.base[(size_t)2 * N + i], ny = tr.base[(size_t)3 * N + i];
        rL[i] = make_double2(px + wi.x * nx, py + wi.x * ny);
        rR[i] = make_double2(px - wi.y * nx, py - wi.y * ny);
      }
    }
  } else if (form == 2) {   // bound points
    const double4* w = reinterpret_cast<const double4*>(in) + (size_t)b * N;
    for (int i = tid; i < N; i += BLOCK) {
      const double4 wi = w[i];
      rL[i] = make_double2(wi.x, wi.y);
      rR[i] = make_double2(wi.z, wi.w);
    }
  } else {
    for (int i = tid; i < nL; i += BLOCK) rL[i] = ringL[i];
    for (int i = tid; i < nR; i += BLOCK) rR[i] = ringR[i];
  }
  __syncthreads();
  for (int q = tid; q < 2 * kRingPad; q += BLOCK) {   // repeat the first vertices behind the last
    if (q < kRingPad) rL[nL + q] = rL[q % nL]; else rR[nR + q - kRingPad] = rR[(q - kRingPad) % nR];
  }
  __syncthreads();
}

// Chunk circles (culled and windowed search), chunk separations and the coordinate bound (windowed search) of the two
// rings.  Returns the search mode in effect: the windowed mode needs rings longer than its window (as k_sweep decides it).
// Every thread of the block calls it; the CALLER's next __syncthreads() completes the tables.
template <int BLOCK>
__device__ __forceinline__ int tables_chunk_tables(int search, const double2* rL, const double2* rR, int nL, int nR, int ncL,
                                                   int ncR, double* circL, double* circR, double* sepL, double* sepR,
                                                   double* cmax, int tid) {
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int mode = (search == 2 && nL > 2 * kWinEdges && nR > 2 * kWinEdges) ? 2 : (search >= 1 ? 1 : 0);
  if (mode >= 1) {
    for (int c = tid; c < ncL + ncR; c += BLOCK) {
      const bool left = c < ncL;
      const int cc = left ? c : c - ncL;
      const double2* ring = left ? rL : rR;
      const int nr = left ? nL : nR;
      const int j0 = cc * kChunk, j1 = min(j0 + kChunk, nr);
      double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
      for (int j = j0; j <= j1; ++j) {
        const double2 v = ring[j >= nr ? j - nr : j];
        xmin = fmin(xmin, v.x); xmax = fmax(xmax, v.x);
        ymin = fmin(ymin, v.y); ymax = fmax(ymax, v.y);
      }
      const double mx = 0.5 * (xmin + xmax), my = 0.5 * (ymin + ymax);
      double r2 = 0.0;
      for (int j = j0; j <= j1; ++j) {
        const double2 v = ring[j >= nr ? j - nr : j];
        const double ex = v.x - mx, ey = v.y - my;
        r2 = fmax(r2, ex * ex + ey * ey);
      }
      double* o = (left ? circL : circR) + 3 * cc;
      o[0] = mx; o[1] = my; o[2] = sqrt(r2) * (1.0 + 1e-12);
    }
    __syncthreads();
    if (mode == 2) {
      // a bound on every chunk radius for the pruned separation pass (rl_sep.hpp; a NaN radius: +inf, no pruning): every wave
      // forms it for itself, which needs neither a slot of LDS nor another barrier
      double rmax = 0.0;
      for (int c = lane; c < ncL + ncR; c += kWave) {
        const double rc = c < ncL ? circL[3 * c + 2] : circR[3 * (c - ncL) + 2];
        rmax = rc <= 0x1p+1000 ? fmax(rmax, rc) : INFINITY;
      }
      rmax = wave_max_bfly(rmax);
      for (int c = tid; c < ncL + ncR; c += BLOCK) {
        const bool left = c < ncL;
        const int cc = left ? c : c - ncL;
        (left ? sepL : sepR)[cc] = chunk_separation(left ? circL : circR, left ? ncL : ncR, cc, kNear, rmax);
      }
      if (wave == 0) {   // a bound on every ring coordinate, for the quick sign pass of the window scan (+inf: no quick pass)
        double m = 0.0;
        for (int c = lane; c < ncL + ncR; c += kWave) {
          const double* o = c < ncL ? circL + 3 * c : circR + 3 * (c - ncL);
          const double v = fmax(fabs(o[0]), fabs(o[1])) + o[2];
          m = v <= 0x1p+1000 ? fmax(m, v) : INFINITY;
        }
        m = wave_max_bfly(m);
        if (lane == 0) cmax[0] = m;
      }
    }
  }
  return mode;
}

// Hint of the windowed search for sample i of N along a ring of nr edges: continue the run of the wave's previous 64 samples
// (e0, e1: the edges its first and last lane found, < 0: none) along the ring; a wave's first tile guesses proportionally.
// A wrong hint costs the slow path of the search, never the result.
__device__ __forceinline__ int ring_hint(int e0, int e1, int nr, int i, int N, int lane) {
  if (e0 < 0 || e1 < 0) return (int)(((long long)i * nr) / N);
  int d = e1 - e0;
  if (d > nr / 2) d -= nr;
  if (d < -(nr / 2)) d += nr;
  int h = (e1 + (d * (lane + 1)) / (kWave - 1)) % nr;
  return h < 0 ? h + nr : h;
}

// A wave's tile of `rows` (<= 64) table rows to global memory, consecutive lanes on consecutive addresses: column c comes
// from the staged column src[c] (COLS staged doubles per row), or from other(row, c) where src[c] < 0.
template <int COLS, typename Other>
__device__ __forceinline__ void tile_rows_out(double* o, const double* stg, const signed char* src, int rows, int lane,
                                              Other&& other) {
  for (int e = lane; e < rows * 19; e += kWave) {
    const int r = e / 19, c = e - r * 19;
    const int s = src[c];
    o[e] = s >= 0 ? stg[r * COLS + s] : other(r, c);
  }
}

template <int K, bool RINGS_LDS>
__global__ __launch_bounds__(kTablesThreads) void k_tables(TablesArgs a) {
  extern __shared__ double tab_lds[];
  constexpr int BLOCK = kTablesThreads;
  const TrackDev& tr = a.tr;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n = tr.n, N = tr.N, nt = tr.nt, nL = a.nL, nR = a.nR;
  const TablesLds L = tables_lds_layout(nt, n, N, nL, nR, RINGS_LDS);
  double* t = tab_lds + L.off_t;
  double* cx = tab_lds + L.off_cx;
  double* cy = tab_lds + L.off_cy;
  double* seg = tab_lds + L.off_seg;
  double* circL = tab_lds + L.off_cL;
  double* circR = tab_lds + L.off_cR;
  double* sepL = tab_lds + L.off_pL;
  double* sepR = tab_lds + L.off_pR;
  double* cmax = tab_lds + L.off_cmax;
  double* stg = tab_lds + L.off_stage + (size_t)wave * kWave * kTabCols;
  double2* rL; double2* rR;
  if constexpr (RINGS_LDS) {
    rL = reinterpret_cast<double2*>(tab_lds + L.off_rL);
    rR = reinterpret_cast<double2*>(tab_lds + L.off_rR);
  } else {
    rL = reinterpret_cast<double2*>(a.gscratch + (size_t)b * a.gscratch_stride);
    rR = rL + nL + kRingPad;
  }

  // ---- prologue: knots, control points, ring vertices (as k_sweep's prologue builds them), chunk tables
  for (int j = tid; j < nt; j += BLOCK) t[j] = tr.t[j];
  {
    const double2* cb = reinterpret_cast<const double2*>(a.ctrl) + (size_t)b * n;
    for (int j = tid; j < n; j += BLOCK) { const double2 c = cb[j]; cx[j] = c.x; cy[j] = c.y; }
  }
  tables_build_rings<BLOCK>(tr, a.form, a.strict_rings, a.in, b, a.ringL, a.ringR, nL, nR, rL, rR, tid);
  const int mode = tables_chunk_tables<BLOCK>(a.search, rL, rR, nL, nR, L.ncL, L.ncR, circL, circR, sepL, sepR, cmax, tid);

  // ---- phase 1: segment lengths (trajectory.py:283-289: quad over [u_{i-1}, u_i] = one GK21 panel)
  const double step = 1.0 / (double)N;   // np.linspace(0, 1, N, endpoint=False)
  for (int i = tid; i < N; i += BLOCK)
    seg[i] = i > 0 ? gk21_segment<K>(t, n, cx, cy, (double)(i - 1) * step, (double)i * step) : 0.0;
  __syncthreads();
  // ---- phase 2: the running sum in index order, one lane for the instance (seg[0] = 0: acc starts as the reference's does)
  if (tid == 0) {
    double acc = 0.0;
    for (int i0 = 0; i0 < N; i0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = i0 + u < N ? seg[i0 + u] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc = acc + v[u];
        if (i0 + u < N) seg[i0 + u] = acc;
      }
    }
  }
  __syncthreads();

  // ---- phase 3: geometry, bounds, rows
  const int ntiles = (N + kWave - 1) / kWave, per_wave = (ntiles + kTablesWaves - 1) / kTablesWaves;
  const int tile0 = wave * per_wave, tile1 = min(ntiles, tile0 + per_wave);
  const bool dist = a.length > 0.0;
  double* out = a.points + (size_t)b * N * 19;
  const double* bank = a.bank ? a.bank + (a.bank_per_instance ? (size_t)b * N : 0) : nullptr;
  int pL0 = -1, pL1 = -1, pR0 = -1, pR1 = -1;   // shared rings: edges found by the first and the last lane of the wave's previous tile
  for (int tl = tile0; tl < tile1; ++tl) {
    const int i_raw = tl * kWave + lane;
    const bool active = i_raw < N;
    const int i = active ? i_raw : N - 1;
    const double x = (double)i * step;
    const int l = tr.ell[i];
    double v[6];
    {
      double h[K + 1];
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        deboor<K>(t, x, l, m, h);
        double sx = 0, sy = 0;
#pragma unroll
        for (int q = 0; q <= K; ++q) { sx += cx[l - K + q] * h[q]; sy += cy[l - K + q] * h[q]; }
        v[2 * m] = sx; v[2 * m + 1] = sy;
      }
    }
    const double px = v[0], py = v[1];
    const double yaw = atan2(v[3], v[2]);
    const double s2 = v[2] * v[2] + v[3] * v[3];
    const double curvature = fabs(v[2] * v[5] - v[3] * v[4]) / sqrt(s2 * s2 * s2);
    const double radius = 1.0 / fabs(curvature);
    // the two normal segments of fill_bounds (trajectory.py:87-92), as k_fill_bounds forms them
    const double yl = yaw + M_PI / 2.0, yr = yaw - M_PI / 2.0;
    const double dLx = a.max_dist * cos(yl), dLy = a.max_dist * sin(yl);
    const double dRx = a.max_dist * cos(yr), dRy = a.max_dist * sin(yr);
    Hit hl{INFINITY, 0.0, kNoEdge}, hr{INFINITY, 0.0, kNoEdge};
    if (mode == 2) {
      int hintL = i, hintR = i;   // widths / points: vertex i sits on sample i's (initial) normal
      if (a.form == 0) {
        // shared rings: continue the run of the wave's previous 64 samples along the ring; the first tile of a wave guesses
        // proportionally (a wrong hint costs the slow path of the search, never the result)
        auto guess = [&](int e0, int e1, int nr) { return ring_hint(e0, e1, nr, i, N, lane); };
        hintL = guess(pL0, pL1, nL);
        hintR = guess(pR0, pR1, nR);
      }
      hl = search_ring_windowed<false, false>(const_cast<const double2*>(rL), nL, const_cast<const double*>(circL),
                                              const_cast<const double*>(sepL), L.ncL, active, hintL, px, py, dLx, dLy,
                                              a.max_dist, cmax);
      hr = search_ring_windowed<false, false>(const_cast<const double2*>(rR), nR, const_cast<const double*>(circR),
                                              const_cast<const double*>(sepR), L.ncR, active, hintR, px, py, dRx, dRy,
                                              a.max_dist, cmax);
      if (a.form == 0) {
        const int eL = hl.edge == kNoEdge ? -1 : hl.edge, eR = hr.edge == kNoEdge ? -1 : hr.edge;
        pL0 = __builtin_amdgcn_readlane(eL, 0); pL1 = __builtin_amdgcn_readlane(eL, kWave - 1);
        pR0 = __builtin_amdgcn_readlane(eR, 0); pR1 = __builtin_amdgcn_readlane(eR, kWave - 1);
      }
    } else if (active) {
      if (mode == 1) {
        hl = search_ring_culled(const_cast<const double2*>(rL), nL, const_cast<const double*>(circL), L.ncL, px, py, dLx, dLy, a.max_dist);
        hr = search_ring_culled(const_cast<const double2*>(rR), nR, const_cast<const double*>(circR), L.ncR, px, py, dRx, dRy, a.max_dist);
      } else {
        hl = search_ring_brute(const_cast<const double2*>(rL), nL, px, py, dLx, dLy);
        hr = search_ring_brute(const_cast<const double2*>(rR), nR, px, py, dRx, dRy);
      }
    }
    if (active) {
      double* s = stg + lane * kTabCols;
      const double acc = dist ? seg[i] : 0.0;
      s[0] = px; s[1] = py; s[2] = yaw; s[3] = radius;
      s[4] = acc; s[5] = dist ? a.length - acc : 0.0;
      // best_s is 0 when there is no crossing: the waypoint itself (trajectory.py:127)
      s[6] = px + hl.best_s * dLx; s[7] = py + hl.best_s * dLy;
      s[8] = px + hr.best_s * dRx; s[9] = py + hr.best_s * dRy;
      s[10] = bank ? bank[i] : 0.0;
    }
    wave_lds_sync();
    // the tile's rows, consecutive lanes on consecutive addresses
    const int row0 = tl * kWave, rows = min(kWave, N - row0);
    double* o = out + (size_t)row0 * 19;
    tile_rows_out<kTabCols>(o, stg, c_tab_src, rows, lane,
                            [&](int r, int c) { return c == 17 ? (double)(row0 + r) : (c == 18 ? -1.0 : 0.0); });
    wave_lds_sync();   // the tile is free again
  }
}

// ------------------------------------------------------------------------------------------------
// out[b][8] = sum of TIME in index order, TIME[0], DIST_TO_SF_FWD[0] / TIME[0], max / min SPEED, max LAT_ACC, max / min LON_ACC.
// One wave per instance: the lanes stage TIME in LDS and take the extrema; lane 0 adds TIME up in index order.
__global__ __launch_bounds__(kWave) void k_table_summary(const double* __restrict__ points, int N, const int* __restrict__ iters,
                                                         double* __restrict__ out) {
  extern __shared__ double sum_lds[];   // [N] TIME
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* P = points + (size_t)b * N * 19;
  double* o = out + (size_t)b * 8;
  if (iters && iters[b] < 0) {
    if (lane < 8) o[lane] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  double vmax = -INFINITY, vmin = INFINITY, latmax = -INFINITY, lonmax = -INFINITY, lonmin = INFINITY;
  bool nan_v = false, nan_lat = false, nan_lon = false;
  for (int i = lane; i < N; i += kWave) {
    const double* p = P + (size_t)i * 19;
    const double v = p[4], lon = p[14], lat = p[15];
    sum_lds[i] = p[16];
    nan_v |= v != v; nan_lat |= lat != lat; nan_lon |= lon != lon;
    vmax = fmax(vmax, v); vmin = fmin(vmin, v);
    latmax = fmax(latmax, lat);
    lonmax = fmax(lonmax, lon); lonmin = fmin(lonmin, lon);
  }
  vmax = wave_max(vmax); vmin = wave_min(vmin); latmax = wave_max(latmax);
  lonmax = wave_max(lonmax); lonmin = wave_min(lonmin);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (__any(nan_v)) { vmax = qnan; vmin = qnan; }       // numpy's max / min return NaN when one is present
  if (__any(nan_lat)) latmax = qnan;
  if (__any(nan_lon)) { lonmax = qnan; lonmin = qnan; }
  wave_lds_sync();
  if (lane == 0) {
    double acc = 0.0;   // np.cumsum(TIME)[-1]: 0 + t_0 + t_1 + ... one addition at a time
    for (int i0 = 0; i0 < N; i0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = i0 + u < N ? sum_lds[i0 + u] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) if (i0 + u < N) acc = acc + v[u];
    }
    const double t0 = sum_lds[0];
    o[0] = acc; o[1] = t0; o[2] = P[7] / t0;
    o[3] = vmax; o[4] = vmin; o[5] = latmax; o[6] = lonmax; o[7] = lonmin;
  }
}

}  // namespace rl
