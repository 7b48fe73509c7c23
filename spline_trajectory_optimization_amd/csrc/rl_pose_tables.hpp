// rl_pose_tables.hpp -- the 19-column Trajectory table of every instance of a batch of POSES (gfx950): what the reference's
// min-time pipeline does after its solve (entrypoints/traj_opt_double_track.py:75-82) -- frenet_to_global, X / Y / YAW / SPEED
// into a copy of the input table, fill_trajectory_boundaries, fill_distance -- for B instances in one launch.
//
//   k_pose_tables   RaceTrack.frenet_to_global (or poses taken as they are) + Trajectory.fill_distance + Trajectory.fill_bounds
//
// Organised like k_tables (rl_tables.hpp), whose prologue, hint and tile epilogue it shares; the ring searches are those of
// rl_device.hpp.  One workgroup of kTablesThreads per instance:
//   prologue  the instance's rings -> LDS, or its slice of the arena where they do not fit; chunk circles, chunk separations
//             and the coordinate bound for the windowed search
//   phase 1   the pose of every node, one node per thread, into LDS.  RL_POSE_FRENET: (s, n, xi) on the centre line's periodic
//             piecewise cubics x(s), y(s) (scipy CubicSpline pieces: interval by binary search over the breakpoints, value and
//             first derivative in scipy's order of operations); RL_POSE_GLOBAL: (x, y, theta) as given
//   phase 2   chord i -> i + 1 (the last node to node 0) per thread, then ONE lane adds the chords up in index order
//   phase 3   a wave owns a contiguous range of nodes and takes it 64 at a time: both ring searches along the table's own YAW,
//             the eleven computed columns of its 64 rows into a wave-private LDS tile, then the 64 x 19 doubles of the tile to
//             global memory with consecutive lanes on consecutive addresses (the other columns come from the base table or are
//             made on the way out)
// The number of nodes N is independent of the ring sizes: the hint of the windowed search always continues the run of the
// wave's previous tile (ring_hint).
#pragma once
#include "rl_tables.hpp"

namespace rl {

constexpr int kPoseCols = 11;   // staged per row: X, Y, YAW, SPEED, DIST_BWD, DIST_FWD, LBX, LBY, RBX, RBY, TIME

struct PoseTablesArgs {
  TrackDev tr;            // widths form: the initial line and its normals; widths / points: tr.N vertices per ring
  int form;               // RL_POSE_*
  const double* X;        // [B,N,6] (s, n, xi, ., ., v) or [B,N,5] (x, y, theta, ., v)
  int B, N;
  const double* ss; const double* cxs; const double* cys; int M;   // centre line: breakpoints [M+1], coefficients [4][M]
  int bounds_form;        // RL_BOUNDS_*
  const double* in;       // widths [B,tr.N,2] or bound points [B,tr.N,4]
  const double2* ringL; const double2* ringR;   // shared rings
  int nL, nR;
  int strict_rings;       // as TablesArgs
  int search;             // RL_SEARCH_*
  double max_dist;
  const double* base; int base_per_instance;    // [N,19] / [B,N,19] or null: the columns this kernel does not compute
  const double* T;        // [B,N] or null: TIME[(i + 1) % N] = T[b,i]
  double* points;         // [B,N,19]
  double* gscratch;       // rings of the instances when they do not fit LDS
  size_t gscratch_stride; // doubles per instance
};

// LDS image of one instance, in doubles (every offset even: the rings are double2)
struct PoseLds {
  int ncL, ncR;
  size_t off_x, off_y, off_phi, off_seg, off_cL, off_cR, off_pL, off_pR, off_cmax, off_stage, off_rL, off_rR, total;
};
__host__ __device__ inline PoseLds pose_lds_layout(int N, int nL, int nR, bool rings_lds) {
  PoseLds L;
  auto even = [](size_t v) { return (v + 1) & ~(size_t)1; };
  L.ncL = (nL + kChunk - 1) / kChunk;
  L.ncR = (nR + kChunk - 1) / kChunk;
  size_t o = 0;
  L.off_x = o; o += even(N);
  L.off_y = o; o += even(N);
  L.off_phi = o; o += even(N);
  L.off_seg = o; o += even(N);
  L.off_cL = o; o += even((size_t)3 * L.ncL);
  L.off_cR = o; o += even((size_t)3 * L.ncR);
  L.off_pL = o; o += even(L.ncL);
  L.off_pR = o; o += even(L.ncR);
  L.off_cmax = o; o += 2;   // [0] the coordinate bound of the window scan, [1] the sum of all chords
  L.off_stage = o; o += (size_t)kTablesWaves * kWave * kPoseCols;
  L.off_rL = o; if (rings_lds) o += (size_t)2 * (nL + kRingPad);
  L.off_rR = o; if (rings_lds) o += (size_t)2 * (nR + kRingPad);
  L.total = o;
  return L;
}

// staged column of table column c, -1: from the base table, or a constant column (IDX = i, ITERATION_FLAG = -1, the others 0)
__constant__ signed char c_pose_src[19] = {0, 1, -1, 2, 3, -1, 4, 5, -1, 6, 7, 8, 9, -1, -1, -1, 10, -1, -1};

// value (der = 0) and first derivative (der = 1) of the scipy PPoly piece c[.][j] at offset d from its breakpoint:
// scipy's evaluate_poly1 -- the terms from the constant one upwards, the power of d built up by multiplication
__device__ __forceinline__ void ppoly_cubic(const double* __restrict__ c, int M, int j, double d, double& v, double& dv) {
#pragma clang fp contract(off)
  const double c0 = c[j], c1 = c[(size_t)M + j], c2 = c[(size_t)2 * M + j], c3 = c[(size_t)3 * M + j];
  double z = d;
  v = c3 + c2 * z;
  dv = c2 + c1 * z * 2.0;
  z *= d;
  v += c1 * z;
  dv += c0 * z * 3.0;
  z *= d;
  v += c0 * z;
}
// RaceTrack.frenet_to_global at one node: centre-line point (x0, y0) with tangent (dx, dy), lateral offset nn, relative heading xi
__device__ __forceinline__ void frenet_pose(double x0, double y0, double dx, double dy, double nn, double xi, double& x,
                                            double& y, double& phi) {
#pragma clang fp contract(off)
  const double yaw0 = atan2(dy, dx);
  const double ph = yaw0 + xi;
  x = x0 - sin(yaw0) * nn;
  y = y0 + cos(yaw0) * nn;
  phi = atan2(sin(ph), cos(ph));   // align_yaw(., 0)
}
__device__ __forceinline__ double chord_length(double ex, double ey) {
#pragma clang fp contract(off)
  return sqrt(ex * ex + ey * ey);
}

template <bool RINGS_LDS>
__global__ __launch_bounds__(kTablesThreads) void k_pose_tables(PoseTablesArgs a) {
  extern __shared__ double pose_lds[];
  constexpr int BLOCK = kTablesThreads;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int N = a.N, nL = a.nL, nR = a.nR;
  const PoseLds L = pose_lds_layout(N, nL, nR, RINGS_LDS);
  double* xs = pose_lds + L.off_x;
  double* ys = pose_lds + L.off_y;
  double* phis = pose_lds + L.off_phi;
  double* seg = pose_lds + L.off_seg;
  double* circL = pose_lds + L.off_cL;
  double* circR = pose_lds + L.off_cR;
  double* sepL = pose_lds + L.off_pL;
  double* sepR = pose_lds + L.off_pR;
  double* cmax = pose_lds + L.off_cmax;
  double* stg = pose_lds + L.off_stage + (size_t)wave * kWave * kPoseCols;
  double2* rL; double2* rR;
  if constexpr (RINGS_LDS) {
    rL = reinterpret_cast<double2*>(pose_lds + L.off_rL);
    rR = reinterpret_cast<double2*>(pose_lds + L.off_rR);
  } else {
    rL = reinterpret_cast<double2*>(a.gscratch + (size_t)b * a.gscratch_stride);
    rR = rL + nL + kRingPad;
  }

  // ---- prologue: ring vertices, chunk tables
  tables_build_rings<BLOCK>(a.tr, a.bounds_form, a.strict_rings, a.in, b, a.ringL, a.ringR, nL, nR, rL, rR, tid);
  const int mode = tables_chunk_tables<BLOCK>(a.search, rL, rR, nL, nR, L.ncL, L.ncR, circL, circR, sepL, sepR, cmax, tid);

  // ---- phase 1: poses
  const int stride = a.form == 0 ? 6 : 5;
  const double* Xb = a.X + (size_t)b * N * stride;
  if (a.form == 0) {   // race_track.py: frenet_to_global
    const int M = a.M;
    const double len = a.ss[M];
    for (int i = tid; i < N; i += BLOCK) {
      const double s = Xb[(size_t)i * 6], nn = Xb[(size_t)i * 6 + 1], xi = Xb[(size_t)i * 6 + 2];
      double q = fmod(s, len);             // numpy's mod: the sign of the divisor
      if (q != 0.0 && q < 0.0) q += len;
      int lo = 0, hi = M;                  // the interval ss[lo] <= q < ss[lo + 1]; q = ss[M] belongs to the last one
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.ss[mid] <= q) lo = mid; else hi = mid;
      }
      const double d = q - a.ss[lo];
      double x0, dx, y0, dy;
      ppoly_cubic(a.cxs, M, lo, d, x0, dx);
      ppoly_cubic(a.cys, M, lo, d, y0, dy);
      frenet_pose(x0, y0, dx, dy, nn, xi, xs[i], ys[i], phis[i]);
    }
  } else {
    for (int i = tid; i < N; i += BLOCK) {
      xs[i] = Xb[(size_t)i * 5]; ys[i] = Xb[(size_t)i * 5 + 1]; phis[i] = Xb[(size_t)i * 5 + 2];
    }
  }
  __syncthreads();
  // ---- phase 2: Trajectory.fill_distance -- the chord from node i to its successor, then the running sum in index order
  for (int i = tid; i < N; i += BLOCK) {
    const int j = i + 1 < N ? i + 1 : 0;
    seg[i] = chord_length(xs[j] - xs[i], ys[j] - ys[i]);
  }
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int i0 = 0; i0 < N; i0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = i0 + u < N ? seg[i0 + u] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (i0 + u < N) seg[i0 + u] = acc;   // DIST_TO_SF_BWD of node i: the chords before it
        acc = acc + v[u];
      }
    }
    cmax[1] = acc;
  }
  __syncthreads();

  // ---- phase 3: bounds, rows
  const int ntiles = (N + kWave - 1) / kWave, per_wave = (ntiles + kTablesWaves - 1) / kTablesWaves;
  const int tile0 = wave * per_wave, tile1 = min(ntiles, tile0 + per_wave);
  const double total = cmax[1];
  double* out = a.points + (size_t)b * N * 19;
  const double* base = a.base ? a.base + (a.base_per_instance ? (size_t)b * N * 19 : 0) : nullptr;
  const double* Tb = a.T ? a.T + (size_t)b * N : nullptr;
  const int vcol = a.form == 0 ? 5 : 4;
  int pL0 = -1, pL1 = -1, pR0 = -1, pR1 = -1;   // edges found by the first and the last lane of the wave's previous tile
  for (int tl = tile0; tl < tile1; ++tl) {
    const int i_raw = tl * kWave + lane;
    const bool active = i_raw < N;
    const int i = active ? i_raw : N - 1;
    const double px = xs[i], py = ys[i], yaw = phis[i];
    // the two normal segments of fill_bounds (trajectory.py:87-92), as k_fill_bounds forms them
    const double yl = yaw + M_PI / 2.0, yr = yaw - M_PI / 2.0;
    const double dLx = a.max_dist * cos(yl), dLy = a.max_dist * sin(yl);
    const double dRx = a.max_dist * cos(yr), dRy = a.max_dist * sin(yr);
    Hit hl{INFINITY, 0.0, kNoEdge}, hr{INFINITY, 0.0, kNoEdge};
    if (mode == 2) {
      const int hintL = ring_hint(pL0, pL1, nL, i, N, lane), hintR = ring_hint(pR0, pR1, nR, i, N, lane);
      hl = search_ring_windowed<false, false>(const_cast<const double2*>(rL), nL, const_cast<const double*>(circL),
                                              const_cast<const double*>(sepL), L.ncL, active, hintL, px, py, dLx, dLy,
                                              a.max_dist, cmax);
      hr = search_ring_windowed<false, false>(const_cast<const double2*>(rR), nR, const_cast<const double*>(circR),
                                              const_cast<const double*>(sepR), L.ncR, active, hintR, px, py, dRx, dRy,
                                              a.max_dist, cmax);
      const int eL = hl.edge == kNoEdge ? -1 : hl.edge, eR = hr.edge == kNoEdge ? -1 : hr.edge;
      pL0 = __builtin_amdgcn_readlane(eL, 0); pL1 = __builtin_amdgcn_readlane(eL, kWave - 1);
      pR0 = __builtin_amdgcn_readlane(eR, 0); pR1 = __builtin_amdgcn_readlane(eR, kWave - 1);
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
      double* s = stg + lane * kPoseCols;
      const double acc = seg[i];
      s[0] = px; s[1] = py; s[2] = yaw; s[3] = Xb[(size_t)i * stride + vcol];
      s[4] = acc; s[5] = total - acc;
      // best_s is 0 when there is no crossing: the waypoint itself (trajectory.py:127)
      s[6] = px + hl.best_s * dLx; s[7] = py + hl.best_s * dLy;
      s[8] = px + hr.best_s * dRx; s[9] = py + hr.best_s * dRy;
      // T[i] is the duration of the step that starts at node i; TIME sits on the step's END point (Trajectory.fill_time)
      s[10] = Tb ? Tb[i > 0 ? i - 1 : N - 1] : (base ? base[(size_t)i * 19 + 16] : 0.0);
    }
    wave_lds_sync();
    // the tile's rows, consecutive lanes on consecutive addresses
    const int row0 = tl * kWave, rows = min(kWave, N - row0);
    double* o = out + (size_t)row0 * 19;
    const double* bo = base ? base + (size_t)row0 * 19 : nullptr;
    tile_rows_out<kPoseCols>(o, stg, c_pose_src, rows, lane, [&](int r, int c) {
      return bo ? bo[r * 19 + c] : (c == 17 ? (double)(row0 + r) : (c == 18 ? -1.0 : 0.0));
    });
    wave_lds_sync();   // the tile is free again
  }
}

}  // namespace rl
