// rl_global.hpp -- a15: the GLOBAL min-curvature QP (BASELINE.json north_star:
// "QP with the lateral offset from the centre line bounded by the left/right track widths, banded
// KKT structure from the spline basis factorised in LDS, one track instance per workgroup").
//
// The reference has no working global solver (its Julia notebook prototype does not converge,
// SURVEY.md App. A.6), so the formulation is this build's own; its CPU twin is
// oracle/mincurv_oracle.c: orc_global_mincurv, and the comment block there states the maths.
//
//   unknowns   a_j (j < np = n - k): periodic control point j slides along the fixed unit normal
//              nu_j of the centre line at its Greville site
//   rows       lo_i <= A_i . a <= hi_i, one per sample; row i touches the k+1 control points of its
//              knot span, so A'DA is cyclic-banded with half-bandwidth k
//   cost       Gauss-Newton on sum kappa_i^2, re-linearised n_outer times
//   QP         Mehrotra predictor-corrector interior point, common primal/dual step
//
// Mapping to the machine
//   * one workgroup = one instance; thread = one CHUNK of <= kGRows consecutive samples of ONE knot
//     span.  The interior-point state of those rows (slacks, duals, primal residuals) never leaves
//     the thread's registers, and because a chunk has a single span its k+1 unknowns are read from
//     LDS once per phase.
//   * A'DA, A'w and G'G are sums over rows of one span: every thread reduces its chunk in
//     registers, the chunk partials of a span are added in chunk order through a small LDS
//     staging area (fixed order -> run-to-run reproducible), and span sums are gathered into the
//     cyclic band.
//   * the np x np normal matrix is stored as a band (rows < np-k) plus k dense border rows (the
//     periodic wrap) in LDS and factorised L D L' by wave 0, one lane per entry of the trailing
//     update; the triangular solves keep the vector in registers and broadcast the pivot with
//     v_readlane, so only L is read from LDS.
//   * the constraint rows A (instance independent) are a track-level table that stays in L2.
#pragma once
#include "rl_device.hpp"
#include "rl_kernels.hpp"   // kWeightMin, kWeightMax

namespace rl {

// (the interior-point exit rule of all global-QP kernels: rl_device.hpp, ipm_done)

constexpr int kGRows = 8;     // samples per chunk == per thread
constexpr int kGRound = 11;   // span outputs staged per flush round
constexpr int kGMaxNp = 192;  // 3 rows per lane in the triangular solves

struct GlobalArgs {
  TrackDev trk;
  const double* A;       // [N][k+1] constraint rows: D0[a][i] * (n0_i . nu_j)
  const double* nu;      // [np][2]
  const int* chunk;      // [nc][2]: (first row | count << 24, span)
  const int* span_ch0;   // [np+1] first chunk of every span (chunks of a span are consecutive)
  int nc, np;
  const double* widths;  // [B][N][2] (w_left, w_right)
  double margin;
  int n_outer, max_ipm;
  int last_as_mid;       // test hook "global_last_as_mid": the last linearisation leaves at the intermediate tolerance
  double* out_ctrl;      // [B][n][2]
  double* out_xy;        // [B][N][2] or null
  double* out_a;         // [B][np] or null
  double* out_stats;     // [B][8]: ipm iterations, sum kappa^2 first / last, bound violation, last step
};

struct GlobalLayout {  // offsets in doubles
  int xs, dxs, avs, qv, rdP, rd, rhs, dinv, cxs, cys, nus, Pc, Lb, W, Ssum, Spart, red, sch, total;
};

__host__ __device__ inline GlobalLayout global_layout(int k, int n, int np, int block) {
  const int K1 = k + 1, NO = K1 * (K1 + 1) / 2 + 2 * K1;
  GlobalLayout L;
  int o = 0;
  auto take = [&](int c) { const int r = o; o += c; return r; };
  L.xs = take(np); L.dxs = take(np); L.avs = take(np); L.qv = take(np); L.rdP = take(np);
  L.rd = take(np); L.rhs = take(np); L.dinv = take(np);
  L.cxs = take(n); L.cys = take(n); L.nus = take(2 * np);
  L.Pc = take(np * K1); L.Lb = take(np * K1); L.W = take(k * np);
  L.Ssum = take(np * NO); L.Spart = take(block * kGRound);
  L.red = take(3 * 16);
  L.sch = take((np + 2) / 2 + 1);  // np+1 ints
  L.total = o;
  return L;
}

// ------------------------------------------------------------------------------------------------
// track-level tables
template <int K>
__global__ void k_global_normals(TrackDev tr, int np, double* __restrict__ nu) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= np) return;
  double g = 0.0;
  for (int q = 1; q <= K; ++q) g += tr.t[j + q];
  g /= (double)K;
  g -= floor(g);
  const int l = find_interval(tr.t, K, tr.n, g);
  double h[K + 1];
  deboor<K>(tr.t, g, l, 1, h);
  double dx = 0, dy = 0;
#pragma unroll
  for (int a = 0; a <= K; ++a) { dx += tr.c0[l - K + a] * h[a]; dy += tr.c0[tr.n + l - K + a] * h[a]; }
  const double s = sqrt(dx * dx + dy * dy);
  nu[2 * j] = -dy / s;
  nu[2 * j + 1] = dx / s;
}

template <int K>
__global__ void k_global_rows(TrackDev tr, int np, const double* __restrict__ nu, double* __restrict__ A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = tr.N;
  if (i >= N) return;
  const int s = tr.ell[i] - K;
  const double n0x = tr.base[(size_t)2 * N + i], n0y = tr.base[(size_t)3 * N + i];
#pragma unroll
  for (int a = 0; a <= K; ++a) {
    int j = s + a;
    if (j >= np) j -= np;
    A[(size_t)i * (K + 1) + a] = tr.D[(size_t)a * N + i] * (n0x * nu[2 * j] + n0y * nu[2 * j + 1]);
  }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lane_bcast(double v, int l) {  // l wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// In-place L D L' of the bordered band: rows r < m = np-K hold K[r][r-d] at Lb[r*(K+1)+d], the K
// border rows hold K[m+q][c] at W[q*np+c].  Afterwards the strictly lower entries are L, the
// diagonal slots still hold D and dinv[c] = 1/D_c.  ONE wave; lane = one entry (t1,t2) of the
// trailing update of the current column, whose at most 2K rows are the band rows below the pivot
// and the border rows.
template <int K>
__device__ __forceinline__ void band_factor(double* Lb, double* W, double* dinv, int np, int lane) {
  constexpr int K1 = K + 1;
  const int m = np - K;
  int t1 = 0;
  while ((t1 + 1) * (t1 + 2) / 2 <= lane) ++t1;
  const int t2 = lane - t1 * (t1 + 1) / 2;
  auto E = [&](int r, int q) -> double* { return r < m ? Lb + r * K1 + (r - q) : W + (r - m) * np + q; };
  for (int c = 0; c < np; ++c) {
    const int nb = c < m ? min(K, m - 1 - c) : 0;
    const int bs = max(m, c + 1);
    const int T = nb + np - bs;
    const bool pv = t1 < T;
    const int r1 = t1 < nb ? c + 1 + t1 : bs + (t1 - nb);
    const int r2 = t2 < nb ? c + 1 + t2 : bs + (t2 - nb);
    const double inv = 1.0 / *E(c, c);
    double u1 = 0.0, u2 = 0.0, own = 0.0;
    if (pv) { u1 = *E(r1, c); u2 = *E(r2, c); own = *E(r1, r2); }
    wave_lds_fence();
    if (pv) {
      *E(r1, r2) = fma(-u1, u2 * inv, own);
      if (t1 == t2) *E(r1, c) = u1 * inv;
    }
    if (lane == 0) dinv[c] = inv;
    wave_lds_fence();
  }
}

// Solves (L D L') x = rhs with the factor above; ONE wave, x in registers (row = lane + 64 q).
template <int K>
__device__ __forceinline__ void band_solve(const double* Lb, const double* W, const double* dinv, int np,
                                           int lane, const double* rhs, double* out) {
  constexpr int K1 = K + 1;
  constexpr int RLM = kGMaxNp / kWave;
  const int m = np - K;
  double y[RLM];
#pragma unroll
  for (int q = 0; q < RLM; ++q) { const int r = lane + kWave * q; y[q] = r < np ? rhs[r] : 0.0; }
  auto pivot = [&](int c) {
    const int seg = c >> 6;
    const double v = seg == 0 ? y[0] : (seg == 1 ? y[1] : y[2]);
    return lane_bcast(v, c & (kWave - 1));
  };
  static_assert(RLM == 3, "pivot() selects among three row groups");
  for (int c = 0; c + 1 < np; ++c) {  // L y = rhs, column sweep
    const double yc = pivot(c);
#pragma unroll
    for (int q = 0; q < RLM; ++q) {
      if (kWave * q < np) {
        const int r = lane + kWave * q;
        if (r < np && r > c && (r >= m || r - c <= K)) {
          const double l = r < m ? Lb[r * K1 + (r - c)] : W[(r - m) * np + c];
          y[q] = fma(-l, yc, y[q]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < RLM; ++q) { const int r = lane + kWave * q; if (r < np) y[q] *= dinv[r]; }
  for (int c = np - 1; c > 0; --c) {  // L' x = y
    const double xc = pivot(c);
#pragma unroll
    for (int q = 0; q < RLM; ++q) {
      if (kWave * q < c) {
        const int r = lane + kWave * q;
        if (r < c && (c >= m || c - r <= K)) {
          const double l = c < m ? Lb[c * K1 + (c - r)] : W[(c - m) * np + r];
          y[q] = fma(-l, xc, y[q]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < RLM; ++q) { const int r = lane + kWave * q; if (r < np) out[r] = y[q]; }
}

// Chunk partials -> span sums.  acc[0..NOUT) of every chunk thread go through Spart in rounds of
// kGRound outputs; task (span, output) adds the partials of the span's chunks in chunk order and
// stores the sum at Ssum[span * NO + out0 + output].
template <int NOUT, int NACC>
__device__ __forceinline__ void flush_outputs(const double (&acc)[NACC], bool has, int tid, int nthreads,
                                              int np, const int* sch, double* Spart, double* Ssum,
                                              int NO, int out0) {
#pragma unroll
  for (int r0 = 0; r0 < NOUT; r0 += kGRound) {
    const int w = NOUT - r0 < kGRound ? NOUT - r0 : kGRound;
    if (has) {
#pragma unroll
      for (int o = 0; o < kGRound; ++o)
        if (r0 + o < NOUT) Spart[tid * kGRound + o] = acc[r0 + o];
    }
    __syncthreads();
    for (int task = tid; task < np * w; task += nthreads) {
      const int sp = task / w, o = task - sp * w;
      double sum = 0.0;
      for (int ch = sch[sp]; ch < sch[sp + 1]; ++ch) sum += Spart[ch * kGRound + o];
      Ssum[sp * NO + out0 + r0 + o] = sum;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// the kernel, unweighted and speed-weighted (rl_global_kernel.hpp states the difference)
#define RL_GQ_WEIGHTED 0
#include "rl_global_kernel.hpp"
#undef RL_GQ_WEIGHTED
#define RL_GQ_WEIGHTED 1
#include "rl_global_kernel.hpp"
#undef RL_GQ_WEIGHTED

}  // namespace rl
