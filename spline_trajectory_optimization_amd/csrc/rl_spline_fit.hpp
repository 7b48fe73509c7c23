// rl_spline_fit.hpp -- k_spline_fit<K>: periodic least-squares B-spline fit of P points per instance ONTO THE TRACK'S KNOTS, one
// workgroup per instance (rl_spline_fit_batch_*).  What scipy's splprep(task=-1, per=True, t=knots)
// (FITPACK clocur) returns, by the normal equations:
//
//   1. parameters   given, or chord length of the closed polygon (block-wise running sums in a fixed order); knot span per point
//   2. lists        the points of every span, in point order (one thread per span walks the span numbers: no sort, no atomics on data)
//   3. accumulation one thread per span adds the (k+1)(k+2)/2 basis products and 2(k+1) right-hand-side terms of its points in
//                   list order; entry (i, i+d) of the cyclic band G = A^T A then adds its k+1-d spans in span order.  Every sum
//                   has ONE order, fixed by the input alone: the same points give the same bits in every run and at every batch
//                   position (no floating-point atomics anywhere)
//   4. solve        G = [[G11, G12], [G12^T, G22]] with G11 banded (half-bandwidth k) and the last k unknowns as the border
//                   that carries the periodic corners: Cholesky of G11 (rows in registers), forward solves of the k border
//                   columns and the two right-hand sides, the k x k Schur complement, back substitution.  The pivots are those
//                   of the Cholesky factorisation of G in its natural order, so smallest pivot / largest diagonal >= 1 / cond2(G)
//   5. residuals    second pass over the points with the fitted coefficients
#pragma once
#include "rl_device.hpp"

namespace rl {

constexpr int kFitThreads = 256;
constexpr int kFitMaxM = 192;     // n - k unknowns per coordinate
constexpr int kFitMaxP = 4096;    // points per instance (span numbers and point indices are kept as 16-bit values)
constexpr double kFitRankTol = 1e-12;   // smallest pivot <= kFitRankTol * largest diagonal: rank deficient (rl_mincurv.h derives it)

__host__ __device__ constexpr int fit_pairs(int k) { return (k + 1) * (k + 2) / 2; }
__host__ __device__ constexpr int fit_nacc(int k) { return fit_pairs(k) + 2 * (k + 1); }

// LDS carve of k_spline_fit (offsets in doubles; the 16-bit arrays and the counters behind them)
struct FitLds {
  size_t off_u, off_W, off_G, off_rhs, off_L, off_Y, off_S, off_x, off_red, doubles;
  size_t off_span_b, off_list_b, off_cnt_b, total_bytes;
};
__host__ __device__ inline FitLds fit_lds_layout(int k, int m, int P) {
  FitLds L;
  const size_t Pp = (size_t)(P + 3) & ~(size_t)3;
  size_t o = 0;
  L.off_u = o; o += Pp;
  L.off_W = o; o += (size_t)m * fit_nacc(k);
  L.off_G = o; o += (size_t)m * (k + 1);
  L.off_rhs = o; o += (size_t)2 * m;
  L.off_L = o; o += (size_t)m * (k + 1);
  L.off_Y = o; o += (size_t)m * (k + 2);
  L.off_S = o; o += (size_t)kMaxK * kMaxK + 2 * kMaxK + 2;
  L.off_x = o; o += (size_t)2 * m;
  L.off_red = o; o += (size_t)2 * kFitThreads;
  L.doubles = o;
  size_t bytes = o * sizeof(double);
  L.off_span_b = bytes; bytes += Pp * sizeof(unsigned short);
  L.off_list_b = bytes; bytes += Pp * sizeof(unsigned short);
  L.off_cnt_b = bytes; bytes += (size_t)(m + 4) * sizeof(int);
  L.total_bytes = (bytes + 15) & ~(size_t)15;
  return L;
}

template <int K>
__global__ __launch_bounds__(kFitThreads) void k_spline_fit(TrackDev tr, const double* __restrict__ xy, int P, int stride,
                                                             const double* __restrict__ u, int u_per_instance,
                                                             double* __restrict__ out_ctrl, double* __restrict__ out_stats) {
  constexpr int K1 = K + 1, NP = fit_pairs(K), NACC = fit_nacc(K), BLOCK = kFitThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char fit_smem[];
  const int n = tr.n, m = n - K, M1 = m - K;
  const int b = blockIdx.x, tid = threadIdx.x;
  const FitLds L = fit_lds_layout(K, m, P);
  double* smem = reinterpret_cast<double*>(fit_smem);
  double* up = smem + L.off_u;        // [P] spline parameter of every point
  double* W = smem + L.off_W;         // [m][NACC] per-span sums
  double* Gb = smem + L.off_G;        // [m][K+1] cyclic band: Gb[i][d] = G[i][(i + d) mod m]
  double* rhs = smem + L.off_rhs;     // [m][2]
  double* Lb = smem + L.off_L;        // [M1][K+1]: [0] = 1 / L[i][i], [d] = L[i][i-d]
  double* Y = smem + L.off_Y;         // [M1][K+2]: L^-1 (k border columns | rhs x | rhs y)
  double* Sm = smem + L.off_S;        // [K][K] Schur complement, then [K][2] its right-hand sides, then 2 scalars
  double* xs = smem + L.off_x;        // [m][2] the solution
  double* red = smem + L.off_red;     // [2][BLOCK]
  unsigned short* span = reinterpret_cast<unsigned short*>(fit_smem + L.off_span_b);   // [P]
  unsigned short* list = reinterpret_cast<unsigned short*>(fit_smem + L.off_list_b);   // [P] point indices, span after span
  int* cnt = reinterpret_cast<int*>(fit_smem + L.off_cnt_b);   // [m+1] points per span -> offsets; [m+1] = bad input, [m+2] = bad result
  const double* pts = xy + (size_t)b * P * stride;
  const double* __restrict__ t = tr.t;
  const double t0 = t[K], tspan = t[n] - t[K];

  for (int s = tid; s < m + 4; s += BLOCK) cnt[s] = 0;
  __syncthreads();

  // ---- 1. parameters
  bool bad = false;
  if (u) {
    const double* ub = u + (u_per_instance ? (size_t)b * P : 0);
    for (int p = tid; p < P; p += BLOCK) up[p] = ub[p];
  } else {
    // chord length of the closed polygon: thread q adds the chords of its block of consecutive points in order, the block
    // totals are added up in block order
    const int chunk = (P + BLOCK - 1) / BLOCK;
    const int p0 = min(P, tid * chunk), p1 = min(P, p0 + chunk);
    double run = 0.0;
    for (int p = p0; p < p1; ++p) {
      const int q = p + 1 < P ? p + 1 : 0;
      const double ex = pts[(size_t)q * stride] - pts[(size_t)p * stride];
      const double ey = pts[(size_t)q * stride + 1] - pts[(size_t)p * stride + 1];
      up[p] = run;
      run += sqrt(ex * ex + ey * ey);
    }
    red[tid] = run;
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (int q = 0; q < BLOCK; ++q) { const double v = red[q]; red[q] = acc; acc += v; }
      red[BLOCK] = acc;   // the perimeter
    }
    __syncthreads();
    const double base = red[tid], perimeter = red[BLOCK];
    for (int p = p0; p < p1; ++p) up[p] = (base + up[p]) / perimeter;
  }
  __syncthreads();
  // knot span of every point; 1 is taken as 0; a parameter outside [0, 1) or a non-finite coordinate: status 2
  for (int p = tid; p < P; p += BLOCK) {
    double v = up[p];
    if (v == 1.0) v = 0.0;
    const double px = pts[(size_t)p * stride], py = pts[(size_t)p * stride + 1];
    int s = 0;
    if (!(v >= 0.0 && v < 1.0) || !isfinite(px) || !isfinite(py)) {
      bad = true;
    } else {
      v = t0 + v * tspan;
      s = find_interval(t, K, n, v) - K;
      atomicAdd(&cnt[s], 1);   // (an integer count: the same whatever the order)
    }
    up[p] = v;
    span[p] = (unsigned short)s;
  }
  if (bad) cnt[m + 1] = 1;
  __syncthreads();
  const bool bad_input = cnt[m + 1] != 0;

  double ratio = NAN, rms = NAN, rmax = NAN;
  int status = bad_input ? 2 : 0;
  if (!bad_input) {   // (uniform: every barrier below is reached by the whole workgroup)
    // ---- 2. the points of every span in point order
    if (tid == 0) {
      int acc = 0;
      for (int s = 0; s < m; ++s) { const int c = cnt[s]; cnt[s] = acc; acc += c; }
      cnt[m] = acc;
    }
    __syncthreads();
    if (tid < m) {
      int o = cnt[tid];
      for (int p = 0; p < P; ++p)
        if (span[p] == tid) list[o++] = (unsigned short)p;
    }
    __syncthreads();
    // ---- 3. per-span sums in list order, then the band and the right-hand sides in span order
    if (tid < m) {
      double acc[NACC];
#pragma unroll
      for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
      const int r0 = cnt[tid], r1 = cnt[tid + 1];
      for (int r = r0; r < r1; ++r) {
        const int p = list[r];
        double h[K1];
        deboor<K>(t, up[p], K + tid, 0, h);
        const double px = pts[(size_t)p * stride], py = pts[(size_t)p * stride + 1];
        int q = 0;
#pragma unroll
        for (int a = 0; a < K1; ++a)
#pragma unroll
          for (int a2 = a; a2 < K1; ++a2) { acc[q] += h[a] * h[a2]; ++q; }
#pragma unroll
        for (int a = 0; a < K1; ++a) { acc[NP + a] += h[a] * px; acc[NP + K1 + a] += h[a] * py; }
      }
#pragma unroll
      for (int q = 0; q < NACC; ++q) W[(size_t)tid * NACC + q] = acc[q];
    }
    __syncthreads();
    for (int e = tid; e < m * K1; e += BLOCK) {
      const int i = e / K1, d = e % K1;
      double sum = 0.0;
      for (int a = K - d; a >= 0; --a) {       // spans i+d-K .. i: basis i is local function a, basis i+d local function a+d
        int s = i - a;
        if (s < 0) s += m;
        sum += W[(size_t)s * NACC + a * K1 - a * (a - 1) / 2 + d];
      }
      Gb[e] = sum;
    }
    for (int e = tid; e < 2 * m; e += BLOCK) {
      const int i = e >> 1, r = e & 1;
      double sum = 0.0;
      for (int a = K; a >= 0; --a) {
        int s = i - a;
        if (s < 0) s += m;
        sum += W[(size_t)s * NACC + NP + r * K1 + a];
      }
      rhs[e] = sum;
    }
    __syncthreads();
    // ---- 4. Cholesky of the banded block G11 (rows 0 .. M1-1), the last K rows of L in registers
    if (tid == 0) {
      double R[K][K1];   // R[q-1] = row i-q: [0] = 1 / diagonal, [d] = L[i-q][i-q-d]; rows before the first are zero
#pragma unroll
      for (int q = 0; q < K; ++q) {
        R[q][0] = 1.0;
#pragma unroll
        for (int d = 1; d < K1; ++d) R[q][d] = 0.0;
      }
      double minpiv = INFINITY, maxdiag = 0.0;
      for (int i = 0; i < m; ++i) maxdiag = fmax(maxdiag, Gb[i * K1]);
      for (int i = 0; i < M1; ++i) {
        double nw[K1];
#pragma unroll
        for (int d = K; d >= 1; --d) {
          const int j = i - d;
          double sum = j >= 0 ? Gb[j * K1 + d] : 0.0;
#pragma unroll
          for (int e = K; e > d; --e) sum -= nw[e] * R[d - 1][e - d];
          nw[d] = sum * R[d - 1][0];
        }
        double piv = Gb[i * K1];
#pragma unroll
        for (int e = K; e >= 1; --e) piv -= nw[e] * nw[e];
        minpiv = fmin(minpiv, piv);
        nw[0] = 1.0 / sqrt(piv);
#pragma unroll
        for (int d = 0; d < K1; ++d) Lb[i * K1 + d] = nw[d];
#pragma unroll
        for (int q = K - 1; q >= 1; --q)
#pragma unroll
          for (int d = 0; d < K1; ++d) R[q][d] = R[q - 1][d];
#pragma unroll
        for (int d = 0; d < K1; ++d) R[0][d] = nw[d];
      }
      Sm[K * K + 2 * K] = minpiv;
      Sm[K * K + 2 * K + 1] = maxdiag;
    }
    __syncthreads();
    // forward solves: lane c < K the border column c (unknown M1 + c), lanes K, K+1 the two right-hand sides
    if (tid < K + 2) {
      const int c = tid;
      double yw[K];   // yw[d-1] = y[i-d]
#pragma unroll
      for (int d = 0; d < K; ++d) yw[d] = 0.0;
      for (int i = 0; i < M1; ++i) {
        double v;
        if (c < K) {
          const int d = M1 + c - i, d2 = m - d;   // forward / backward cyclic distance of (i, M1 + c): at most one is <= K
          v = d <= K ? Gb[i * K1 + d] : (d2 <= K ? Gb[(M1 + c) * K1 + d2] : 0.0);
        } else {
          v = rhs[2 * i + (c - K)];
        }
#pragma unroll
        for (int d = K; d >= 1; --d) v -= Lb[i * K1 + d] * yw[d - 1];
        v *= Lb[i * K1];
        Y[i * (K + 2) + c] = v;
#pragma unroll
        for (int d = K - 1; d >= 1; --d) yw[d] = yw[d - 1];
        yw[0] = v;
      }
    }
    __syncthreads();
    // Schur complement of the border and its right-hand sides: one entry per lane, each a sum in row order
    if (tid < K * K) {
      const int c = tid / K, c2 = tid % K;
      if (c <= c2) {
        double v = Gb[(M1 + c) * K1 + (c2 - c)];
        for (int i = 0; i < M1; ++i) v -= Y[i * (K + 2) + c] * Y[i * (K + 2) + c2];
        Sm[c * K + c2] = v;
        Sm[c2 * K + c] = v;
      }
    } else if (tid < K * K + 2 * K) {
      const int e = tid - K * K, c = e >> 1, r = e & 1;
      double v = rhs[2 * (M1 + c) + r];
      for (int i = 0; i < M1; ++i) v -= Y[i * (K + 2) + c] * Y[i * (K + 2) + K + r];
      Sm[K * K + e] = v;
    }
    __syncthreads();
    if (tid == 0) {   // Cholesky of the K x K complement, its two solves, the verdict on the pivots
      double minpiv = Sm[K * K + 2 * K];
      const double maxdiag = Sm[K * K + 2 * K + 1];
      double S[K][K], inv[K], z[K][2];
#pragma unroll
      for (int c = 0; c < K; ++c)
#pragma unroll
        for (int c2 = 0; c2 < K; ++c2) S[c][c2] = Sm[c * K + c2];
#pragma unroll
      for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int j = 0; j < c; ++j) {
          double v = S[c][j];
#pragma unroll
          for (int q = 0; q < j; ++q) v -= S[c][q] * S[j][q];
          S[c][j] = v * inv[j];
        }
        double piv = S[c][c];
#pragma unroll
        for (int q = 0; q < c; ++q) piv -= S[c][q] * S[c][q];
        minpiv = fmin(minpiv, piv);
        inv[c] = 1.0 / sqrt(piv);
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
          double v = Sm[K * K + 2 * c + r];
#pragma unroll
          for (int q = 0; q < c; ++q) v -= S[c][q] * z[q][r];
          z[c][r] = v * inv[c];
        }
#pragma unroll
        for (int c = K - 1; c >= 0; --c) {
          double v = z[c][r];
#pragma unroll
          for (int q = c + 1; q < K; ++q) v -= S[q][c] * z[q][r];
          z[c][r] = v * inv[c];
          xs[2 * (M1 + c) + r] = z[c][r];
        }
      }
      Sm[K * K + 2 * K] = minpiv / maxdiag;
      if (!(minpiv > kFitRankTol * maxdiag)) cnt[m + 1] = 1;   // rank deficient (or not positive, or NaN)
    }
    __syncthreads();
    // back substitution, one coordinate per lane: L^T x1 = y - Y x2
    if (tid < 2) {
      const int r = tid;
      double x2[K], xw[K];   // xw[d-1] = x[i+d]
#pragma unroll
      for (int c = 0; c < K; ++c) { x2[c] = xs[2 * (M1 + c) + r]; xw[c] = 0.0; }
      for (int i = M1 - 1; i >= 0; --i) {
        double v = Y[i * (K + 2) + K + r];
#pragma unroll
        for (int c = 0; c < K; ++c) v -= Y[i * (K + 2) + c] * x2[c];
#pragma unroll
        for (int d = K; d >= 1; --d)
          if (i + d < M1) v -= Lb[(i + d) * K1 + d] * xw[d - 1];
        v *= Lb[i * K1];
        xs[2 * i + r] = v;
#pragma unroll
        for (int d = K - 1; d >= 1; --d) xw[d] = xw[d - 1];
        xw[0] = v;
      }
    }
    __syncthreads();
    ratio = Sm[K * K + 2 * K];
    if (cnt[m + 1] != 0) {
      status = 1;
    } else {
      // ---- 5. a non-finite result; the residuals (every thread its points in order, the threads' sums in thread order)
      bool nf = false;
      for (int e = tid; e < 2 * m; e += BLOCK) nf |= !isfinite(xs[e]);
      if (nf) cnt[m + 2] = 1;
      double s2 = 0.0, mx = 0.0;
      for (int p = tid; p < P; p += BLOCK) {
        const int s = span[p];
        double h[K1];
        deboor<K>(t, up[p], K + s, 0, h);
        double fx = 0.0, fy = 0.0;
#pragma unroll
        for (int a = 0; a < K1; ++a) {
          int j = s + a;
          if (j >= m) j -= m;
          fx += h[a] * xs[2 * j];
          fy += h[a] * xs[2 * j + 1];
        }
        const double ex = pts[(size_t)p * stride] - fx, ey = pts[(size_t)p * stride + 1] - fy;
        const double r2 = ex * ex + ey * ey;
        s2 += r2;
        mx = fmax(mx, r2);
      }
      red[tid] = s2;
      red[BLOCK + tid] = mx;
      __syncthreads();
      if (cnt[m + 2] != 0) {
        status = 2;
      } else {
        double acc = 0.0, top = 0.0;
        for (int q = 0; q < BLOCK; ++q) { acc += red[q]; top = fmax(top, red[BLOCK + q]); }
        rms = sqrt(acc / (double)P);
        rmax = sqrt(top);
      }
    }
  }
  // ---- output: the fit in scipy's periodic layout, or (status != 0) the track's initial control points
  double2* oc = reinterpret_cast<double2*>(out_ctrl) + (size_t)b * n;
  for (int j = tid; j < n; j += BLOCK) {
    if (status == 0) {
      const int q = j >= m ? j - m : j;
      oc[j] = make_double2(xs[2 * q], xs[2 * q + 1]);
    } else {
      oc[j] = make_double2(tr.c0[j], tr.c0[n + j]);
    }
  }
  if (tid == 0) {
    double* o = out_stats + (size_t)b * 4;
    o[0] = (double)status; o[1] = rms; o[2] = rmax; o[3] = ratio;
  }
}

}  // namespace rl
