// rl_frenet.hpp -- global -> Frenet: the inverse of RaceTrack.frenet_to_global for B lines of P points in one launch, and a line's
// Frenet coordinates at given abscissae (gfx950; rl_frenet_batch_* / rl_frenet_resample_*).
//
//   k_frenet           (s, n, xi, g) of every point: the foot of the perpendicular on the closed centre line, GLOBALLY nearest
//   k_frenet_resample  (n, xi, channels) of a projected line at node abscissae, linear in s between the bracketing points
//
// The centre line is what k_pose_tables takes for RL_POSE_FRENET: M periodic cubic pieces x(s), y(s) (scipy CubicSpline:
// breakpoints ss[M+1], ss[M] = L; coefficients c[4][M], c[0] the cubic term), evaluated in ppoly_cubic's order of operations.
//
// k_frenet, one workgroup of kFrenetThreads per instance:
//   prologue  the coarse table, once per workgroup, in LDS: per piece a circle that contains it -- centre c_j(h_j / 2), a point
//             ON the piece, radius the largest distance of the piece's four Bezier control points from it (convex hull), widened
//             by a rounding margin.  With e = |p - centre|: e - r <= dist(p, piece j) <= e.  24 B per piece.
//   search    a thread owns a run of consecutive points.  An upper bound u on the distance to the line: the exact minimum over
//             the piece the thread's previous point landed on ("frenet_search" 1, the default; lines are ordered, so that piece
//             or a neighbour is almost always the answer) or, without one and always with "frenet_search" 0, the smallest e of
//             the table.  Then ONE pass over the table: a piece with e - r > u is dropped, every other piece is minimised
//             exactly and u shrinks to the best distance found.  A piece that holds a global minimiser has e - r <= the global
//             minimum <= u at all times, so it is never dropped, whatever u started from and in whatever order pieces are met.
//   minimise  on piece j, over its CLOSED interval: f(d) = (c(d) - p) . c'(d) sampled at kFrenetSub + 1 offsets, an |f| within
//             the rounding that c - p carries into it taken as 0; every sub-interval with f < 0 at its left and f >= 0 at its
//             right end holds a local minimum, refined by Newton on f safeguarded by the bracket (a step that leaves it, or
//             f' <= 0, is replaced by bisection) until f = 0 or a Newton step is below 2^-26 h, plus one more evaluation (the
//             better of the two by |f| is kept); at most kFrenetIters evaluations, else status 2 with the best iterate.  The
//             ends count as candidates where the distance decreases towards them (f(0) >= 0, f(h) < 0), so that a foot on a
//             breakpoint is found even when the two pieces that meet there round f to opposite sides of zero.
//   choice    the smallest squared distance, then the smallest piece index: a function of the SET of pieces minimised that is
//             the same for every superset of the pieces that hold a minimiser -- both searches return the same bits.  d = h
//             is handed to the next piece as d = 0 ("a foot on a breakpoint belongs to the piece that starts there"), s >= L
//             is returned as 0.
//   stats     per thread, then added up / compared by ONE lane in thread order (no floating-point atomics).
// Every loop is bounded by M, P, kFrenetSub or kFrenetIters.  Limits: M >= 3, P >= 1, and the table (24 M + 6 KiB) must fit LDS.
//
// The per-point functions are __host__ __device__, so that the search can be stepped through on a CPU build as well.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace rl {

constexpr int kFrenetThreads = 256;
constexpr int kFrenetSub = 8;      // sub-intervals of a piece that f is sampled on
constexpr int kFrenetIters = 48;   // evaluations of one refinement at most (bisection alone brings |f| below its rounding in about 45)

struct FrenetArgs {
  const double* points; int B, P, stride;   // [B,P,stride], x and y in columns 0, 1; stride 19: YAW in column 3
  const double* yaw;                        // [B,P] or null (stride 2 only)
  const double* ss; const double* cxs; const double* cys; int M;
  int search;                               // 0: every point from the table's own bound, 1: from the previous point's piece
  double* out;                              // [B,P,4] = (s, n, xi, g)
  int* status;                              // [B,P] or null: 0 ok, 1 non-finite coordinate, 2 iteration cap
  double* stats;                            // [B,4] or null: points with status != 0, min g, max |n| (both over status 0), most evaluations
};

// LDS carve of k_frenet in bytes, every offset a multiple of 16
struct FrenetLds { size_t off_cx, off_cy, off_r, off_g, off_n, off_bad, off_it, total_bytes; };
__host__ __device__ inline FrenetLds frenet_lds_layout(int M) {
  FrenetLds L;
  const size_t col = ((size_t)M * sizeof(double) + 15) & ~(size_t)15;
  size_t o = 0;
  L.off_cx = o; o += col;
  L.off_cy = o; o += col;
  L.off_r = o; o += col;
  L.off_g = o; o += (size_t)kFrenetThreads * sizeof(double);
  L.off_n = o; o += (size_t)kFrenetThreads * sizeof(double);
  L.off_bad = o; o += (size_t)kFrenetThreads * sizeof(int);
  L.off_it = o; o += (size_t)kFrenetThreads * sizeof(int);
  L.total_bytes = o;
  return L;
}

struct FrenetPiece { double h, ax[4], ay[4]; };   // a[0] the cubic term, offsets d in [0, h]
__host__ __device__ inline FrenetPiece frenet_load_piece(const double* __restrict__ ss, const double* __restrict__ cxs,
                                                         const double* __restrict__ cys, int M, int j) {
  FrenetPiece q;
  q.h = ss[j + 1] - ss[j];
#pragma unroll
  for (int r = 0; r < 4; ++r) { q.ax[r] = cxs[(size_t)r * M + j]; q.ay[r] = cys[(size_t)r * M + j]; }
  return q;
}
// value, first and second derivative of one coordinate at offset d: ppoly_cubic's order (scipy's evaluate_poly1)
__host__ __device__ inline void frenet_cubic(const double* a, double d, double& v, double& dv, double& d2v) {
#pragma clang fp contract(off)
  double z = d;
  v = a[3] + a[2] * z;
  dv = a[2] + a[1] * z * 2.0;
  d2v = a[1] * 2.0 + a[0] * z * 6.0;
  z *= d;
  v += a[1] * z;
  dv += a[0] * z * 3.0;
  z *= d;
  v += a[0] * z;
}
// c - p, c', f = (c - p) . c' with |f| <= nf (the rounding of c - p carried into f) taken as 0, f' = |c'|^2 + (c - p) . c''
struct FrenetEval { double ex, ey, dx, dy, f, fp; };
__host__ __device__ inline FrenetEval frenet_eval(const FrenetPiece& q, double d, double px, double py) {
#pragma clang fp contract(off)
  FrenetEval e;
  double x, y, d2x, d2y;
  frenet_cubic(q.ax, d, x, e.dx, d2x);
  frenet_cubic(q.ay, d, y, e.dy, d2y);
  e.ex = x - px; e.ey = y - py;
  e.f = e.ex * e.dx + e.ey * e.dy;
  const double nf = 0x1p-51 * ((fabs(x) + fabs(px)) * fabs(e.dx) + (fabs(y) + fabs(py)) * fabs(e.dy));
  if (fabs(e.f) <= nf) e.f = 0.0;
  e.fp = (e.dx * e.dx + e.dy * e.dy) + (e.ex * d2x + e.ey * d2y);
  return e;
}

// the circle of the coarse table for piece q
__host__ __device__ inline void frenet_circle(const FrenetPiece& q, double& cx, double& cy, double& r) {
#pragma clang fp contract(off)
  double dv, d2v;
  frenet_cubic(q.ax, 0.5 * q.h, cx, dv, d2v);
  frenet_cubic(q.ay, 0.5 * q.h, cy, dv, d2v);
  const double h = q.h, h3 = h / 3.0;
  double bx[4], by[4];   // Bezier control points of the piece
  bx[0] = q.ax[3]; by[0] = q.ay[3];
  bx[1] = q.ax[3] + q.ax[2] * h3; by[1] = q.ay[3] + q.ay[2] * h3;
  bx[2] = q.ax[3] + q.ax[2] * h3 * 2.0 + q.ax[1] * h * h3; by[2] = q.ay[3] + q.ay[2] * h3 * 2.0 + q.ay[1] * h * h3;
  frenet_cubic(q.ax, h, bx[3], dv, d2v);
  frenet_cubic(q.ay, h, by[3], dv, d2v);
  double r2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double ux = bx[i] - cx, uy = by[i] - cy;
    r2 = fmax(r2, ux * ux + uy * uy);
  }
  // rounding of the control points, of the centre and of the distances compared against r: far below 2^-40 of the magnitudes
  r = sqrt(r2) * (1.0 + 0x1p-30) + 0x1p-40 * (fabs(cx) + fabs(cy) + h);
}

struct FrenetBest { double D, d; int piece, iters, status; };   // piece < 0: nothing yet

// the minimum of |c_j(d) - p|^2 over the closed piece j; `best` takes it if it is smaller (or equal on a smaller piece index)
__host__ __device__ inline void frenet_piece_min(const FrenetPiece& q, int j, double px, double py, FrenetBest& best) {
#pragma clang fp contract(off)
  const double h = q.h, tol = 0x1p-26 * h;
  double cD = INFINITY, cd = 0.0;
  int cit = 0, cst = 0;
  auto offer = [&](double d, const FrenetEval& e, int it, int st) {
    const double D = e.ex * e.ex + e.ey * e.ey;
    if (D < cD) { cD = D; cd = d; cit = it; cst = st; }
  };
  double a = 0.0;
  FrenetEval ea = frenet_eval(q, 0.0, px, py);
  if (ea.f >= 0.0) offer(0.0, ea, 0, 0);
  for (int u = 1; u <= kFrenetSub; ++u) {
    const double b = u == kFrenetSub ? h : h * ((double)u / (double)kFrenetSub);
    const FrenetEval eb = frenet_eval(q, b, px, py);
    if (ea.f < 0.0 && eb.f >= 0.0) {
      if (eb.f == 0.0) {
        offer(b, eb, 0, 0);
      } else {
        double lo = a, hi = b;
        double x = a - ea.f * (b - a) / (eb.f - ea.f);
        if (!(x > lo && x < hi)) x = 0.5 * (lo + hi);
        double bx = x, bf = INFINITY;
        FrenetEval ebest = eb;
        int st = 2, it = 0;
        for (int k = 0; k < kFrenetIters; ++k) {
          const FrenetEval e = frenet_eval(q, x, px, py);
          ++it;
          if (fabs(e.f) < bf) { bf = fabs(e.f); bx = x; ebest = e; }
          if (e.f == 0.0) { st = 0; break; }
          if (e.f < 0.0) lo = x; else hi = x;
          double xn = e.fp > 0.0 ? x - e.f / e.fp : NAN;
          const bool newton = xn > lo && xn < hi;
          if (!newton) xn = 0.5 * (lo + hi);
          if (newton && fabs(xn - x) <= tol) {   // (a bisection step runs on: it ends at |f| <= its rounding, an exhausted bracket included)
            const FrenetEval e2 = frenet_eval(q, xn, px, py);
            ++it;
            if (fabs(e2.f) < bf) { bf = fabs(e2.f); bx = xn; ebest = e2; }
            st = 0;
            break;
          }
          x = xn;
        }
        if (bf < INFINITY) offer(bx, ebest, it, st);
      }
    }
    a = b; ea = eb;
  }
  if (ea.f < 0.0) offer(h, ea, 0, 0);
  if (cD < best.D || (cD == best.D && cD < INFINITY && j < best.piece)) {
    best.D = cD; best.d = cd; best.piece = j; best.iters = cit; best.status = cst;
  }
}

// one finite point against the table (tcx, tcy, tr: the circles, wherever they live); hint: a piece to start from, or -1
__host__ __device__ inline FrenetBest frenet_search(const double* __restrict__ ss, const double* __restrict__ cxs,
                                                    const double* __restrict__ cys, int M, const double* tcx, const double* tcy,
                                                    const double* tr, double px, double py, int hint) {
#pragma clang fp contract(off)
  FrenetBest best{INFINITY, 0.0, -1, 0, 0};
  double lim;
  if (hint >= 0) {
    frenet_piece_min(frenet_load_piece(ss, cxs, cys, M, hint), hint, px, py, best);
    lim = sqrt(best.D);
  } else {
    double e2 = INFINITY;
    for (int j = 0; j < M; ++j) {
      const double ux = px - tcx[j], uy = py - tcy[j];
      e2 = fmin(e2, ux * ux + uy * uy);
    }
    lim = sqrt(e2);
  }
  // every lane walks to ITS next surviving piece, then the lanes minimise together
  int j = 0;
  while (j < M) {
    bool hit = false;
    for (; j < M && !hit; ++j) {
      if (j == hint) continue;
      const double ux = px - tcx[j], uy = py - tcy[j], t = lim + tr[j];
      hit = !(ux * ux + uy * uy > t * t);
    }
    if (hit) {
      frenet_piece_min(frenet_load_piece(ss, cxs, cys, M, j - 1), j - 1, px, py, best);
      lim = fmin(lim, sqrt(best.D));
    }
  }
  return best;
}

// (s, n, xi, g) at the chosen foot; have_yaw false: xi = 0
__host__ __device__ inline void frenet_finish(const double* __restrict__ ss, const double* __restrict__ cxs,
                                              const double* __restrict__ cys, int M, FrenetBest best, double px, double py,
                                              bool have_yaw, double yaw, double* o) {
#pragma clang fp contract(off)
  int j = best.piece;
  double d = best.d;
  if (d >= ss[j + 1] - ss[j]) { j = j + 1 < M ? j + 1 : 0; d = 0.0; }
  const FrenetEval e = frenet_eval(frenet_load_piece(ss, cxs, cys, M, j), d, px, py);
  const double v2 = e.dx * e.dx + e.dy * e.dy;
  double s = ss[j] + d;
  if (s >= ss[M]) s = 0.0;
  o[0] = s;
  o[1] = (e.ex * e.dy - e.ey * e.dx) / sqrt(v2);   // (p - c) . (-c'_y, c'_x) / |c'|
  double xi = 0.0;
  if (have_yaw) {
    const double dd = yaw - atan2(e.dy, e.dx);
    xi = atan2(sin(dd), cos(dd));
  }
  o[2] = xi;
  o[3] = e.fp / v2;
}

__global__ __launch_bounds__(kFrenetThreads) void k_frenet(FrenetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char frenet_smem[];
  constexpr int BLOCK = kFrenetThreads;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M, P = a.P, stride = a.stride;
  const FrenetLds L = frenet_lds_layout(M);
  double* tcx = reinterpret_cast<double*>(frenet_smem + L.off_cx);
  double* tcy = reinterpret_cast<double*>(frenet_smem + L.off_cy);
  double* tr = reinterpret_cast<double*>(frenet_smem + L.off_r);
  double* red_g = reinterpret_cast<double*>(frenet_smem + L.off_g);
  double* red_n = reinterpret_cast<double*>(frenet_smem + L.off_n);
  int* red_bad = reinterpret_cast<int*>(frenet_smem + L.off_bad);
  int* red_it = reinterpret_cast<int*>(frenet_smem + L.off_it);

  for (int j = tid; j < M; j += BLOCK) frenet_circle(frenet_load_piece(a.ss, a.cxs, a.cys, M, j), tcx[j], tcy[j], tr[j]);
  __syncthreads();

  const double* pts = a.points + (size_t)b * P * stride;
  const double* yw = stride == 19 ? nullptr : (a.yaw ? a.yaw + (size_t)b * P : nullptr);
  const bool have_yaw = stride == 19 || yw != nullptr;
  double* out = a.out + (size_t)b * P * 4;
  int* stat = a.status ? a.status + (size_t)b * P : nullptr;
  const int chunk = (P + BLOCK - 1) / BLOCK;
  const int i0 = min(P, tid * chunk), i1 = min(P, i0 + chunk);
  double ming = INFINITY, maxn = 0.0;
  int nbad = 0, maxit = 0, hint = -1;
  for (int i = i0; i < i1; ++i) {
    const double px = pts[(size_t)i * stride], py = pts[(size_t)i * stride + 1];
    double o[4] = {NAN, NAN, NAN, NAN};
    int st = 1;
    if (isfinite(px) && isfinite(py)) {
      const FrenetBest best = frenet_search(a.ss, a.cxs, a.cys, M, tcx, tcy, tr, px, py, a.search ? hint : -1);
      st = 2;
      if (best.piece >= 0) {
        st = best.status;
        const double yaw = stride == 19 ? pts[(size_t)i * stride + 3] : (yw ? yw[i] : 0.0);
        frenet_finish(a.ss, a.cxs, a.cys, M, best, px, py, have_yaw, yaw, o);
        maxit = max(maxit, best.iters);
        hint = best.piece;
      }
    }
    if (st == 0) { ming = fmin(ming, o[3]); maxn = fmax(maxn, fabs(o[1])); } else { ++nbad; }
    if (st != 0) hint = -1;
    out[(size_t)i * 4] = o[0]; out[(size_t)i * 4 + 1] = o[1]; out[(size_t)i * 4 + 2] = o[2]; out[(size_t)i * 4 + 3] = o[3];
    if (stat) stat[i] = st;
  }
  if (a.stats) {   // (uniform)
    red_g[tid] = ming; red_n[tid] = maxn; red_bad[tid] = nbad; red_it[tid] = maxit;
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < BLOCK; ++q) {
        ming = fmin(ming, red_g[q]); maxn = fmax(maxn, red_n[q]); nbad += red_bad[q]; maxit = max(maxit, red_it[q]);
      }
      double* so = a.stats + (size_t)b * 4;
      so[0] = (double)nbad; so[1] = ming; so[2] = maxn; so[3] = (double)maxit;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_frenet_resample: per instance fr[P,4] of k_frenet, channels vals[P,C] (or null), node abscissae s_nodes[Nn] shared by the
// batch -> out[Nn,2+C] = (n, xi, channels) at the nodes.  The s_i must be finite and cyclically strictly increasing: exactly one i
// with s_{(i+1) % P} <= s_i (the wrap); otherwise status 1 and rows of zeros.  Per node (wrapped into [0, L)): the bracketing
// pair by binary search in the sequence rotated to start behind the wrap, the wrap pair bridged with + L; n, xi and the channels
// linear in s in numpy.interp's form slope * (q - s_l) + v_l, the right neighbour's xi first brought to within pi of the left one.
constexpr int kResampleThreads = 256;

__host__ __device__ inline void frenet_resample_node(const double* __restrict__ fr, const double* __restrict__ vals, int C, int P,
                                                     int k0, double len, double node, double* __restrict__ o) {
#pragma clang fp contract(off)
  double q = fmod(node, len);
  if (q != 0.0 && q < 0.0) q += len;
  auto s_at = [&](int m) { int i = k0 + m; if (i >= P) i -= P; return fr[(size_t)i * 4]; };
  int ml, mr;
  double sl, sr;
  if (q < s_at(0)) {
    ml = P - 1; mr = 0; sl = s_at(P - 1) - len; sr = s_at(0);
  } else {
    int lo = 0, hi = P;   // s_at(lo) <= q < s_at(hi), s_at(P) = +inf
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_at(mid) <= q) lo = mid; else hi = mid;
    }
    ml = lo; sl = s_at(lo);
    if (lo + 1 < P) { mr = lo + 1; sr = s_at(mr); } else { mr = 0; sr = s_at(0) + len; }
  }
  int il = k0 + ml, ir = k0 + mr;
  if (il >= P) il -= P;
  if (ir >= P) ir -= P;
  const double ds = sr - sl, dq = q - sl;
  auto lerp = [&](double vl, double vr) { return (vr - vl) / ds * dq + vl; };
  o[0] = lerp(fr[(size_t)il * 4 + 1], fr[(size_t)ir * 4 + 1]);
  const double xl = fr[(size_t)il * 4 + 2], dx = fr[(size_t)ir * 4 + 2] - xl;
  o[1] = lerp(xl, atan2(sin(dx), cos(dx)) + xl);
  for (int c = 0; c < C; ++c) o[2 + c] = lerp(vals[(size_t)il * C + c], vals[(size_t)ir * C + c]);
}

__global__ __launch_bounds__(kResampleThreads) void k_frenet_resample(const double* __restrict__ fr, const double* __restrict__ vals,
                                                                      int C, int P, const double* __restrict__ s_nodes, int Nn,
                                                                      double len, double* __restrict__ out, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resample_smem[];
  int* flags = reinterpret_cast<int*>(resample_smem);   // [0] descents, [1] index behind the descent, [2] bad points
  constexpr int BLOCK = kResampleThreads;
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* frb = fr + (size_t)b * P * 4;
  const double* vb = vals ? vals + (size_t)b * P * C : nullptr;
  double* ob = out + (size_t)b * Nn * (2 + C);
  if (tid < 4) flags[tid] = 0;
  __syncthreads();
  int desc = 0, pos = 0, bad = 0;
  for (int i = tid; i < P; i += BLOCK) {
    const int i1 = i + 1 < P ? i + 1 : 0;
    const double s0 = frb[(size_t)i * 4], s1 = frb[(size_t)i1 * 4];
    if (!isfinite(s0) || !isfinite(frb[(size_t)i * 4 + 1]) || !isfinite(frb[(size_t)i * 4 + 2])) bad = 1;
    if (s1 <= s0) { ++desc; pos = i1; }
  }
  if (desc) { atomicAdd(&flags[0], desc); atomicMax(&flags[1], pos); }   // (integers: the same whatever the order)
  if (bad) flags[2] = 1;
  __syncthreads();
  const bool ok = flags[0] == 1 && flags[2] == 0;
  const int k0 = flags[1];
  const int W = 2 + C;
  for (int j = tid; j < Nn; j += BLOCK) {
    if (ok) frenet_resample_node(frb, vb, C, P, k0, len, s_nodes[j], ob + (size_t)j * W);
    else for (int c = 0; c < W; ++c) ob[(size_t)j * W + c] = 0.0;
  }
  if (tid == 0) status[b] = ok ? 0 : 1;
}

}  // namespace rl
