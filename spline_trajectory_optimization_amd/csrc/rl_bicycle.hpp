// rl_bicycle.hpp -- the min-time NLP of the reference's set_up_bicycle_problem (min_time_optm/min_time_optimizer.py:14-90)
// on the GPU: its functions and its solve for B instances.
//
// The NLP (closed lap, node j = the reference's loop turn i = j + 1, pair (j, j+1) wrapping around), per node 8 scaled
// unknowns w = (X[5], U[2], T): x = X * (10, 10, 3.14, 0.1, 80) + (P0, 0, 0, 0), u = U * (20, 1) (:33-35).  Cost sum T
// (:9-10).  Equalities: the RK4 defect of x_j -> x_{j+1} over T_j with u_j after aligning theta_{j+1} to theta_j
// (:55-56; utils/integrator.py:13-19), the longitudinal Frenet coordinate of x_j - P0_j is 0 (:59-65).  Inequalities: the
// lateral Frenet coordinate in [-|BoundR - P0|, |BoundL - P0|] (:66-68), the traction circle lat^2 + lon^2 <= acc_max^2
// (:71-74; models/dynamic_bicycle.py:4-23, :65-71), box bounds on delta, v, a, delta_dot (:86-87; models/dynamic_bicycle.py
// :34-54), T >= 0 (:88).
//
// Solve: primal-dual interior point (barrier, IPOPT's update rules), one kernel launch per iteration and one workgroup of
// 256 threads per instance.  The two general inequalities get slacks, condensed into the node's 8 x 8 block, so the
// Newton system is a cyclic block-tridiagonal KKT matrix with 14 x 14 node blocks (8 unknowns + 6 multipliers); the only
// coupling of node j+1 into pair j is -x_{j+1} * scale in the defect, i.e. a constant.  The blocks are eliminated
// node by node in order (in-place Gauss-Jordan inversion of each pivot block, one entry per thread), carrying the
// wrap-around coupling as a border on the last node; the signs of the pivots give the inertia, which must be
// 6N negative, else the unknowns' diagonal is regularised (IPOPT's delta_w rule).  Exact Hessian of the pair's
// Lagrangian (only theta, delta, v, a, delta_dot, T carry curvature) by forward-over-forward duals (rl_dtrack.hpp).
// Fraction to the boundary, filter line search with backtracking, IPOPT's z safeguard.  CPU twin: tests/bicycle_twin.py.
//
// Two forms of the problem data, one text of the kernels: BkProblem (one model, one line for the batch; only dl / dr may
// differ per instance) and BkProblemV (model, line and bounds of instance b from row b of device tables), see there.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_dtrack.hpp"

namespace rl {

// parameter slots (include/rl_mincurv.h: RL_BK_*)
enum BkParam { BK_LR, BK_L, BK_DELTA_MAX, BK_V_MAX, BK_A_LON_MAX, BK_A_LON_MIN, BK_DELTA_DOT_MAX, BK_ACC_MAX, BK_NPARAM };
constexpr int kBkNv = 8, kBkNe = 6, kBkNb = 10, kBkK = 14, kBkKK = kBkK * kBkK;
constexpr int kBkThreads = 256, kBkFilter = 256, kBkScal = 16, kBkStats = 12;   // kBkStats: doubles per instance of the caller's report, scal 0-11
constexpr int kBkNd = 2, kBkJd = kBkNd * kBkNv;   // the two inequality functions (lateral, traction) and their Jacobian rows
static_assert(kBkKK <= kBkThreads, "one thread per entry of a 14 x 14 block");
// the reference's variable scaling (:33-35)
__device__ constexpr double kBkSx[5] = {10.0, 10.0, 3.14, 0.1, 80.0};
__device__ constexpr double kBkSu[2] = {20.0, 1.0};
// interior-point constants (tests/bicycle_twin.py holds the same)
constexpr double kBkMu0 = 0.1, kBkKappaEps = 10.0, kBkKappaMu = 0.2, kBkThetaMu = 1.5, kBkTauMin = 0.99;
constexpr double kBkDeltaC = 1e-10, kBkKappaSigma = 1e10;
constexpr double kBkGammaTh = 1e-5, kBkGammaPhi = 1e-8, kBkEta = 1e-4, kBkSTh = 1.1, kBkSPhi = 2.3;
constexpr int kBkMaxHalvings = 20;
constexpr double kBkDw0 = 1e-4, kBkDwFirstUp = 100.0, kBkDwUp = 8.0, kBkDwDown = 1.0 / 3.0, kBkDwMax = 1e40;
constexpr double kBkPivRel = 1e-10;

// scal[B][16]: 0-11 as stats (iterations, dual inf, constraint violation, complementarity, lap time, status, mu, delta_w,
// step length, refactorisations, fraction-to-the-boundary step, halvings), 12 done, 13 theta_max, 14 theta_min, 15 filter size
enum { BS_IT, BS_DUAL, BS_PRIM, BS_COMP, BS_LAP, BS_STATUS, BS_MU, BS_DW, BS_ALPHA, BS_REFAC, BS_AMAX, BS_HALV, BS_DONE,
       BS_THMAX, BS_THMIN, BS_NFILT };

struct BkProblem {
  double m[BK_NPARAM];
  int N, per;            // per: dl / dr are [B,N] (else [N])
  const double* P0;      // [N,2]
  const double* yaw;     // [N]
  const double* dl;      // > 0
  const double* dr;      // < 0
  double tol;
};

// One line and one vehicle per instance (rl_bicycle_solve_lines*): the model of instance b is row b of a table
// [B, BK_NPARAM] in device memory instead of a kernel argument, and with `lines` P0 / yaw are [B,N,2] / [B,N].  Every kernel
// takes its instance from blockIdx, so a row's address is the same in all lanes; bk_instance moves the pointers to the
// instance's rows once, at the kernel's head, and everything below reads P.m[], P.P0[], P.yaw[] with the text it reads them
// with from BkProblem -- node j+1 of the wrap-around pair included, which is then the instance's own P0 at jn.  The table
// pointer is in the constant address space (the table is written by a copy that is complete before the first kernel of the
// solve starts, and by nothing else), as the model table of rl_mintime.hpp: a value is a scalar load whatever the kernel
// stores in between.  The kernels and the device functions that read the problem are templates over the problem type:
// <BkProblem> is what the shared-model entries launch, <BkProblemV> what the per-instance entries launch.
typedef const double __attribute__((address_space(4))) * BkTab;
struct BkProblemV {
  BkTab m;               // row 0 of the table [B, BK_NPARAM]
  int N, per, lines;     // per: dl / dr are [B,N] (else [N]); lines: P0 [B,N,2], yaw [B,N] (else [N,2], [N])
  const double* P0;
  const double* yaw;
  const double* dl;
  const double* dr;
  double tol;
};
__device__ __forceinline__ void bk_instance(BkProblem&, int) {}
__device__ __forceinline__ void bk_instance(BkProblemV& P, int b) {
  P.m += (size_t)b * BK_NPARAM;
  if (P.lines) { P.P0 += (size_t)b * P.N * 2; P.yaw += (size_t)b * P.N; }
}

struct BkState {         // per-instance device arrays, instance-major; their shapes are kBkArrays below
  int B, N;
  double *p, *yc, *yd, *zl, *zu, *D, *r, *Dinv, *Tk, *v, *Jd, *dcur, *dp, *scal, *filt;
};

// The one statement of BkState's shapes (StateArray, rl_dtrack.hpp), in the order the host carves them.
constexpr StateArray<BkState> kBkArrays[] = {
    {&BkState::p, kBkNb, 0},       // [B,N,10] unknowns w (8, scaled) and the slacks of the lateral and traction rows
    {&BkState::yc, kBkNe, 0},      // [B,N,6]  multipliers of the equalities
    {&BkState::yd, kBkNd, 0},      // [B,N,2]  multipliers of (inequality function - slack) = 0
    {&BkState::zl, kBkNb, 0},      // [B,N,10] bound multipliers (0 where the bound is infinite)
    {&BkState::zu, kBkNb, 0},      // [B,N,10]
    {&BkState::D, kBkKK, 0},       // [B,N,196] node KKT blocks before regularisation
    {&BkState::r, kBkK, 0},        // [B,N,14]  gradient of the Lagrangian w/o bounds (8) and equality values (6), then the Newton rhs
    {&BkState::Dinv, kBkKK, 0},    // [B,N,196] inverses of the pivot blocks
    {&BkState::Tk, kBkKK, 0},      // [B,N,196] border multipliers (block of the last node times Dinv)
    {&BkState::v, kBkK, 0},        // [B,N,14]  forward-solve values, then the Newton step (dw, dyc)
    {&BkState::Jd, kBkJd, 0},      // [B,N,16]  Jacobian of the two inequality functions
    {&BkState::dcur, kBkNd, 0},    // [B,N,2]   the inequality functions at the current point
    {&BkState::dp, kBkNb, 0},      // [B,N,10]  primal step (unknowns and slacks)
    {&BkState::scal, 0, kBkScal},  // [B,16]    (BS_* above)
    {&BkState::filt, 0, kBkFilter * 2},   // [B,kBkFilter,2]
};
static_assert(sizeof(kBkArrays) / sizeof(kBkArrays[0]) == (sizeof(BkState) - offsetof(BkState, p)) / sizeof(double*), "every array of BkState has its row");

__device__ __forceinline__ double bk_tan(double x) { return tan(x); }
template <int ND, typename T>
__device__ __forceinline__ Dual<ND, T> bk_tan(const Dual<ND, T>& x) {
  const T t = bk_tan(x.v);
  return chain(x, t, 1.0 + t * t);
}

// d/dt (x, y, theta, delta, v) of models/dynamic_bicycle.py:4-23; beta = atan2(lr delta, L) = atan(lr delta / L), L > 0
template <typename M, typename S>
__device__ __forceinline__ void bk_dyn(M m, const S& th, const S& de, const S& v, S (&f)[3]) {
  const S beta = m_atan(de * (m[BK_LR] / m[BK_L]));
  S sb, cb, st, ct;
  m_sincos(beta, sb, cb);
  m_sincos(th + beta, st, ct);
  f[0] = v * ct; f[1] = v * st;
  f[2] = v * cb * bk_tan(de) / m[BK_L];
}

// the curved part of a node: q = scaled (theta, delta, v, a, delta_dot, T) -> RK4 increments of the 5 states and the
// traction function lat^2 + lon^2 (lat = omega |(vx, vy)|, lon = a)
template <typename M, typename S>
__device__ __forceinline__ void bk_curved(M m, const S (&q)[6], S (&inc)[5], S& trac) {
  const S th = q[0] * kBkSx[2], de = q[1] * kBkSx[3], v = q[2] * kBkSx[4];
  const S a = q[3] * kBkSu[0], dd = q[4] * kBkSu[1], dt = q[5];
  S k1[3], k2[3], k3[3], k4[3];
  bk_dyn(m, th, de, v, k1);
  const S h = dt * 0.5;
  bk_dyn(m, th + h * k1[2], de + h * dd, v + h * a, k2);
  bk_dyn(m, th + h * k2[2], de + h * dd, v + h * a, k3);
  bk_dyn(m, th + dt * k3[2], de + dt * dd, v + dt * a, k4);
  const S w6 = dt * (1.0 / 6.0);
  for (int i = 0; i < 3; ++i) inc[i] = w6 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
  inc[3] = w6 * (dd + 2.0 * dd + 2.0 * dd + dd);
  inc[4] = w6 * (a + 2.0 * a + 2.0 * a + a);
  trac = k1[2] * k1[2] * (k1[0] * k1[0] + k1[1] * k1[1]) + a * a;
}

template <typename PT>
__device__ __forceinline__ void bk_bounds(const PT& P, int b, int j, double (&lo)[kBkNb], double (&hi)[kBkNb]) {
  const auto m = P.m;
  const double inf = __builtin_huge_val();
  const size_t o = P.per ? (size_t)b * P.N + j : (size_t)j;
  lo[0] = lo[1] = lo[2] = -inf; hi[0] = hi[1] = hi[2] = inf;
  lo[3] = -m[BK_DELTA_MAX] / kBkSx[3]; hi[3] = m[BK_DELTA_MAX] / kBkSx[3];
  lo[4] = 0.0; hi[4] = m[BK_V_MAX] / kBkSx[4];
  lo[5] = m[BK_A_LON_MIN] / kBkSu[0]; hi[5] = m[BK_A_LON_MAX] / kBkSu[0];
  lo[6] = -m[BK_DELTA_DOT_MAX] / kBkSu[1]; hi[6] = m[BK_DELTA_DOT_MAX] / kBkSu[1];
  lo[7] = 0.0; hi[7] = inf;
  lo[8] = P.dr[o]; hi[8] = P.dl[o];
  lo[9] = -inf; hi[9] = m[BK_ACC_MAX] * m[BK_ACC_MAX];
}

// values of node j's functions: c [6] (defect 5, longitudinal coordinate), d [2] (lateral coordinate, traction)
template <typename PT>
__device__ __forceinline__ void bk_values(const PT& P, int j, const double* w, const double* wn, double (&c)[kBkNe],
                                          double (&d)[2]) {
  const int jn = j + 1 == P.N ? 0 : j + 1;
  double q[6] = {w[2], w[3], w[4], w[5], w[6], w[7]}, inc[5], trac;
  bk_curved(P.m, q, inc, trac);
  double sy, cy;
  sincos(P.yaw[j], &sy, &cy);
  const double px = w[0] * kBkSx[0], py = w[1] * kBkSx[1];
  const double x1[5] = {px + P.P0[2 * j], py + P.P0[2 * j + 1], w[2] * kBkSx[2], w[3] * kBkSx[3], w[4] * kBkSx[4]};
  double x2[5] = {wn[0] * kBkSx[0] + P.P0[2 * jn], wn[1] * kBkSx[1] + P.P0[2 * jn + 1], wn[2] * kBkSx[2], wn[3] * kBkSx[3],
                  wn[4] * kBkSx[4]};
  const double dth = x2[2] - x1[2];
  x2[2] = atan2(sin(dth), cos(dth)) + x1[2];   // utils/utils.py:10-13
  for (int i = 0; i < 5; ++i) c[i] = x1[i] + inc[i] - x2[i];
  c[5] = cy * px + sy * py;
  d[0] = -sy * px + cy * py;
  d[1] = trac;
}

// ---- block reductions over the workgroup (op 0 sum, 1 max, 2 min)
template <int NV>
__device__ __forceinline__ void bk_reduce(double (&v)[NV], const int (&op)[NV], double* red /* [NV * kBkThreads / 64] */) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < NV; ++k) {
    double x = v[k];
    for (int o = 32; o > 0; o >>= 1) {
      const double y = __shfl_xor(x, o);
      x = op[k] == 0 ? x + y : (op[k] == 1 ? fmax(x, y) : fmin(x, y));
    }
    if (lane == 0) red[k * (kBkThreads / 64) + wv] = x;
  }
  __syncthreads();
  for (int k = 0; k < NV; ++k) {
    double x = red[k * (kBkThreads / 64)];
    for (int i = 1; i < kBkThreads / 64; ++i) {
      const double y = red[k * (kBkThreads / 64) + i];
      x = op[k] == 0 ? x + y : (op[k] == 1 ? fmax(x, y) : fmin(x, y));
    }
    v[k] = x;
  }
  __syncthreads();
}

// IPOPT's bound push (bound_push = bound_frac = 1e-2)
__device__ __forceinline__ double bk_push(double p, double lo, double hi) {
  const bool fl = isfinite(lo), fh = isfinite(hi);
  double wl = fl ? 1e-2 * fmax(1.0, fabs(lo)) : 0.0, wh = fh ? 1e-2 * fmax(1.0, fabs(hi)) : 0.0;
  if (fl && fh) { wl = fmin(wl, 1e-2 * (hi - lo)); wh = fmin(wh, 1e-2 * (hi - lo)); }
  if (fl) p = fmax(p, lo + wl);
  if (fh) p = fmin(p, hi - wh);
  return p;
}

// physical X [B,N,5], U [B,N,2], T [B,N] -> scaled unknowns, pushed inside their bounds; slacks; multipliers; scalars
template <typename PT>
__global__ void __launch_bounds__(kBkThreads) k_bk_init(PT P, BkState st, const double* X, const double* U,
                                                        const double* T) {
  const int b = blockIdx.x, N = P.N;
  bk_instance(P, b);
  for (int j = threadIdx.x; j < N; j += kBkThreads) {
    const size_t n = (size_t)b * N + j;
    double lo[kBkNb], hi[kBkNb];
    bk_bounds(P, b, j, lo, hi);
    double* w = st.p + n * kBkNb;
    w[0] = (X[n * 5 + 0] - P.P0[2 * j]) / kBkSx[0];
    w[1] = (X[n * 5 + 1] - P.P0[2 * j + 1]) / kBkSx[1];
    for (int i = 2; i < 5; ++i) w[i] = X[n * 5 + i] / kBkSx[i];
    w[5] = U[n * 2] / kBkSu[0]; w[6] = U[n * 2 + 1] / kBkSu[1]; w[7] = T[n];
    for (int i = 0; i < kBkNv; ++i) w[i] = bk_push(w[i], lo[i], hi[i]);
    for (int i = 0; i < kBkNe; ++i) st.yc[n * kBkNe + i] = 0.0;
    st.yd[n * 2] = st.yd[n * 2 + 1] = 0.0;
  }
  __syncthreads();   // bk_values reads the neighbour's unknowns
  for (int j = threadIdx.x; j < N; j += kBkThreads) {
    const size_t n = (size_t)b * N + j;
    double lo[kBkNb], hi[kBkNb], c[kBkNe], d[2];
    bk_bounds(P, b, j, lo, hi);
    double* w = st.p + n * kBkNb;
    const int jn = j + 1 == N ? 0 : j + 1;
    bk_values(P, j, w, st.p + ((size_t)b * N + jn) * kBkNb, c, d);
    w[8] = bk_push(d[0], lo[8], hi[8]);
    w[9] = bk_push(d[1], lo[9], hi[9]);
    for (int i = 0; i < kBkNb; ++i) {
      st.zl[n * kBkNb + i] = isfinite(lo[i]) ? 1.0 : 0.0;
      st.zu[n * kBkNb + i] = isfinite(hi[i]) ? 1.0 : 0.0;
    }
  }
  if (threadIdx.x < kBkScal) {
    double* s = st.scal + (size_t)b * kBkScal;
    s[threadIdx.x] = threadIdx.x == BS_MU ? kBkMu0 : (threadIdx.x == BS_THMAX ? -1.0 : 0.0);
  }
}

// node j: functions, Jacobians and Hessian of the Lagrangian into D (H in the unknowns' block, Jc and Jc^T), the
// gradient of the Lagrangian without bound terms into r[0:8], c into r[8:14]; Jd, d.  Returns the error contributions.
template <typename PT>
__device__ __forceinline__ void bk_node_derivs(const PT& P, const BkState& st, int b, int j, double& dual, double& prim,
                                               double& gzmax, double& gzmin, double& comp0, double& lap) {
  const int N = P.N, jn = j + 1 == N ? 0 : j + 1, jp = j == 0 ? N - 1 : j - 1;
  const size_t n = (size_t)b * N + j;
  const double* w = st.p + n * kBkNb;
  const double* yc = st.yc + n * kBkNe;
  const double* yd = st.yd + n * 2;
  double c[kBkNe], d[2];
  bk_values(P, j, w, st.p + ((size_t)b * N + jn) * kBkNb, c, d);
  double sy, cy;
  sincos(P.yaw[j], &sy, &cy);
  double Jc[kBkNe][kBkNv] = {}, Jd[2][kBkNv] = {};
  {   // first derivatives of the curved part
    using D1 = Dual<6, double>;
    D1 q[6], inc[5], trac;
    for (int k = 0; k < 6; ++k) { q[k].v = w[2 + k]; for (int t = 0; t < 6; ++t) q[k].d[t] = t == k ? 1.0 : 0.0; }
    bk_curved(P.m, q, inc, trac);
    for (int i = 0; i < 5; ++i) for (int t = 0; t < 6; ++t) Jc[i][2 + t] = inc[i].d[t];
    for (int t = 0; t < 6; ++t) Jd[1][2 + t] = trac.d[t];
  }
  for (int i = 0; i < 5; ++i) Jc[i][i] += kBkSx[i];
  Jc[5][0] = cy * kBkSx[0]; Jc[5][1] = sy * kBkSx[1];
  Jd[0][0] = -sy * kBkSx[0]; Jd[0][1] = cy * kBkSx[1];
  double* Dn = st.D + n * kBkKK;
  for (int i = 0; i < kBkKK; ++i) Dn[i] = 0.0;
  for (int t = 0; t < 6; ++t) {   // row t of the Hessian of yc . inc + yd[1] trac (the other rows are linear)
    using D1 = Dual<6, double>;
    using D2 = Dual<1, D1>;
    D2 q[6], inc[5], trac;
    for (int k = 0; k < 6; ++k) {
      q[k].v.v = w[2 + k];
      for (int u = 0; u < 6; ++u) q[k].v.d[u] = u == k ? 1.0 : 0.0;
      q[k].d[0].v = k == t ? 1.0 : 0.0;
      for (int u = 0; u < 6; ++u) q[k].d[0].d[u] = 0.0;
    }
    bk_curved(P.m, q, inc, trac);
    for (int u = 0; u < 6; ++u) {
      double h = yd[1] * trac.d[0].d[u];
      for (int i = 0; i < 5; ++i) h += yc[i] * inc[i].d[0].d[u];
      Dn[(2 + t) * kBkK + 2 + u] = h;
    }
  }
  for (int i = 0; i < kBkNe; ++i)
    for (int k = 0; k < kBkNv; ++k) { Dn[(kBkNv + i) * kBkK + k] = Jc[i][k]; Dn[k * kBkK + kBkNv + i] = Jc[i][k]; }
  // gradient of the Lagrangian (cost, equalities incl. the coupling of pair j-1, inequality rows)
  const double* ycp = st.yc + ((size_t)b * N + jp) * kBkNe;
  double* rn = st.r + n * kBkK;
  const double* zl = st.zl + n * kBkNb;
  const double* zu = st.zu + n * kBkNb;
  double lo[kBkNb], hi[kBkNb];
  bk_bounds(P, b, j, lo, hi);
  for (int k = 0; k < kBkNv; ++k) {
    double g = k == 7 ? 1.0 : 0.0;
    for (int i = 0; i < kBkNe; ++i) g += Jc[i][k] * yc[i];
    if (k < 5) g -= kBkSx[k] * ycp[k];
    rn[k] = g;
    const double gl = g + Jd[0][k] * yd[0] + Jd[1][k] * yd[1] - zl[k] + zu[k];
    dual = fmax(dual, fabs(gl));
  }
  for (int i = 0; i < 2; ++i) dual = fmax(dual, fabs(-yd[i] - zl[kBkNv + i] + zu[kBkNv + i]));
  for (int i = 0; i < kBkNe; ++i) { rn[kBkNv + i] = c[i]; prim = fmax(prim, fabs(c[i])); }
  for (int i = 0; i < 2; ++i) prim = fmax(prim, fabs(d[i] - w[kBkNv + i]));
  for (int i = 0; i < kBkNb; ++i) {
    if (isfinite(lo[i])) { const double gz = (w[i] - lo[i]) * zl[i]; gzmax = fmax(gzmax, gz); gzmin = fmin(gzmin, gz); comp0 = fmax(comp0, fabs(gz)); }
    if (isfinite(hi[i])) { const double gz = (hi[i] - w[i]) * zu[i]; gzmax = fmax(gzmax, gz); gzmin = fmin(gzmin, gz); comp0 = fmax(comp0, fabs(gz)); }
  }
  for (int k = 0; k < kBkNv; ++k) { st.Jd[n * kBkJd + k] = Jd[0][k]; st.Jd[n * kBkJd + 8 + k] = Jd[1][k]; }
  st.dcur[n * 2] = d[0]; st.dcur[n * 2 + 1] = d[1];
  lap += w[7];
}

// theta (sum |c| + |d - s|) and phi (sum T - mu sum log gaps) at p + a dp
template <typename PT>
__device__ __forceinline__ void bk_trial(const PT& P, const BkState& st, const double* dp, int b, double a, double mu,
                                         double& th, double& ph) {
  const int N = P.N;
  th = 0.0; ph = 0.0;
  for (int j = threadIdx.x; j < N; j += kBkThreads) {
    const int jn = j + 1 == N ? 0 : j + 1;
    const size_t n = (size_t)b * N + j, nn = (size_t)b * N + jn;
    double w[kBkNb], wn[kBkNv], c[kBkNe], d[2], lo[kBkNb], hi[kBkNb];
    for (int i = 0; i < kBkNb; ++i) w[i] = st.p[n * kBkNb + i] + a * dp[n * kBkNb + i];
    for (int i = 0; i < kBkNv; ++i) wn[i] = st.p[nn * kBkNb + i] + a * dp[nn * kBkNb + i];
    bk_values(P, j, w, wn, c, d);
    bk_bounds(P, b, j, lo, hi);
    for (int i = 0; i < kBkNe; ++i) th += fabs(c[i]);
    th += fabs(d[0] - w[8]) + fabs(d[1] - w[9]);
    double lg = 0.0;
    for (int i = 0; i < kBkNb; ++i) {
      if (isfinite(lo[i])) lg += log(w[i] - lo[i]);
      if (isfinite(hi[i])) lg += log(hi[i] - w[i]);
    }
    ph += w[7] - mu * lg;
  }
}

// Gauss-Jordan inversion in place of the 14 x 14 block M (LDS), one entry per thread t < 196; the pivots are those of
// an LDL^T factorisation without pivoting, so their signs give the block's inertia.  Thread 0 counts.
// A pivot that is zero up to cancellation (|pivot| <= kBkPivRel |its diagonal entry before the elimination|) counts as
// a wrong inertia: e.g. y after x when only the rank-1 lateral row acts on them, whose pivot is rounding noise.
__device__ __forceinline__ void bk_invert(double* M, double* diag0, int t, int& neg, bool& bad) {
  const int i = t / kBkK, jj = t % kBkK;
  if (t < kBkK) diag0[t] = fabs(M[t * kBkK + t]);
  __syncthreads();
  for (int p = 0; p < kBkK; ++p) {
    double nv = 0.0;
    const double piv = M[p * kBkK + p];
    if (t < kBkKK) {
      const double aip = M[i * kBkK + p], apj = M[p * kBkK + jj], aij = M[t];
      const double ip = 1.0 / piv;
      nv = (i == p && jj == p) ? ip : (i == p ? apj * ip : (jj == p ? -aip * ip : aij - aip * apj * ip));
    }
    if (t == 0) {
      if (piv < 0.0) ++neg;
      if (!(fabs(piv) > kBkPivRel * diag0[p]) || !isfinite(piv)) bad = true;
    }
    __syncthreads();
    if (t < kBkKK) M[t] = nv;
    __syncthreads();
  }
}

// one interior-point iteration per instance; final != 0: only the convergence test and the statistics
template <typename PT>
__global__ void __launch_bounds__(kBkThreads) k_bk_iter(PT P, BkState st, int final_pass) {
  const int b = blockIdx.x, N = P.N, t = threadIdx.x;
  bk_instance(P, b);
  double* sc = st.scal + (size_t)b * kBkScal;
  if (sc[BS_DONE] != 0.0) return;
  __shared__ double red[8 * (kBkThreads / 64)];
  __shared__ double M[kBkKK], Bt[kBkKK], Last[kBkKK], Tm[kBkKK];
  __shared__ double vec[5][kBkK];
  __shared__ double diag0[kBkK];
  __shared__ int ibc[2];
  double mu = sc[BS_MU];
  // ---- 1. derivatives, errors
  {
    double e[6] = {0.0, 0.0, -1e300, 1e300, 0.0, 0.0};   // dual, prim, gz max, gz min, comp0, lap
    for (int j = t; j < N; j += kBkThreads) bk_node_derivs(P, st, b, j, e[0], e[1], e[2], e[3], e[4], e[5]);
    const int op[6] = {1, 1, 1, 2, 1, 0};
    bk_reduce(e, op, red);
    const double tol = P.tol;
    const bool conv = fmax(e[0], fmax(e[1], e[4])) <= tol;
    if (conv || final_pass) {
      if (t == 0) {
        sc[BS_DUAL] = e[0]; sc[BS_PRIM] = e[1]; sc[BS_COMP] = e[4]; sc[BS_LAP] = e[5];
        sc[BS_STATUS] = conv ? 1.0 : 0.0; sc[BS_DONE] = 1.0;
      }
      return;
    }
    // barrier update (IPOPT's monotone rule), filter reset
    bool changed = false;
    while (mu > tol / 10.0 && fmax(fmax(e[0], e[1]), fmax(e[2] - mu, mu - e[3])) <= kBkKappaEps * mu) {
      mu = fmax(tol / 10.0, fmin(kBkKappaMu * mu, pow(mu, kBkThetaMu)));
      changed = true;
    }
    if (t == 0) { sc[BS_MU] = mu; if (changed) sc[BS_NFILT] = 0.0; }
  }
  // ---- 2. condensed node blocks and right-hand sides
  for (int j = t; j < N; j += kBkThreads) {
    const size_t n = (size_t)b * N + j;
    const double* w = st.p + n * kBkNb;
    const double* zl = st.zl + n * kBkNb;
    const double* zu = st.zu + n * kBkNb;
    const double* Jd = st.Jd + n * kBkJd;
    double lo[kBkNb], hi[kBkNb], sig[kBkNb], bar[kBkNb];
    bk_bounds(P, b, j, lo, hi);
    for (int i = 0; i < kBkNb; ++i) {
      sig[i] = 0.0; bar[i] = 0.0;
      if (isfinite(lo[i])) { const double g = w[i] - lo[i]; sig[i] += zl[i] / g; bar[i] -= mu / g; }
      if (isfinite(hi[i])) { const double g = hi[i] - w[i]; sig[i] += zu[i] / g; bar[i] += mu / g; }
    }
    double rs[2];
    for (int i = 0; i < 2; ++i) rs[i] = sig[kBkNv + i] * (st.dcur[n * 2 + i] - w[kBkNv + i]) + bar[kBkNv + i];
    double* Dn = st.D + n * kBkKK;
    double* rn = st.r + n * kBkK;
    for (int k = 0; k < kBkNv; ++k) {
      Dn[k * kBkK + k] += sig[k];
      for (int l = 0; l < kBkNv; ++l) Dn[k * kBkK + l] += Jd[k] * sig[8] * Jd[l] + Jd[8 + k] * sig[9] * Jd[8 + l];
      rn[k] = -(rn[k] + bar[k] + Jd[k] * rs[0] + Jd[8 + k] * rs[1]);
    }
    for (int i = 0; i < kBkNe; ++i) rn[kBkNv + i] = -rn[kBkNv + i];
  }
  __syncthreads();
  // ---- 3. elimination with inertia correction
  const int ei = t / kBkK, ej = t % kBkK;
  const double* Db = st.D + (size_t)b * N * kBkKK;
  double* Dinv = st.Dinv + (size_t)b * N * kBkKK;
  double* Tk = st.Tk + (size_t)b * N * kBkKK;
  double dw = 0.0, dw_last = sc[BS_DW];
  int tries = 0;
  bool failed = false;
  for (;;) {
    const double reg = (ei == ej) ? (ei < kBkNv ? dw : -kBkDeltaC) : 0.0;
    int neg = 0;
    bool bad = false;
    if (t < kBkKK) {
      Last[t] = Db[(size_t)(N - 1) * kBkKK + t] + reg;
      Bt[t] = (ei >= kBkNv && ej < 5 && ei - kBkNv == ej) ? -kBkSx[ej] : 0.0;   // K[N-1, 0] = E_{N-1}^T
      M[t] = Db[t] + reg;
    }
    __syncthreads();
    for (int k = 0; k < N - 1; ++k) {
      const double pre = (t < kBkKK && k + 1 < N - 1) ? Db[(size_t)(k + 1) * kBkKK + t] : 0.0;   // in flight during the inversion
      bk_invert(M, diag0, t, neg, bad);
      double tv = 0.0;
      if (t < kBkKK) {
        Dinv[(size_t)k * kBkKK + t] = M[t];
        for (int m = 0; m < kBkK; ++m) tv += Bt[ei * kBkK + m] * M[m * kBkK + ej];
        Tm[t] = tv;
      }
      __syncthreads();
      double nm = 0.0, nb = 0.0;
      if (t < kBkKK) {
        Tk[(size_t)k * kBkKK + t] = tv;
        double s = 0.0;
        for (int m = 0; m < kBkK; ++m) s += Tm[ei * kBkK + m] * Bt[ej * kBkK + m];
        Last[t] -= s;
        if (k + 1 < N - 1) {
          nm = pre + reg;
          if (ei < 5 && ej < 5) nm -= kBkSx[ei] * kBkSx[ej] * M[(kBkNv + ei) * kBkK + kBkNv + ej];
          nb = ej < 5 ? Tm[ei * kBkK + kBkNv + ej] * kBkSx[ej] : 0.0;
          if (k + 1 == N - 2 && ei < 5 && ej == kBkNv + ei) nb -= kBkSx[ei];   // K[N-1, N-2] = E_{N-2}
        }
      }
      __syncthreads();
      if (t < kBkKK && k + 1 < N - 1) { M[t] = nm; Bt[t] = nb; }
      __syncthreads();
    }
    bk_invert(Last, diag0, t, neg, bad);
    if (t < kBkKK) Dinv[(size_t)(N - 1) * kBkKK + t] = Last[t];
    if (t == 0) { ibc[0] = neg; ibc[1] = bad ? 1 : 0; }
    __syncthreads();
    const int negc = ibc[0];
    const bool badc = ibc[1] != 0;
    __syncthreads();
    ++tries;
    if (!badc && negc == kBkNe * N) break;
    if (dw == 0.0) dw = dw_last == 0.0 ? kBkDw0 : fmax(1e-20, kBkDwDown * dw_last);
    else dw *= dw_last == 0.0 ? kBkDwFirstUp : kBkDwUp;
    if (dw > kBkDwMax) { failed = true; break; }
  }
  if (failed) {
    if (t == 0) { sc[BS_STATUS] = 2.0; sc[BS_DONE] = 1.0; }
    return;
  }
  if (t == 0) { sc[BS_REFAC] += tries - 1; if (dw > 0.0) sc[BS_DW] = dw; }
  // ---- 4. forward and backward substitution
  const double* rb = st.r + (size_t)b * N * kBkK;
  double* vb = st.v + (size_t)b * N * kBkK;
  double* rcur = vec[0];
  double* rlast = vec[1];
  double* zlast = vec[2];
  double* znext = vec[3];
  double* vk = vec[4];
  if (t < kBkK) { rlast[t] = rb[(size_t)(N - 1) * kBkK + t]; rcur[t] = rb[t]; }
  __syncthreads();
  for (int k = 0; k < N - 1; ++k) {
    double x = 0.0;
    if (t < kBkK) {
      for (int m = 0; m < kBkK; ++m) x += Dinv[(size_t)k * kBkKK + t * kBkK + m] * rcur[m];
      vb[(size_t)k * kBkK + t] = x;
    } else if (t >= 64 && t < 64 + kBkK) {
      const int i = t - 64;
      for (int m = 0; m < kBkK; ++m) x += Tk[(size_t)k * kBkKK + i * kBkK + m] * rcur[m];
    }
    if (t < kBkK) vk[t] = x;
    __syncthreads();
    if (t >= 64 && t < 64 + kBkK) rlast[t - 64] -= x;
    if (t < kBkK && k + 1 < N - 1) rcur[t] = rb[(size_t)(k + 1) * kBkK + t] + (t < 5 ? kBkSx[t] * vk[kBkNv + t] : 0.0);
    __syncthreads();
  }
  if (t < kBkK) {
    double x = 0.0;
    for (int m = 0; m < kBkK; ++m) x += Dinv[(size_t)(N - 1) * kBkKK + t * kBkK + m] * rlast[m];
    zlast[t] = x; znext[t] = x;
    vb[(size_t)(N - 1) * kBkK + t] = x;
  }
  __syncthreads();
  for (int k = N - 2; k >= 0; --k) {
    double x = 0.0;
    if (t < kBkK) {
      x = vb[(size_t)k * kBkK + t];
      for (int m = 0; m < kBkK; ++m) x -= Tk[(size_t)k * kBkKK + m * kBkK + t] * zlast[m];
      if (k + 1 < N - 1)
        for (int c = 0; c < 5; ++c) x += Dinv[(size_t)k * kBkKK + t * kBkK + kBkNv + c] * kBkSx[c] * znext[c];
    }
    __syncthreads();
    if (t < kBkK) { znext[t] = x; vb[(size_t)k * kBkK + t] = x; }
    __syncthreads();
  }
  // ---- 5. steps of slacks and multipliers, fraction to the boundary, theta / phi at the current point
  double* dpb = st.dp;
  const double tau = fmax(kBkTauMin, 1.0 - mu);
  double e[5] = {1.0, 1.0, 0.0, 0.0, 0.0};   // alpha_max, alpha_z, grad phi . dp, theta0, phi0
  for (int j = t; j < N; j += kBkThreads) {
    const size_t n = (size_t)b * N + j;
    const double* w = st.p + n * kBkNb;
    const double* zl = st.zl + n * kBkNb;
    const double* zu = st.zu + n * kBkNb;
    const double* Jd = st.Jd + n * kBkJd;
    const double* sol = vb + (size_t)j * kBkK;
    double lo[kBkNb], hi[kBkNb], dp[kBkNb];
    bk_bounds(P, b, j, lo, hi);
    for (int i = 0; i < kBkNv; ++i) dp[i] = sol[i];
    for (int i = 0; i < 2; ++i) {
      double s = st.dcur[n * 2 + i] - w[kBkNv + i];
      for (int k = 0; k < kBkNv; ++k) s += Jd[8 * i + k] * dp[k];
      dp[kBkNv + i] = s;
    }
    for (int i = 0; i < kBkNb; ++i) {
      dpb[n * kBkNb + i] = dp[i];
      if (isfinite(lo[i])) {
        const double g = w[i] - lo[i];
        const double dz = mu / g - zl[i] - zl[i] / g * dp[i];
        if (dp[i] < 0.0) e[0] = fmin(e[0], -tau * g / dp[i]);
        if (dz < 0.0) e[1] = fmin(e[1], -tau * zl[i] / dz);
        e[2] += -mu / g * dp[i];
      }
      if (isfinite(hi[i])) {
        const double g = hi[i] - w[i];
        const double dz = mu / g - zu[i] + zu[i] / g * dp[i];
        if (dp[i] > 0.0) e[0] = fmin(e[0], tau * g / dp[i]);
        if (dz < 0.0) e[1] = fmin(e[1], -tau * zu[i] / dz);
        e[2] += mu / g * dp[i];
      }
    }
    e[2] += dp[7];
  }
  __syncthreads();   // the steps of the neighbours
  {
    bk_trial(P, st, dpb, b, 0.0, mu, e[3], e[4]);   // theta and phi at the current point
    const int op[5] = {2, 2, 0, 0, 0};
    bk_reduce(e, op, red);
  }
  const double amax = e[0], az = e[1], gphi = e[2], th0 = e[3], ph0 = e[4];
  double thmax = sc[BS_THMAX], thmin = sc[BS_THMIN];
  if (thmax < 0.0) { thmax = 1e4 * fmax(1.0, th0); thmin = 1e-4 * fmax(1.0, th0); }
  // ---- 6. filter line search
  const double* filt = st.filt + (size_t)b * kBkFilter * 2;
  const int nfilt = (int)sc[BS_NFILT];
  double a = amax;
  bool accepted = false, ftype = false;
  int halv = 0;
  for (halv = 0; halv < kBkMaxHalvings; ++halv) {
    double v2[2];
    bk_trial(P, st, dpb, b, a, mu, v2[0], v2[1]);
    const int op[2] = {0, 0};
    bk_reduce(v2, op, red);
    const double tht = v2[0], pht = v2[1];
    bool ok = tht <= thmax;
    for (int f = 0; f < nfilt && ok; ++f)
      if (tht >= filt[2 * f] && pht >= filt[2 * f + 1]) ok = false;
    ftype = false;
    if (ok) {
      if (gphi < 0.0 && a * pow(-gphi, kBkSPhi) > pow(th0, kBkSTh) && th0 <= thmin) {
        ftype = true;
        ok = pht <= ph0 + kBkEta * a * gphi;
      } else {
        ok = tht <= (1.0 - kBkGammaTh) * th0 || pht <= ph0 - kBkGammaPhi * th0;
      }
    }
    if (ok) { accepted = true; break; }
    if (halv < kBkMaxHalvings - 1) a *= 0.5;
  }
  if (halv == kBkMaxHalvings) halv = kBkMaxHalvings - 1;
  if (t == 0) {
    if (!ftype || !accepted) {
      const int f = nfilt < kBkFilter ? nfilt : kBkFilter - 1;
      double* fw = st.filt + (size_t)b * kBkFilter * 2;
      fw[2 * f] = (1.0 - kBkGammaTh) * th0; fw[2 * f + 1] = ph0 - kBkGammaPhi * th0;
      sc[BS_NFILT] = (double)(f + 1);
    }
    sc[BS_THMAX] = thmax; sc[BS_THMIN] = thmin;
    sc[BS_ALPHA] = a; sc[BS_AMAX] = amax; sc[BS_HALV] = halv;
    sc[BS_IT] += 1.0;
  }
  // ---- 7. update (multiplier steps from the old point, then the primal step)
  for (int j = t; j < N; j += kBkThreads) {
    const size_t n = (size_t)b * N + j;
    double* w = st.p + n * kBkNb;
    double* zl = st.zl + n * kBkNb;
    double* zu = st.zu + n * kBkNb;
    const double* sol = vb + (size_t)j * kBkK;
    double lo[kBkNb], hi[kBkNb];
    bk_bounds(P, b, j, lo, hi);
    for (int i = 0; i < kBkNe; ++i) st.yc[n * kBkNe + i] += a * sol[kBkNv + i];
    double sig[2], bar[2];
    for (int i = 0; i < 2; ++i) {
      const int q = kBkNv + i;
      sig[i] = 0.0; bar[i] = 0.0;
      if (isfinite(lo[q])) { const double g = w[q] - lo[q]; sig[i] += zl[q] / g; bar[i] -= mu / g; }
      if (isfinite(hi[q])) { const double g = hi[q] - w[q]; sig[i] += zu[q] / g; bar[i] += mu / g; }
      const double dyd = sig[i] * dpb[n * kBkNb + q] - st.yd[n * 2 + i] + bar[i];
      st.yd[n * 2 + i] += a * dyd;
    }
    for (int i = 0; i < kBkNb; ++i) {
      const double dp = dpb[n * kBkNb + i];
      double dzl = 0.0, dzu = 0.0;
      if (isfinite(lo[i])) { const double g = w[i] - lo[i]; dzl = mu / g - zl[i] - zl[i] / g * dp; }
      if (isfinite(hi[i])) { const double g = hi[i] - w[i]; dzu = mu / g - zu[i] + zu[i] / g * dp; }
      w[i] += a * dp;
      if (isfinite(lo[i])) {
        const double g = w[i] - lo[i];
        zl[i] = fmin(fmax(zl[i] + az * dzl, mu / (kBkKappaSigma * g)), kBkKappaSigma * mu / g);
      }
      if (isfinite(hi[i])) {
        const double g = hi[i] - w[i];
        zu[i] = fmin(fmax(zu[i] + az * dzu, mu / (kBkKappaSigma * g)), kBkKappaSigma * mu / g);
      }
    }
  }
}

template <typename PT>
__global__ void k_bk_unpack(PT P, BkState st, double* X, double* U, double* T, double* stats) {
  const int b = blockIdx.y, N = P.N;
  bk_instance(P, b);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < N) {
    const size_t n = (size_t)b * N + j;
    const double* w = st.p + n * kBkNb;
    X[n * 5 + 0] = w[0] * kBkSx[0] + P.P0[2 * j];
    X[n * 5 + 1] = w[1] * kBkSx[1] + P.P0[2 * j + 1];
    for (int i = 2; i < 5; ++i) X[n * 5 + i] = w[i] * kBkSx[i];
    U[n * 2] = w[5] * kBkSu[0]; U[n * 2 + 1] = w[6] * kBkSu[1]; T[n] = w[7];
  }
  if (blockIdx.x == 0 && threadIdx.x < kBkStats) stats[(size_t)b * kBkStats + threadIdx.x] = st.scal[(size_t)b * kBkScal + threadIdx.x];
}

// functions at a given physical point, one thread per (instance, node): eq [B,N,6], ineq [B,N,2] (lateral coordinate,
// lat^2 + lon^2), cost part T
template <typename PT>
__global__ void k_bk_eval(PT P, int B, const double* X, const double* U, const double* T, double* eq, double* ineq) {
  const int b = blockIdx.y, N = P.N;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N || b >= B) return;
  bk_instance(P, b);
  const int jn = j + 1 == N ? 0 : j + 1;
  const size_t n = (size_t)b * N + j, nn = (size_t)b * N + jn;
  double w[kBkNv], wn[kBkNv];
  auto scale = [&](size_t q, int jj, double* o) {
    o[0] = (X[q * 5 + 0] - P.P0[2 * jj]) / kBkSx[0];
    o[1] = (X[q * 5 + 1] - P.P0[2 * jj + 1]) / kBkSx[1];
    for (int i = 2; i < 5; ++i) o[i] = X[q * 5 + i] / kBkSx[i];
    o[5] = U[q * 2] / kBkSu[0]; o[6] = U[q * 2 + 1] / kBkSu[1]; o[7] = T[q];
  };
  scale(n, j, w); scale(nn, jn, wn);
  double c[kBkNe], d[2];
  bk_values(P, j, w, wn, c, d);
  for (int i = 0; i < kBkNe; ++i) eq[n * kBkNe + i] = c[i];
  ineq[n * 2] = d[0]; ineq[n * 2 + 1] = d[1];
}

}  // namespace rl
