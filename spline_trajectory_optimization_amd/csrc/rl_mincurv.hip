// rl_mincurv.hip -- C ABI (include/rl_mincurv.h) over the HIP kernels in rl_kernels.hpp, rl_sweep.hpp and the headers below.
// Built for gfx950 only:  hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC
//
// There is deliberately no CPU path in this library: every entry point launches HIP kernels and
// fails with RL_ERR_HIP when no device is usable.
#include "rl_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>

#include "rl_kernels.hpp"
#include "rl_sweep.hpp"
#include "rl_qss_df.hpp"
#include "rl_global.hpp"
#include "rl_global2.hpp"
#include "rl_global_xy.hpp"
#include "rl_dtrack.hpp"
#include "rl_mintime.hpp"
#include "rl_bicycle.hpp"
#include "rl_region.hpp"
#include "rl_tables.hpp"
#include "rl_pose_tables.hpp"
#include "rl_spline_fit.hpp"
#include "rl_frenet.hpp"

namespace {
double* g_dbg_buf = nullptr;   // rl_debug_dump_enable: step / window dump of the sweep kernels (tests)
size_t g_dbg_len = 0;
int g_dbg_instances = 0;
}  // namespace

struct rl_track {
  rl_ctx* ctx = nullptr;
  int k = 0, n = 0, nt = 0, N = 0;
  std::vector<double> t_host;
  DevBuf<double> t, c0, D, base;
  DevBuf<int> ell, sup;
  // reference-order mode (RL_ARITH_REFERENCE): unfused de Boor tables and the initial line with its two normal
  // directions, built by the first solve that asks for them, rebuilt when the control points change
  mutable DevBuf<double> Ds, base_s;
  mutable bool strict_valid = false;
  mutable DevBuf<double> aux;   // reference-order sweep, per instance: table control points + per-sample flags (numpy's error state)
  DevBuf<double> ringL, ringR;  // shared rings as (x,y) pairs
  int nL = 0, nR = 0;
  double length = 0.0;          // BSplineTrajectory._length of the INITIAL spline (rl_track_set_length); 0 = not given
  // Device scratch owned by the track (sweep residency variant, global-QP tables): a track is therefore
  // SINGLE-STREAM -- two contexts / streams must not run solves on the same rl_track concurrently
  // (include/rl_mincurv.h, "Threading").
  mutable DevBuf<double> gscratch;  // for the non-LDS-resident sweep variant
  // tables of the global QP (a15), built on first use and dropped when the centre line changes
  mutable DevBuf<double> gq_A, gq_nu;
  mutable DevBuf<int> gq_chunk, gq_span;    // chunks of <= rl::kGRows rows (k_global_qp)
  mutable DevBuf<int> gq2_chunk, gq2_span;  // chunks of <= gq2_rows rows (k_global_qp2), if they fit
  mutable int gq_nc = 0, gq2_nc = 0, gq2_rows = 0;  // gq2_rows = 0: the fast path does not fit
  mutable bool gq_valid = false;
  // tables of the two-coordinate global QP (rl_global_xy.hpp)
  mutable DevBuf<int> gxy_span, gxy_chunk, gxy_sch0;
  mutable int gxy_nch = 0;
  mutable DevBuf<double> gxy_bbx;
  mutable bool gxy_valid = false;
  rl::TrackDev dev() const {
    rl::TrackDev d;
    d.k = k; d.n = n; d.nt = nt; d.N = N;
    d.t = t.p; d.c0 = c0.p; d.ell = ell.p; d.D = D.p; d.sup = sup.p; d.base = base.p;
    d.Ds = Ds.p; d.base_s = base_s.p;
    return d;
  }
};

namespace {

bool degree_supported(int k) { return k == 3 || k == 5; }

// dispatch on the spline degree: f(std::integral_constant<int, K>) for K = 3 or 5 (a generic lambda; RL_DEGREE names its K)
template <typename F>
int by_degree(int k, F&& f) {
  if (k == 3) return f(std::integral_constant<int, 3>{});
  if (k == 5) return f(std::integral_constant<int, 5>{});
  return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
}
#define RL_DEGREE(kc) (std::decay_t<decltype(kc)>::value)

// the same for a run-time flag that selects a template argument: f(std::bool_constant<V>)
template <typename F>
int by_flag(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// Samples [s0, s1) under control points j .. j + span - 1, with the reference's own mask (u >= t[j]) & (u < t[j+span+k]),
// u_i = i * (1/N).  The two loops ARE the mask: the indices are part of the bit-exact contract.
struct SupportRange { int s0, s1; };
SupportRange support_range(const std::vector<double>& t_host, int k, int N, int j, int span = 1) {
  const double step = 1.0 / (double)N;
  const double ts = t_host[j], te = t_host[j + span + k];
  int a = 0;
  while (a < N && !((double)a * step >= ts)) ++a;
  int b = a;
  while (b < N && (double)b * step < te) ++b;
  return {a, b};
}

int check_spline(const double* t, int nt, const double* cx, const double* cy, int k) {
  if (!t || !cx || !cy) return fail(RL_ERR_ARG, "null spline pointer");
  if (!degree_supported(k)) return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
  if (nt < 2 * (k + 1)) return fail(RL_ERR_ARG, "knot vector too short");
  return RL_OK;
}

struct SweepPlan {
  rl::Residency residency;
  size_t lds_bytes;
  size_t gscratch_doubles;  // per instance
  int block;
};

SweepPlan plan_sweep(const rl_ctx* ctx, int n, int N, int nL, int nR, int B, bool joint = false, bool strict = false) {
  using rl::Residency;
  SweepPlan p;
  p.block = rl::kSweepThreads;
  // Residency of the per-instance state (ring vertices 16 B x (nL + nR), crossings 8 B x 2N):
  //   all in LDS      : lowest latency per step, but ~120 KB at N = 2000 -> one workgroup per CU;
  //   all in global   : ~31 KB of LDS -> four workgroups per CU (VGPR-limited), state served by L1/L2;
  //   crossings in LDS, rings in global (RL_FORCE_RESIDENCY=2 only): ~63 KB -> two workgroups per CU, no
  //                     global writes inside the sweep (measured slower than all-global; DESIGN_HISTORY.md section 6).
  // The kernel is FP64-issue / latency bound, so once a batch offers more than ~2 workgroups per
  // CU the occupancy wins (measured: 12.5 ms vs 20.2 ms for 1024 instances, N = 2000).
  // RL_FORCE_GLOBAL_RINGS=0/1 and RL_FORCE_RESIDENCY=0/1/2 override (tests cover the variants).
  const char* force = getenv("RL_FORCE_GLOBAL_RINGS");
  int want = B >= 2 * ctx->num_cu ? 0 : 1;    // 0 all global, 1 all LDS, 2 crossings in LDS
  if (force && (force[0] == '0' || force[0] == '1')) want = force[0] == '1' ? 0 : 1;
  if (const char* r = getenv("RL_FORCE_RESIDENCY")) if (r[0] >= '0' && r[0] <= '2') want = r[0] - '0';
  if (strict && want == 2) want = 0;   // the reference-order mode exists all-LDS and all-global
  rl::SweepLds in = rl::sweep_lds_layout(n, N, nL, nR, Residency::Lds, joint, strict);
  if (want == 1 && in.total * sizeof(double) > (size_t)ctx->max_lds) want = 0;
  if (want == 2) {
    rl::SweepLds mid = rl::sweep_lds_layout(n, N, nL, nR, Residency::CrossingsLds, joint);
    if (mid.total * sizeof(double) > (size_t)ctx->max_lds) want = 0;
  }
  p.residency = want == 1 ? Residency::Lds : want == 2 ? Residency::CrossingsLds : Residency::Global;
  rl::SweepLds L = rl::sweep_lds_layout(n, N, nL, nR, p.residency, joint, strict);
  p.lds_bytes = L.total * sizeof(double);
  // crossings (fast mode: one double per sample and side) or bound points (reference-order mode: two), and behind them the
  // table's X, Y where the sweep keeps them (rl_sweep.hpp: sweep_keeps_table_xy)
  const size_t per_sample_arrays = rl::sweep_keeps_table_xy(joint, strict) ? 3 : 2;
  p.gscratch_doubles = (p.residency != Residency::Global ? 0 : per_sample_arrays * ((N + 1) & ~1) * (strict ? 2 : 1)) +
                       (p.residency == Residency::Lds ? 0 : (size_t)2 * (nL + rl::kRingPad) + (size_t)2 * (nR + rl::kRingPad) +
                                                            rl::sweep_cone_doubles(L.ncL, L.ncR));   // rings, and behind them their windows' cone records
  return p;
}

// One instantiation in the residency the plan chose (all-LDS or all-global; the third residency has a line of its own below).
constexpr bool kRecordSteps = true;   // the DUMP instantiation
template <int K, rl::Driver DRIVER, rl::Arith ARITH, bool DUMP = false>
int launch_sweep_in(const rl_ctx* ctx, const SweepPlan& p, const rl::SweepArgs& a) {
  using rl::Residency; using rl::SweepConfig;
  const dim3 grid(a.B), block(rl::kSweepThreads);
  return p.residency == Residency::Lds
             ? launch(ctx, rl::k_sweep<SweepConfig<K, Residency::Lds, DRIVER, ARITH, DUMP>>, grid, block, p.lds_bytes, a)
             : launch(ctx, rl::k_sweep<SweepConfig<K, Residency::Global, DRIVER, ARITH, DUMP>>, grid, block, p.lds_bytes, a);
}

int launch_sweep(const rl_ctx* ctx, int k, const SweepPlan& p, const rl::SweepArgs& a, bool joint = false, bool strict = false,
                 bool lite = false) {
  using rl::Arith; using rl::Driver; using rl::Residency; using rl::SweepConfig;
  const dim3 grid(a.B), block(rl::kSweepThreads);
  if (strict) {   // RL_ARITH_REFERENCE / _BRANCH: degree-5 splines (the reference's wrap is written for k = 5, optimizer.py:281-285)
#ifdef RL_STAMPS
    if (k == 5 && !joint && !lite && p.residency == Residency::Global)   // diagnostic build: the plain reference-order kernel with its phase stamps in a.dbg
      return launch(ctx, rl::k_sweep<SweepConfig<5, Residency::Global, Driver::Sweep, Arith::Reference>>, grid, block, p.lds_bytes, a);
#endif
    if (k != 5 || a.dbg || (joint && lite)) return fail(RL_ERR_UNSUPPORTED, "reference-order / branch arithmetic: degree-5 splines, no step dump; the sliding-window driver in the reference-order arithmetic only");
    if (joint)    // run_joint_min_curvature_qp in the reference-order arithmetic
      return launch_sweep_in<5, Driver::Window, Arith::Reference>(ctx, p, a);
    if (lite)     // RL_ARITH_BRANCH
      return launch_sweep_in<5, Driver::Sweep, Arith::Branch>(ctx, p, a);
    // the plain kernel flags the instances that need numpy's error state modelled (a sample of exactly zero curvature while
    // numpy is in raise mode); the ReferenceRaise instantiation behind it redoes those and returns at once on all others
    if (int rc = launch_sweep_in<5, Driver::Sweep, Arith::Reference>(ctx, p, a)) return rc;
    return launch_sweep_in<5, Driver::Sweep, Arith::ReferenceRaise>(ctx, p, a);
  }
  if (joint) {
    if (k != 5) return fail(RL_ERR_UNSUPPORTED, "the sliding-window variant is built for degree 5 (span 5)");
    return launch_sweep_in<5, Driver::Window, Arith::Fast>(ctx, p, a);
  }
  if (k == 5 && p.residency == Residency::CrossingsLds)
    return launch(ctx, rl::k_sweep<SweepConfig<5, Residency::CrossingsLds>>, grid, block, p.lds_bytes, a);
#ifdef RL_STAMPS
  if (k == 5 && p.residency == Residency::Global) return launch(ctx, rl::k_sweep<SweepConfig<5, Residency::Global>>, grid, block, p.lds_bytes, a);  // stamps go to a.dbg
#endif
  if (k == 5) {
    if (a.dbg)  // recording instantiation (test aid): same source, one extra store block per step
      return launch_sweep_in<5, Driver::Sweep, Arith::Fast, kRecordSteps>(ctx, p, a);
    return launch_sweep_in<5, Driver::Sweep, Arith::Fast>(ctx, p, a);
  }
  if (k == 3) return launch_sweep_in<3, Driver::Sweep, Arith::Fast>(ctx, p, a);
  return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
}

// The sweep from per-instance start lines / start indices (rl_mincurv_solve_batch_from_*): the SweepConfigFrom instantiations,
// in the residency the plan chose, for every arithmetic of the sweep driver.
template <int K, rl::Arith ARITH>
int launch_sweep_from_in(const rl_ctx* ctx, const SweepPlan& p, const rl::SweepArgs& a) {
  using rl::Residency; using rl::SweepConfigFrom;
  const dim3 grid(a.B), block(rl::kSweepThreads);
  return p.residency == Residency::Lds
             ? launch(ctx, rl::k_sweep<SweepConfigFrom<K, Residency::Lds, ARITH>>, grid, block, p.lds_bytes, a)
             : launch(ctx, rl::k_sweep<SweepConfigFrom<K, Residency::Global, ARITH>>, grid, block, p.lds_bytes, a);
}
int launch_sweep_from(const rl_ctx* ctx, int k, const SweepPlan& p, const rl::SweepArgs& a, bool strict, bool lite) {
  using rl::Arith;
  if (strict) {
    if (k != 5) return fail(RL_ERR_UNSUPPORTED, "reference-order / branch arithmetic: degree-5 splines");
    if (lite) return launch_sweep_from_in<5, Arith::Branch>(ctx, p, a);
    // as launch_sweep: the plain kernel flags, the ReferenceRaise instantiation redoes the flagged instances -- from the same start
    if (int rc = launch_sweep_from_in<5, Arith::Reference>(ctx, p, a)) return rc;
    return launch_sweep_from_in<5, Arith::ReferenceRaise>(ctx, p, a);
  }
  if (k == 5) return launch_sweep_from_in<5, Arith::Fast>(ctx, p, a);
  if (k == 3) return launch_sweep_from_in<3, Arith::Fast>(ctx, p, a);
  return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
}

// The sliding window from per-instance start lines / start indices (rl_mincurv_solve_batch_joint_*): the SweepConfigWindowFrom
// instantiations, in the residency the plan chose, in the two arithmetics the window driver exists in (the reference-order
// loop models numpy's raise mode inline: one launch).
template <rl::Arith ARITH>
int launch_sweep_window_from_in(const rl_ctx* ctx, const SweepPlan& p, const rl::SweepArgs& a) {
  using rl::Residency; using rl::SweepConfigWindowFrom;
  const dim3 grid(a.B), block(rl::kSweepThreads);
  return p.residency == Residency::Lds
             ? launch(ctx, rl::k_sweep<SweepConfigWindowFrom<Residency::Lds, ARITH>>, grid, block, p.lds_bytes, a)
             : launch(ctx, rl::k_sweep<SweepConfigWindowFrom<Residency::Global, ARITH>>, grid, block, p.lds_bytes, a);
}
int launch_sweep_window_from(const rl_ctx* ctx, int k, const SweepPlan& p, const rl::SweepArgs& a, bool strict) {
  using rl::Arith;
  if (k != 5) return fail(RL_ERR_UNSUPPORTED, "the sliding-window variant is built for degree 5 (span 5)");
  if (strict) return launch_sweep_window_from_in<Arith::Reference>(ctx, p, a);
  return launch_sweep_window_from_in<Arith::Fast>(ctx, p, a);
}

// tables of the reference-order mode (rl_kernels.hpp: k_build_tables_strict), built on first use
int ensure_strict_tables(const rl_ctx* ctx, const rl_track* trk) {
  if (trk->strict_valid) return RL_OK;
  const int k = trk->k, N = trk->N;
  if (k != 5) return fail(RL_ERR_UNSUPPORTED, "reference-order arithmetic: degree-5 splines");
  if (!trk->Ds.p) RL_HIP(trk->Ds.alloc((size_t)rl::StrictRows<5>::total * N));
  if (!trk->base_s.p) RL_HIP(trk->base_s.alloc((size_t)6 * N));
  if (int rc = launch(ctx, rl::k_build_tables_strict<5>, dim3((N + 127) / 128), dim3(128), 0, trk->t.p, trk->nt, trk->c0.p, N,
                      trk->Ds.p, trk->base_s.p))
    return rc;
  // like the other table builders: complete (and known to have succeeded) before the tables count as valid -- a later call
  // may arrive on another stream (rl_ctx_set_stream), with no event ordering it behind this launch
  RL_HIP(hipStreamSynchronize(ctx->stream));
  trk->strict_valid = true;
  return RL_OK;
}

// the track's de Boor tables from its knots and control points (rl_kernels.hpp: k_build_tables), complete on return
int build_tables(const rl_ctx* ctx, const rl_track* trk) {
  const int N = trk->N;
  if (int rc = by_degree(trk->k, [&](auto kc) {
        return launch(ctx, rl::k_build_tables<RL_DEGREE(kc)>, dim3((N + 127) / 128), dim3(128), 0, trk->t.p, trk->nt, trk->c0.p, N,
                      trk->ell.p, trk->D.p, trk->base.p);
      }))
    return rc;
  RL_HIP(hipStreamSynchronize(ctx->stream));
  return RL_OK;
}

// The rings an instance is bounded by: the track's shared pair, or N vertices per side that the kernel builds from the
// per-instance input (`in`: widths or bound points).
struct Bounds {
  const double2 *ringL = nullptr, *ringR = nullptr;
  int nL = 0, nR = 0;
};
int resolve_bounds(const rl_track* trk, int form, const double* in, Bounds& b) {
  if (form == RL_BOUNDS_SHARED_RINGS) {
    if (trk->nL == 0) return fail(RL_ERR_ARG, "rl_track_set_rings was not called");
    b.ringL = reinterpret_cast<const double2*>(trk->ringL.p);
    b.ringR = reinterpret_cast<const double2*>(trk->ringR.p);
    b.nL = trk->nL; b.nR = trk->nR;
  } else if (form == RL_BOUNDS_WIDTHS || form == RL_BOUNDS_POINTS) {
    if (!in) return fail(RL_ERR_ARG, "bounds input is null");
    b.nL = trk->N; b.nR = trk->N;
  } else {
    return fail(RL_ERR_ARG, "bad bounds_form");
  }
  return RL_OK;
}
// doubles per sample of the per-instance bounds input (0: the track's shared rings, or no such form)
int bounds_cols(int form) { return form == RL_BOUNDS_WIDTHS ? 2 : (form == RL_BOUNDS_POINTS ? 4 : 0); }

}  // namespace

static int sweep_single(rl_ctx* ctx, rl_track* trk, const int* i_start, int max_iter, double* cx, double* cy,
                        double* points, int* n_success, rl_stats* stats, bool joint);

extern "C" {

int rl_version(void) { return RL_VERSION; }

int rl_debug_dump_enable(int instances) {
  if (instances < 0) return fail(RL_ERR_ARG, "instances < 0");
  g_dbg_instances = instances;
  return RL_OK;
}

int rl_debug_read(double* out, long long n) {
  if (!g_dbg_buf || !out || n < 0 || (size_t)n > g_dbg_len) return fail(RL_ERR_ARG, "no debug dump of that size");
  RL_HIP(hipMemcpy(out, g_dbg_buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return RL_OK;
}

const char* rl_last_error(void) { return g_err.c_str(); }

int rl_ctx_create(int device_id, rl_ctx** out) {
  if (!out) return fail(RL_ERR_ARG, "out is null");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(RL_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= count) return fail(RL_ERR_ARG, "bad device id");
  RL_HIP(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  RL_HIP(hipGetDeviceProperties(&prop, device_id));
  rl_ctx* c = new rl_ctx();
  c->device = device_id;
  c->max_lds = (int)prop.sharedMemPerBlock;  // 160 KiB on gfx950
  {
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess &&
        optin > c->max_lds)
      c->max_lds = optin;
  }
  c->num_cu = prop.multiProcessorCount;
  if (const char* v = getenv("RL_GLOBAL_V1")) c->force_global_v1 = v[0] == '1';
  if (const char* v = getenv("RL_ARITH")) {
    c->arith = (v[0] == 'r' || v[0] == '1') ? RL_ARITH_REFERENCE : ((v[0] == 'b' || v[0] == '2') ? RL_ARITH_BRANCH : RL_ARITH_FAST);
    c->arith_explicit = true;
  }
  if (const char* v = getenv("RL_QSS_DF")) if (v[0] == '0' || v[0] == '1') c->qss_kernel = v[0] - '0';
  if (const char* v = getenv("RL_QSS_V1")) if (v[0] == '1') c->qss_kernel = 0;
  if (const char* v = getenv("RL_QSS_DF_WAVES")) { const int w = atoi(v); if (w == 1 || w == 2 || w == 4) c->qss_df_waves = w; }
  if (const char* v = getenv("RL_QSS_DF_BAIL_AT")) { const int g = atoi(v); if (g >= 0) c->qss_df_bail_at = g; }
  if (const char* v = getenv("RL_MT_HES_SWEEP")) c->mt_hes_sweep = v[0] == '1';
  if (const char* v = getenv("RL_MT_UNFUSED")) c->mt_unfused = v[0] == '1';
  if (const char* v = getenv("RL_MT_KKT4")) c->mt_kkt4 = v[0] == '1';
  if (const char* v = getenv("RL_MT_GROUPS")) { const int g = atoi(v); if (g >= 1 && g <= rl_ctx::kMaxGroups) c->mt_groups = g; }
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    delete c;
    return fail(RL_ERR_HIP, "hipEventCreate failed");
  }
  *out = c;
  return RL_OK;
}

void rl_ctx_destroy(rl_ctx* ctx) {
  if (!ctx) return;
  if (ctx->arena) (void)hipFree(ctx->arena);
  if (ctx->arena_ev) (void)hipEventDestroy(ctx->arena_ev);
  for (auto& blk : ctx->pool)
    if (blk.p) (void)hipFree(blk.p);
  for (int g = 0; g < rl_ctx::kMaxGroups - 1; ++g) {
    if (ctx->aux_stream[g]) (void)hipStreamDestroy(ctx->aux_stream[g]);
    if (ctx->ev_join[g]) (void)hipEventDestroy(ctx->ev_join[g]);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->poll_stream) (void)hipStreamDestroy(ctx->poll_stream);
  for (auto& e : ctx->ev_chunk) if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->ev_poll) if (e) (void)hipEventDestroy(e);
  if (ctx->poll_host) (void)hipHostFree(ctx->poll_host);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  delete ctx;
}

int rl_ctx_set_stream(rl_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(RL_ERR_ARG, "ctx is null");
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return RL_OK;
}

int rl_ctx_set_arith(rl_ctx* ctx, int arith) {
  if (!ctx) return fail(RL_ERR_ARG, "ctx is null");
  if (arith == RL_ARITH_DEFAULT) { ctx->arith = RL_ARITH_REFERENCE; ctx->arith_explicit = false; return RL_OK; }
  if (arith != RL_ARITH_FAST && arith != RL_ARITH_REFERENCE && arith != RL_ARITH_BRANCH)
    return fail(RL_ERR_ARG, "arith must be RL_ARITH_DEFAULT, RL_ARITH_FAST, RL_ARITH_REFERENCE or RL_ARITH_BRANCH");
  ctx->arith = arith;
  ctx->arith_explicit = true;
  return RL_OK;
}

int rl_ctx_get_arith(const rl_ctx* ctx) { return ctx ? (ctx->arith_explicit ? ctx->arith : RL_ARITH_DEFAULT) : RL_ERR_ARG; }

int rl_ctx_set_option(rl_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return fail(RL_ERR_ARG, "null argument");
  const std::string k(name);
  if (k == "qss_kernel") { if (value < -1 || value > 1) return fail(RL_ERR_ARG, "qss_kernel: -1 (auto), 0 (list order), 1 (dataflow)"); ctx->qss_kernel = value; }
  else if (k == "qss_df_waves") { if (value != 1 && value != 2 && value != 4) return fail(RL_ERR_ARG, "qss_df_waves: 1, 2 or 4"); ctx->qss_df_waves = value; }
  else if (k == "qss_df_bail_at") { if (value < 0) return fail(RL_ERR_ARG, "qss_df_bail_at >= 0"); ctx->qss_df_bail_at = value; }
  else if (k == "qss_df_redo") { if (value != 0 && value != 1) return fail(RL_ERR_ARG, "qss_df_redo: 0 or 1"); ctx->qss_df_redo = value; }
  else if (k == "global_last_as_mid") { if (value != 0 && value != 1) return fail(RL_ERR_ARG, "global_last_as_mid: 0 or 1"); ctx->global_last_as_mid = value; }
  else if (k == "sweep_bracket") { if (value != 0 && value != 1) return fail(RL_ERR_ARG, "sweep_bracket: 0 or 1"); ctx->sweep_bracket = value; }
  else if (k == "tables_search") { if (value < RL_SEARCH_BRUTE || value > RL_SEARCH_WINDOWED) return fail(RL_ERR_ARG, "tables_search: RL_SEARCH_BRUTE, _CULLED or _WINDOWED"); ctx->tables_search = value; }
  else if (k == "tables_rings") { if (value != 0 && value != 1) return fail(RL_ERR_ARG, "tables_rings: 0 (LDS where they fit) or 1 (arena)"); ctx->tables_rings_global = value; }
  else if (k == "frenet_search") { if (value != 0 && value != 1) return fail(RL_ERR_ARG, "frenet_search: 0 (table bound for every point) or 1 (from the previous point's piece)"); ctx->frenet_search = value; }
  else return fail(RL_ERR_ARG, "unknown option '" + k + "'");
  return RL_OK;
}

int rl_ctx_set_numpy_raise(rl_ctx* ctx, int on) {
  if (!ctx) return fail(RL_ERR_ARG, "ctx is null");
  ctx->np_raise_at_start = on ? 1 : 0;
  return RL_OK;
}

int rl_debug_cr_heading(rl_ctx* ctx, const double* dx, const double* dy, int n, double* out) {
  if (!ctx || !dx || !dy || !out || n <= 0) return fail(RL_ERR_ARG, "bad argument");
  Staging sg(ctx);
  const double* ddx = sg.in(dx, n);
  const double* ddy = sg.in(dy, n);
  double* dout = sg.out(out, (size_t)5 * n);
  sg.run([&] { return launch(ctx, rl::k_debug_cr_heading, dim3((n + 255) / 256), dim3(256), 0, ddx, ddy, n, dout); });
  return sg.finish();
}

int rl_ctx_synchronize(rl_ctx* ctx) {
  if (!ctx) return fail(RL_ERR_ARG, "ctx is null");
  RL_HIP(hipStreamSynchronize(ctx->stream));
  return RL_OK;
}

// ------------------------------------------------------------------------------------------------
int rl_spline_eval(rl_ctx* ctx, const double* t, int nt, const double* cx, const double* cy, int k,
                   const double* u, int N, int der_max, double* out) {
  if (!ctx || !u || !out) return fail(RL_ERR_ARG, "null argument");
  if (int rc = check_spline(t, nt, cx, cy, k)) return rc;
  if (N <= 0 || der_max < 0 || der_max > 2) return fail(RL_ERR_ARG, "bad N / der_max");
  const int n = nt - k - 1;
  Staging sg(ctx);
  const double *dt = sg.in(t, nt), *dcx = sg.in(cx, n), *dcy = sg.in(cy, n), *du = sg.in(u, N);
  double* dout = sg.out(out, (size_t)2 * (der_max + 1) * N);
  sg.run([&] {
    return by_degree(k, [&](auto kc) {
      return launch(ctx, rl::k_spline_eval<RL_DEGREE(kc)>, dim3((N + 255) / 256), dim3(256), 0, dt, nt, dcx, dcy, du, N, der_max, dout);
    });
  });
  return sg.finish();
}

int rl_sample_along(rl_ctx* ctx, const double* t, int nt, const double* cx, const double* cy, int k,
                    double length, const double* u, int N, double* points) {
  if (!ctx || !u || !points) return fail(RL_ERR_ARG, "null argument");
  if (int rc = check_spline(t, nt, cx, cy, k)) return rc;
  if (N <= 0) return fail(RL_ERR_ARG, "bad N");
  const int n = nt - k - 1;
  Staging sg(ctx);
  const double *dt = sg.in(t, nt), *dcx = sg.in(cx, n), *dcy = sg.in(cy, n), *du = sg.in(u, N);
  double* dpts = sg.out(points, (size_t)N * RL_NCOL);
  double* dseg = sg.scratch<double>(N);
  sg.run([&] {
    if (int rc = by_degree(k, [&](auto kc) {
          return launch(ctx, rl::k_sample_geometry<RL_DEGREE(kc)>, dim3((N + 127) / 128), dim3(128), 0, dt, nt, dcx, dcy, du, N, dpts, dseg);
        }))
      return rc;
    return launch(ctx, rl::k_sample_cumsum, dim3(1), dim3(64), 0, dseg, N, length, dpts);
  });
  return sg.finish();
}

int rl_fill_bounds(rl_ctx* ctx, double* points, int N, const double* ringL, int nL,
                   const double* ringR, int nR, double max_dist) {
  if (!ctx || !points || !ringL || !ringR) return fail(RL_ERR_ARG, "null argument");
  if (N <= 0 || nL < 2 || nR < 2) return fail(RL_ERR_ARG, "bad sizes");
  Staging sg(ctx);
  double* dpts = sg.inout(points, (size_t)N * RL_NCOL);
  const double *dL = sg.in(ringL, (size_t)2 * nL), *dR = sg.in(ringR, (size_t)2 * nR);
  sg.run([&] {
    return launch(ctx, rl::k_fill_bounds, dim3((2 * N + 63) / 64), dim3(64), 0, dpts, N, reinterpret_cast<const double2*>(dL), nL,
                  reinterpret_cast<const double2*>(dR), nR, max_dist);
  });
  return sg.finish();
}

// ------------------------------------------------------------------------------------------------
int rl_track_create(rl_ctx* ctx, const double* t, int nt, const double* cx0, const double* cy0,
                    int k, int N, rl_track** out) {
  if (!ctx || !out) return fail(RL_ERR_ARG, "null argument");
  if (int rc = check_spline(t, nt, cx0, cy0, k)) return rc;
  if (N <= 0) return fail(RL_ERR_ARG, "bad N");
  const int n = nt - k - 1;
  if (n < 2 * k + 1) return fail(RL_ERR_ARG, "too few control points for the periodic wrap");
  RL_HIP(hipSetDevice(ctx->device));
  rl_track* trk = new rl_track();
  trk->ctx = ctx;
  trk->k = k; trk->n = n; trk->nt = nt; trk->N = N;
  trk->t_host.assign(t, t + nt);
  std::vector<int> sup(2 * (size_t)n);
  for (int j = 0; j < n; ++j) {
    const SupportRange r = support_range(trk->t_host, k, N, j);
    sup[2 * j] = r.s0;
    sup[2 * j + 1] = r.s1;
  }
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  ok(trk->t.alloc(nt)); ok(trk->c0.alloc((size_t)2 * n)); ok(trk->D.alloc((size_t)3 * (k + 1) * N));
  ok(trk->base.alloc((size_t)4 * N)); ok(trk->ell.alloc(N)); ok(trk->sup.alloc((size_t)2 * n));
  if (e == hipSuccess) ok(hipMemcpyAsync(trk->t.p, t, nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (e == hipSuccess) ok(hipMemcpyAsync(trk->c0.p, cx0, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (e == hipSuccess) ok(hipMemcpyAsync(trk->c0.p + n, cy0, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (e == hipSuccess) ok(hipMemcpyAsync(trk->sup.p, sup.data(), sup.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const int rc = e == hipSuccess ? build_tables(ctx, trk)   // its synchronisation also covers `sup`, a host vector
                                 : fail(RL_ERR_HIP, std::string("rl_track_create: ") + hipGetErrorString(e));
  if (rc) {
    delete trk;
    return rc;
  }
  *out = trk;
  return RL_OK;
}

void rl_track_destroy(rl_track* trk) { delete trk; }

int rl_track_set_rings(rl_track* trk, const double* ringL, int nL, const double* ringR, int nR) {
  if (!trk || !ringL || !ringR) return fail(RL_ERR_ARG, "null argument");
  if (nL < 3 || nR < 3) return fail(RL_ERR_ARG, "a ring needs at least 3 vertices");
  RL_HIP(hipSetDevice(trk->ctx->device));
  // shapely's LinearRing drops an explicit closing vertex; do the same
  if (ringL[0] == ringL[2 * (nL - 1)] && ringL[1] == ringL[2 * (nL - 1) + 1]) --nL;
  if (ringR[0] == ringR[2 * (nR - 1)] && ringR[1] == ringR[2 * (nR - 1) + 1]) --nR;
  RL_HIP(trk->ringL.alloc((size_t)2 * nL));
  RL_HIP(trk->ringR.alloc((size_t)2 * nR));
  RL_HIP(hipMemcpy(trk->ringL.p, ringL, (size_t)2 * nL * sizeof(double), hipMemcpyHostToDevice));
  RL_HIP(hipMemcpy(trk->ringR.p, ringR, (size_t)2 * nR * sizeof(double), hipMemcpyHostToDevice));
  trk->nL = nL;
  trk->nR = nR;
  return RL_OK;
}

int rl_track_set_length(rl_track* trk, double length) {
  if (!trk) return fail(RL_ERR_ARG, "null argument");
  if (!(length >= 0.0)) return fail(RL_ERR_ARG, "length must be >= 0");
  trk->length = length;
  return RL_OK;
}

int rl_track_set_control_points(rl_track* trk, const double* cx0, const double* cy0) {
  if (!trk || !cx0 || !cy0) return fail(RL_ERR_ARG, "null argument");
  rl_ctx* ctx = trk->ctx;
  RL_HIP(hipSetDevice(ctx->device));
  const int n = trk->n;
  RL_HIP(hipMemcpyAsync(trk->c0.p, cx0, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(hipMemcpyAsync(trk->c0.p + n, cy0, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = build_tables(ctx, trk)) return rc;
  trk->gq_valid = false;
  trk->gxy_valid = false;
  trk->strict_valid = false;
  return RL_OK;
}

// ------------------------------------------------------------------------------------------------
int rl_mincurv_cost(rl_ctx* ctx, const rl_track* trk, const int* idx, int n_idx, const double* z,
                    double* H, double* g, int* M) {
  if (!ctx || !trk || !idx || !H || !g) return fail(RL_ERR_ARG, "null argument");
  if (n_idx <= 0) return fail(RL_ERR_ARG, "n_idx <= 0");
  for (int q = 0; q < n_idx; ++q)
    if (idx[q] < 0 || idx[q] >= trk->n) return fail(RL_ERR_ARG, "control point index out of range");
  const bool strict = ctx->arith == RL_ARITH_REFERENCE && trk->k == 5;   // the oracle's bits (orc_min_curvature_cost)
  Staging sg(ctx);
  const int* didx = sg.in(idx, n_idx);
  const double* dz = sg.in(z, (size_t)2 * n_idx);
  double *dH = sg.out(H, (size_t)4 * n_idx), *dg = sg.out(g, (size_t)2 * n_idx);
  int* dM = sg.out_optional(M, n_idx);
  sg.run([&] {
    if (strict) if (int rc = ensure_strict_tables(ctx, trk)) return rc;
    const rl::TrackDev td = trk->dev();
    const double *cx = trk->c0.p, *cy = trk->c0.p + trk->n;
    const dim3 grid(n_idx), block(256);
    if (strict) return launch(ctx, rl::k_cost_strict<5>, grid, block, 0, td, cx, cy, didx, dz, dH, dg, dM);
    return by_degree(trk->k, [&](auto kc) { return launch(ctx, rl::k_cost<RL_DEGREE(kc)>, grid, block, 0, td, cx, cy, didx, dz, dH, dg, dM); });
  });
  return sg.finish();
}

// host weights of the weighted cost: finite, positive, within [2^-30, 2^30] (rl_kernels.hpp: kWeightMin / kWeightMax)
static bool weights_ok(const double* w, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!(w[i] >= rl::kWeightMin && w[i] <= rl::kWeightMax)) return false;   // NaN fails both comparisons
  return true;
}

int rl_mincurv_cost_weighted(rl_ctx* ctx, const rl_track* trk, const int* idx, int n_idx, const double* z, const double* weights,
                             double* H, double* g, int* M) {
  if (!ctx || !trk || !idx || !weights || !H || !g) return fail(RL_ERR_ARG, "null argument");
  if (n_idx <= 0) return fail(RL_ERR_ARG, "n_idx <= 0");
  for (int q = 0; q < n_idx; ++q)
    if (idx[q] < 0 || idx[q] >= trk->n) return fail(RL_ERR_ARG, "control point index out of range");
  if (!weights_ok(weights, trk->N)) return fail(RL_ERR_ARG, "weights must be finite and within [2^-30, 2^30]");
  const bool strict = ctx->arith == RL_ARITH_REFERENCE && trk->k == 5;
  Staging sg(ctx);
  const int* didx = sg.in(idx, n_idx);
  const double* dz = sg.in(z, (size_t)2 * n_idx);
  const double* dw = sg.in(weights, trk->N);
  double *dH = sg.out(H, (size_t)4 * n_idx), *dg = sg.out(g, (size_t)2 * n_idx);
  int* dM = sg.out_optional(M, n_idx);
  sg.run([&] {
    if (strict) if (int rc = ensure_strict_tables(ctx, trk)) return rc;
    const rl::TrackDev td = trk->dev();
    const double *cx = trk->c0.p, *cy = trk->c0.p + trk->n;
    const dim3 grid(n_idx), block(256);
    if (strict) return launch(ctx, rl::k_cost_strict_weighted<5>, grid, block, 0, td, cx, cy, didx, dz, dw, dH, dg, dM);
    return by_degree(trk->k, [&](auto kc) { return launch(ctx, rl::k_cost_weighted<RL_DEGREE(kc)>, grid, block, 0, td, cx, cy, didx, dz, dw, dH, dg, dM); });
  });
  return sg.finish();
}

int rl_track_constraint(rl_ctx* ctx, const rl_track* trk, const double* points, int idx,
                        double* b, double* lba, double* uba, int* M) {
  if (!ctx || !trk || !points || !b || !lba || !uba || !M) return fail(RL_ERR_ARG, "null argument");
  if (idx < 0 || idx >= trk->n) return fail(RL_ERR_ARG, "control point index out of range");
  const int N = trk->N, k = trk->k;
  const SupportRange sup = support_range(trk->t_host, k, N, idx);
  const int m = sup.s1 - sup.s0;
  *M = m;
  if (m == 0) return RL_OK;
  const bool strict = ctx->arith == RL_ARITH_REFERENCE && k == 5;        // the oracle's bits (orc_track_constraint)
  Staging sg(ctx);
  const double* dpts = sg.in(points, (size_t)N * RL_NCOL);
  double *db = sg.out(b, m), *dl = sg.out(lba, (size_t)2 * m), *du = sg.out(uba, (size_t)2 * m);
  sg.run([&] {
    if (strict) if (int rc = ensure_strict_tables(ctx, trk)) return rc;
    const rl::TrackDev td = trk->dev();
    const double *cx = trk->c0.p, *cy = trk->c0.p + trk->n;
    const dim3 grid((m + 255) / 256), block(256);
    if (strict) return launch(ctx, rl::k_constraint_strict<5>, grid, block, 0, td, cx, cy, dpts, idx, db, dl, du);
    return by_degree(k, [&](auto kc) { return launch(ctx, rl::k_constraint<RL_DEGREE(kc)>, grid, block, 0, td, cx, cy, dpts, idx, db, dl, du); });
  });
  return sg.finish();
}

// ------------------------------------------------------------------------------------------------
static int solve_batch_common(rl_ctx* ctx, const rl_track* trk, int form, const double* in_dev,
                              int B, const int* i_start, int max_iter, int search,
                              double* out_ctrl, double* out_xy, double* out_points, int* n_success,
                              int* status, rl_stats* stats, SweepPlan* plan_out, bool joint = false,
                              const double* ctrl0 = nullptr, const int* i_start_rows = nullptr, bool joint_batch = false) {
  // ctrl0 / i_start_rows (DEVICE, rl_mincurv_solve_batch_from_*): per-instance start lines / start indices; `i_start` is then
  // unused when rows are given.  joint_batch (rl_mincurv_solve_batch_joint_*): the sliding window on the SweepConfigWindowFrom
  // instantiations, whatever ctrl0 and the rows are -- one path, one n_success layout [B,max_iter]
  const bool from = ctrl0 || i_start_rows || joint_batch;
  if (!ctx || !trk || (!i_start && !i_start_rows) || !out_ctrl) return fail(RL_ERR_ARG, "null argument");
  if (from && joint && !joint_batch) return fail(RL_ERR_UNSUPPORTED, "the sliding-window driver has no per-instance start lines");
  if (!out_xy && !out_points) return fail(RL_ERR_ARG, "need out_xy or out_points");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  if (max_iter <= 0 || max_iter > RL_MAX_ITER) return fail(RL_ERR_ARG, "max_iter out of range");
  if (search < RL_SEARCH_BRUTE || search > RL_SEARCH_WINDOWED) return fail(RL_ERR_ARG, "bad search mode");
  const int n = trk->n, N = trk->N, k = trk->k;
  if (joint_batch && k != 5) return fail(RL_ERR_UNSUPPORTED, "the sliding-window variant is built for degree 5 (span 5)");
  const int i_min = k / 2, i_max = n - (k - k / 2) - (joint ? 5 : 0);
  if (i_max <= i_min) return fail(RL_ERR_ARG, "too few control points");
  for (int j = 0; j < max_iter && !i_start_rows; ++j)
    if (i_start[j] < i_min || i_start[j] >= i_max)
      return fail(RL_ERR_ARG, joint ? "i_start outside [k//2, n-(k-k//2)-span) (optimizer.py:176-178)"
                                    : "i_start outside [k//2, n-(k-k//2)) (optimizer.py:301-303)");
  if (joint) {  // the window rows live in registers: 3 per thread
    int widest = 0;
    for (int kk = i_min; kk < i_max; ++kk) {
      const SupportRange w = support_range(trk->t_host, k, N, kk, 5);
      widest = std::max(widest, w.s1 - w.s0);
    }
    if (widest > rl::kJointRowsPerThread * 256)
      return fail(RL_ERR_UNSUPPORTED, "sliding-window variant: a window spans more than 768 samples");
  }
  // the DEFAULT arithmetic is the reference-order one where it exists (degree-5 splines, no step dump) and the fast one
  // elsewhere; an arithmetic chosen with rl_ctx_set_arith / RL_ARITH is taken literally (and fails where it does not exist).
  // rl_stats.reserved[0] names the arithmetic that ran.
  int arith = ctx->arith;
  if (!ctx->arith_explicit && arith == RL_ARITH_REFERENCE && (k != 5 || (g_dbg_instances > 0 && !from))) arith = RL_ARITH_FAST;
  const bool lite = arith == RL_ARITH_BRANCH;
  const bool strict = arith == RL_ARITH_REFERENCE || lite;    // the branch mode shares the reference-order kernel's tables and state
  if (strict) {
    if (joint && lite) return fail(RL_ERR_UNSUPPORTED, "the branch arithmetic (rl_ctx_set_arith) covers run_min_curvature_qp; the sliding-window driver exists in the fast and in the reference-order arithmetic");
    RL_HIP(hipSetDevice(ctx->device));
    if (int rc = ensure_strict_tables(ctx, trk)) return rc;
  }
  rl::SweepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.tr = trk->dev();
  a.B = B;
  a.form = form;
  a.in = in_dev;
  Bounds bd;
  if (int rc = resolve_bounds(trk, form, in_dev, bd)) return rc;
  a.ringL = bd.ringL; a.ringR = bd.ringR; a.nL = bd.nL; a.nR = bd.nR;
  a.max_iter = max_iter;
  for (int j = 0; j < max_iter && !i_start_rows; ++j) a.i_start[j] = i_start[j];
  a.ctrl0 = ctrl0; a.i_start_rows = i_start_rows;
  a.bracket = ctx->sweep_bracket;
  a.search = search;
  a.max_dist = 100.0;  // race_track.py:104
#ifdef RL_ABLATION
  if (const char* dbg = getenv("RL_DEBUG_FLAGS")) a.debug = atoi(dbg);
#endif
#ifdef RL_STAMPS
  const bool dbg_ok = true;
#else
  const bool dbg_ok = !strict;
#endif
  if (g_dbg_instances > 0 && (joint || k == 5) && dbg_ok && !from) {   // (no recording instantiation from per-instance starts)
    const int ninst = std::min(g_dbg_instances, B);
    size_t need = joint ? (size_t)max_iter * (size_t)(i_max - i_min) * (48 + 9 * rl::kJointRowsPerThread * 256 + 2 * n)
                        : (size_t)ninst * max_iter * 2 * (size_t)(i_max - i_min) * (rl::kSweepDumpHead + 2 * n);
#ifdef RL_STAMPS
    need = std::max(need, (size_t)B * 4 * 19);   // diagnostic build: per-wave phase stamps of every instance, [B][4][16], and behind them [B][4] prologue cycles, [B][4] window scans, [B][4] bracketed scans
#endif
    a.dbg_instances = ninst;
    if (g_dbg_len < need) {
      if (g_dbg_buf) (void)hipFree(g_dbg_buf);
      RL_HIP(hipMalloc(reinterpret_cast<void**>(&g_dbg_buf), need * sizeof(double)));
      g_dbg_len = need;
    }
    RL_HIP(hipMemsetAsync(g_dbg_buf, 0, need * sizeof(double), ctx->stream));
    a.dbg = g_dbg_buf;
  }
  a.out_ctrl = out_ctrl; a.out_xy = out_xy; a.out_points = out_points;
  a.n_success = n_success; a.status = status;
  RL_HIP(hipSetDevice(ctx->device));
  SweepPlan p = plan_sweep(ctx, n, N, a.nL, a.nR, B, joint, strict);
  if (p.lds_bytes > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "problem does not fit LDS");
  if (p.residency == rl::Residency::CrossingsLds && (joint || k != 5 || a.dbg || from)) {   // the mixed residency exists for the k = 5 sweep only
    p.residency = rl::Residency::Global;
    p.lds_bytes = rl::sweep_lds_layout(n, N, a.nL, a.nR, rl::Residency::Global, joint).total * sizeof(double);
    p.gscratch_doubles += (size_t)2 * ((N + 1) & ~1);
  }
  if (p.gscratch_doubles) {
    const size_t need = p.gscratch_doubles * (size_t)B;
    if (trk->gscratch.n < need) RL_HIP(trk->gscratch.alloc(need));
    a.gscratch = trk->gscratch.p;
    a.gscratch_stride = p.gscratch_doubles;
  }
  if (strict && !lite) {
    // per instance: [2 cpad] reserved | [ceil(N/16)*2] doubles of per-sample flag bytes | [N] double2 snapshot of the table's X, Y
    const size_t per = (size_t)2 * ((n + 1) & ~1) + (size_t)2 * ((N + 15) / 16) + (size_t)2 * N;
    const size_t flags = ((size_t)B + 1) / 2;    // [B] ints behind the per-instance blocks
    if (trk->aux.n < per * (size_t)B + flags) RL_HIP(trk->aux.alloc(per * (size_t)B + flags));
    a.aux = trk->aux.p;
    a.aux_stride = per;
    a.np_raise_at_start = ctx->np_raise_at_start;
    a.raise_flag = reinterpret_cast<int*>(trk->aux.p + per * (size_t)B);
    RL_HIP(hipMemsetAsync(a.raise_flag, 0, (size_t)B * sizeof(int), ctx->stream));
  }
  if (stats) {
    stats->lds_bytes = (int)p.lds_bytes;
    stats->block_threads = p.block;
    stats->rings_in_lds = p.residency == rl::Residency::Lds ? 1 : (p.residency == rl::Residency::CrossingsLds ? 2 : 0);
    stats->reserved[0] = arith;
  }
  if (plan_out) *plan_out = p;
  if (joint_batch) return launch_sweep_window_from(ctx, k, p, a, strict);
  if (from) return launch_sweep_from(ctx, k, p, a, strict, lite);
  return launch_sweep(ctx, k, p, a, joint, strict, lite);
}

int rl_mincurv_solve_batch_dev(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in,
                               int B, const int* i_start, int max_iter, int search,
                               double* out_ctrl, double* out_xy, int* n_success, int* status,
                               rl_stats* stats) {
  if (!out_xy) return fail(RL_ERR_ARG, "out_xy is null");
  return solve_batch_common(ctx, trk, bounds_form, in, B, i_start, max_iter, search, out_ctrl, out_xy,
                            nullptr, n_success, status, stats, nullptr);
}

int rl_mincurv_solve_batch_host(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in,
                                int B, const int* i_start, int max_iter, int search,
                                double* out_ctrl, double* out_xy, int* n_success, int* status,
                                rl_stats* stats) {
  if (!ctx || !trk || !out_ctrl || !out_xy) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  const int n = trk->n, N = trk->N;
  const int cols = bounds_cols(bounds_form);
  if (cols && !in) return fail(RL_ERR_ARG, "bounds input is null");
  Staging sg(ctx);
  const double* din = cols ? sg.in(in, (size_t)B * N * cols) : nullptr;
  double *dctrl = sg.out(out_ctrl, (size_t)B * n * 2), *dxy = sg.out(out_xy, (size_t)B * N * 2);
  int* dns = sg.out_optional(n_success, (size_t)B * 2 * (max_iter > 0 ? max_iter : 1));
  int* dst = sg.out_optional(status, B);
  sg.run_timed([&] {
    return solve_batch_common(ctx, trk, bounds_form, din, B, i_start, max_iter, search, dctrl, dxy, nullptr, dns, dst, stats, nullptr);
  });
  return sg.finish(stats);
}

// Host pointers of the per-instance entry points (rl_mincurv_solve_batch_from_host / _joint_host): validates host rows against
// the driver's range, stages, runs solve_batch_common, copies back.  joint_batch: the sliding-window driver (its range ends a span
// earlier, it counts once per outer iteration).
static int solve_batch_from_host_common(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in, int B,
                                        const double* ctrl0, const int* i_start, int i_start_per_instance, int max_iter,
                                        int search, double* out_ctrl, double* out_xy, int* n_success, int* status,
                                        rl_stats* stats, bool joint_batch) {
  if (!ctx || !trk || !out_ctrl || !out_xy || !i_start) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  if (max_iter <= 0 || max_iter > RL_MAX_ITER) return fail(RL_ERR_ARG, "max_iter out of range");
  const int n = trk->n, N = trk->N, k = trk->k;
  if (i_start_per_instance) {   // host rows are validated here; the kernel's own check is for rows that never were on the host
    const int i_min = k / 2, i_max = n - (k - k / 2) - (joint_batch ? 5 : 0);
    for (size_t j = 0; j < (size_t)B * max_iter; ++j)
      if (i_start[j] < i_min || i_start[j] >= i_max)
        return fail(RL_ERR_ARG, joint_batch ? "i_start outside [k//2, n-(k-k//2)-span) (optimizer.py:176-178)"
                                            : "i_start outside [k//2, n-(k-k//2)) (optimizer.py:301-303)");
  }
  const int cols = bounds_cols(bounds_form);
  if (cols && !in) return fail(RL_ERR_ARG, "bounds input is null");
  Staging sg(ctx);
  const double* din = cols ? sg.in(in, (size_t)B * N * cols) : nullptr;
  const double* dc0 = sg.in(ctrl0, (size_t)B * n * 2);
  const int* drows = i_start_per_instance ? sg.in(i_start, (size_t)B * max_iter) : nullptr;
  double *dctrl = sg.out(out_ctrl, (size_t)B * n * 2), *dxy = sg.out(out_xy, (size_t)B * N * 2);
  int* dns = sg.out_optional(n_success, (size_t)B * (joint_batch ? 1 : 2) * max_iter);
  int* dst = sg.out_optional(status, B);
  sg.run_timed([&] {
    return solve_batch_common(ctx, trk, bounds_form, din, B, i_start_per_instance ? nullptr : i_start, max_iter, search, dctrl, dxy,
                              nullptr, dns, dst, stats, nullptr, joint_batch, dc0, drows, joint_batch);
  });
  return sg.finish(stats);
}

int rl_mincurv_solve_batch_from_dev(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in, int B,
                                    const double* ctrl0, const int* i_start, int i_start_per_instance, int max_iter,
                                    int search, double* out_ctrl, double* out_xy, int* n_success, int* status, rl_stats* stats) {
  if (!out_xy) return fail(RL_ERR_ARG, "out_xy is null");
  if (!i_start) return fail(RL_ERR_ARG, "i_start is null");
  return solve_batch_common(ctx, trk, bounds_form, in, B, i_start_per_instance ? nullptr : i_start, max_iter, search, out_ctrl,
                            out_xy, nullptr, n_success, status, stats, nullptr, false, ctrl0,
                            i_start_per_instance ? i_start : nullptr);
}

int rl_mincurv_solve_batch_from_host(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in, int B,
                                     const double* ctrl0, const int* i_start, int i_start_per_instance, int max_iter,
                                     int search, double* out_ctrl, double* out_xy, int* n_success, int* status, rl_stats* stats) {
  return solve_batch_from_host_common(ctx, trk, bounds_form, in, B, ctrl0, i_start, i_start_per_instance, max_iter, search,
                                      out_ctrl, out_xy, n_success, status, stats, false);
}

// ---- the sliding-window driver, batched: per-instance start lines, start indices and bounds
int rl_mincurv_solve_batch_joint_dev(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in, int B,
                                     const double* ctrl0, const int* i_start, int i_start_per_instance, int max_iter,
                                     int search, double* out_ctrl, double* out_xy, int* n_success, int* status, rl_stats* stats) {
  if (!out_xy) return fail(RL_ERR_ARG, "out_xy is null");
  if (!i_start) return fail(RL_ERR_ARG, "i_start is null");
  return solve_batch_common(ctx, trk, bounds_form, in, B, i_start_per_instance ? nullptr : i_start, max_iter, search, out_ctrl,
                            out_xy, nullptr, n_success, status, stats, nullptr, true, ctrl0,
                            i_start_per_instance ? i_start : nullptr, true);
}

int rl_mincurv_solve_batch_joint_host(rl_ctx* ctx, const rl_track* trk, int bounds_form, const double* in, int B,
                                      const double* ctrl0, const int* i_start, int i_start_per_instance, int max_iter,
                                      int search, double* out_ctrl, double* out_xy, int* n_success, int* status, rl_stats* stats) {
  return solve_batch_from_host_common(ctx, trk, bounds_form, in, B, ctrl0, i_start, i_start_per_instance, max_iter, search,
                                      out_ctrl, out_xy, n_success, status, stats, true);
}

// ---- periodic least-squares fit onto the track's knots (rl_spline_fit.hpp)
static int spline_fit_check(const rl_ctx* ctx, const rl_track* trk, const double* xy, int B, int P, int stride, const double* out_ctrl,
                            const double* out_stats, size_t& lds_bytes) {
  if (!ctx || !trk || !xy || !out_ctrl || !out_stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  if (stride < 2) return fail(RL_ERR_ARG, "stride < 2");
  const int m = trk->n - trk->k;
  if (m < 2 * trk->k + 1 || m > rl::kFitMaxM) return fail(RL_ERR_UNSUPPORTED, "spline fit: 2k+1 <= n-k <= 192");
  if (P < 1 || P > rl::kFitMaxP) return fail(RL_ERR_UNSUPPORTED, "spline fit: 1 <= P <= 4096");
  lds_bytes = rl::fit_lds_layout(trk->k, m, P).total_bytes;
  if (lds_bytes > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "spline fit: problem does not fit LDS");
  return RL_OK;
}

int rl_spline_fit_batch_dev(rl_ctx* ctx, const rl_track* trk, const double* xy, int B, int P, int stride, const double* u,
                            int u_per_instance, double* out_ctrl, double* out_stats) {
  size_t lds = 0;
  if (int rc = spline_fit_check(ctx, trk, xy, B, P, stride, out_ctrl, out_stats, lds)) return rc;
  RL_HIP(hipSetDevice(ctx->device));
  const rl::TrackDev td = trk->dev();
  return by_degree(trk->k, [&](auto kc) {
    return launch(ctx, rl::k_spline_fit<RL_DEGREE(kc)>, dim3(B), dim3(rl::kFitThreads), lds, td, xy, P, stride, u,
                  u_per_instance, out_ctrl, out_stats);
  });
}

int rl_spline_fit_batch_host(rl_ctx* ctx, const rl_track* trk, const double* xy, int B, int P, int stride, const double* u,
                             int u_per_instance, double* out_ctrl, double* out_stats) {
  size_t lds = 0;
  if (int rc = spline_fit_check(ctx, trk, xy, B, P, stride, out_ctrl, out_stats, lds)) return rc;
  Staging sg(ctx);
  const double* dxy = sg.in(xy, (size_t)B * P * stride);
  const double* du = sg.in(u, u_per_instance ? (size_t)B * P : (size_t)P);
  double* dctrl = sg.out(out_ctrl, (size_t)B * trk->n * 2);
  double* dstats = sg.out(out_stats, (size_t)B * 4);
  sg.run([&] { return rl_spline_fit_batch_dev(ctx, trk, dxy, B, P, stride, du, u_per_instance, dctrl, dstats); });
  return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// a15: global min-curvature QP (rl_global.hpp)
extern "C++" {
namespace {

int host_find_interval(const std::vector<double>& t, int k, int n, double x) {
  int lo = k, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (x >= t[mid]) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Track-level tables: constraint rows, control-point normals, and the partition of the sample
// grid into chunks of <= kGRows consecutive samples of one knot span.
int global_tables(const rl_ctx* ctx, const rl_track* trk) {
  if (trk->gq_valid) return RL_OK;
  const int k = trk->k, n = trk->n, N = trk->N, np = n - k;
  if (np < 2 * (k + 1)) return fail(RL_ERR_UNSUPPORTED, "too few control points for the global QP");
  if (np > rl::kGMaxNp) return fail(RL_ERR_UNSUPPORTED, "global QP: more than 192 free control points");
  if (N >= (1 << 24)) return fail(RL_ERR_UNSUPPORTED, "global QP: N too large");
  std::vector<int> rows(np, 0);
  const double step = 1.0 / (double)N;
  for (int i = 0; i < N; ++i) ++rows[host_find_interval(trk->t_host, k, n, (double)i * step) - k];
  auto partition = [&](int R, std::vector<int>& chunk, std::vector<int>& span) {
    chunk.clear(); span.assign(np + 1, 0);
    int row = 0;
    for (int s = 0; s < np; ++s) {
      span[s] = (int)chunk.size() / 2;
      for (int r = 0; r < rows[s]; r += R) {
        const int c = std::min(R, rows[s] - r);
        chunk.push_back((row + r) | (c << 24));
        chunk.push_back(s);
      }
      row += rows[s];
    }
    span[np] = (int)chunk.size() / 2;
    return span[np];
  };
  std::vector<int> chunk, span, chunk2, span2;
  const int nc = partition(rl::kGRows, chunk, span);
  int rows2 = 0, nc2 = 0;
  for (int R : {5, 6, 10}) {  // fewest rows per thread whose chunks fit the row waves of k_global_qp2
    nc2 = partition(R, chunk2, span2);
    if (nc2 <= rl::kG2Block - 64) { rows2 = R; break; }
  }
  if (nc > 1024) return fail(RL_ERR_UNSUPPORTED, "global QP: N / 8 + n exceeds one workgroup");
  RL_HIP(trk->gq2_chunk.alloc(chunk2.size())); RL_HIP(trk->gq2_span.alloc(span2.size()));
  RL_HIP(hipMemcpyAsync(trk->gq2_chunk.p, chunk2.data(), chunk2.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(hipMemcpyAsync(trk->gq2_span.p, span2.data(), span2.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(trk->gq_A.alloc((size_t)N * (k + 1))); RL_HIP(trk->gq_nu.alloc((size_t)2 * np));
  RL_HIP(trk->gq_chunk.alloc(chunk.size())); RL_HIP(trk->gq_span.alloc(span.size()));
  RL_HIP(hipMemcpyAsync(trk->gq_chunk.p, chunk.data(), chunk.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(hipMemcpyAsync(trk->gq_span.p, span.data(), span.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const rl::TrackDev td = trk->dev();
  if (int rc = by_degree(k, [&](auto kc) {
        if (int rc = launch(ctx, rl::k_global_normals<RL_DEGREE(kc)>, dim3((np + 63) / 64), dim3(64), 0, td, np, trk->gq_nu.p)) return rc;
        return launch(ctx, rl::k_global_rows<RL_DEGREE(kc)>, dim3((N + 127) / 128), dim3(128), 0, td, np, trk->gq_nu.p, trk->gq_A.p);
      }))
    return rc;
  RL_HIP(hipStreamSynchronize(ctx->stream));  // chunk / span are host vectors
  trk->gq_nc = nc;
  trk->gq2_nc = nc2;
  trk->gq2_rows = rows2;
  trk->gq_valid = true;
  return RL_OK;
}

// weights: null = the unweighted kernels (the bits they always returned); else [B][N] on the device, the weighted kernels of
// the same dispatch (they validate the weights themselves)
int global_common(rl_ctx* ctx, const rl_track* trk, const double* widths, const double* weights, int B, double margin, int n_outer,
                  double* out_ctrl, double* out_xy, double* out_a, double* out_stats, rl_stats* stats) {
  if (!ctx || !trk || !widths || !out_ctrl || !out_stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  if (n_outer < 0 || n_outer > 64) return fail(RL_ERR_ARG, "n_outer out of range");
  if (!degree_supported(trk->k)) return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
  RL_HIP(hipSetDevice(ctx->device));
  if (int rc = global_tables(ctx, trk)) return rc;
  rl::GlobalArgs a;
  a.trk = trk->dev();
  a.A = trk->gq_A.p; a.nu = trk->gq_nu.p; a.chunk = trk->gq_chunk.p; a.span_ch0 = trk->gq_span.p;
  a.nc = trk->gq_nc; a.np = trk->n - trk->k;
  a.widths = widths; a.margin = margin; a.n_outer = n_outer; a.max_ipm = 80; a.last_as_mid = ctx->global_last_as_mid;
  a.out_ctrl = out_ctrl; a.out_xy = out_xy; a.out_a = out_a; a.out_stats = out_stats;
  a.weights = weights;
  // the two compile-time choices of every launch below: f(spline degree K, weighted cost W)
  auto by_kernel = [&](auto&& f) {
    return by_degree(trk->k, [&](auto kc) { return by_flag(weights != nullptr, [&](auto wc) { return f(kc, wc); }); });
  };
  // fast path: wave-specialised kernel (rl_global2.hpp) when the chunks fit 7 row waves and the LDS
  if (!ctx->force_global_v1 && trk->gq2_rows != 0 && a.np <= 192) {
    const int groups = a.np <= 64 ? 1 : 3;
    const int block2 = ((trk->gq2_nc + 63) / 64 + 1) * 64;
    const size_t lds2 = (size_t)rl::global2_layout(trk->k, trk->n, a.np, trk->N, groups, block2 - 64).total * sizeof(double);
    if (lds2 <= (size_t)ctx->max_lds) {
      // R = 5, 6: constraint rows register resident; R = 10 (N up to ~4400): re-read from L2, one group only
      const int R = trk->gq2_rows;
      if (R != 10 || groups == 1) {
        a.chunk = trk->gq2_chunk.p; a.span_ch0 = trk->gq2_span.p; a.nc = trk->gq2_nc;
        if (stats) { stats->lds_bytes = (int)lds2; stats->block_threads = block2; stats->rings_in_lds = 0; }
        return by_kernel([&](auto kc, auto wc) {
          constexpr int K = RL_DEGREE(kc);
          constexpr bool W = RL_DEGREE(wc);
          const dim3 grid(B), blk(block2);
          if (R == 5) return groups == 1 ? launch(ctx, rl::k_global_qp2<K, 5, 1, true, W>, grid, blk, lds2, a) : launch(ctx, rl::k_global_qp2<K, 5, 3, true, W>, grid, blk, lds2, a);
          if (R == 6) return groups == 1 ? launch(ctx, rl::k_global_qp2<K, 6, 1, true, W>, grid, blk, lds2, a) : launch(ctx, rl::k_global_qp2<K, 6, 3, true, W>, grid, blk, lds2, a);
          return launch(ctx, rl::k_global_qp2<K, 10, 1, false, W>, grid, blk, lds2, a);
        });
      }
    }
  }
  const int block = std::max(64, (a.nc + 63) / 64 * 64);
  const size_t lds = (size_t)rl::global_layout(trk->k, trk->n, a.np, block).total * sizeof(double);
  if (lds > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "global QP does not fit LDS");
  if (stats) { stats->lds_bytes = (int)lds; stats->block_threads = block; stats->rings_in_lds = 0; }
  return by_kernel([&](auto kc, auto wc) {
    constexpr int K = RL_DEGREE(kc);
    constexpr bool W = RL_DEGREE(wc);
    if (block <= 384) return launch(ctx, rl::k_global_qp<K, 384, W>, dim3(B), dim3(block), lds, a);
    if (block <= 640) return launch(ctx, rl::k_global_qp<K, 640, W>, dim3(B), dim3(block), lds, a);
    return launch(ctx, rl::k_global_qp<K, 1024, W>, dim3(B), dim3(block), lds, a);
  });
}

// ---- the two-coordinate formulation (rl_global_xy.hpp)
int global_xy_tables(const rl_ctx* ctx, const rl_track* trk) {
  if (trk->gxy_valid) return RL_OK;
  const int k = trk->k, n = trk->n, N = trk->N, np = n - k;
  if (np < 2 * (k + 1)) return fail(RL_ERR_UNSUPPORTED, "too few control points for the global QP");
  if (2 * np > rl::kXYMaxNz) return fail(RL_ERR_UNSUPPORTED, "global QP (dof 2): more than 96 free control points");
  std::vector<int> first(np + 1, 0);
  const double step = 1.0 / (double)N;
  int prev = -1;
  for (int i = 0; i < N; ++i) {   // spans are consecutive sample ranges; empty spans get the next span's first sample
    const int s = host_find_interval(trk->t_host, k, n, (double)i * step) - k;
    for (int q = prev + 1; q <= s; ++q) first[q] = i;
    prev = std::max(prev, s);
  }
  for (int q = prev + 1; q <= np; ++q) first[q] = N;
  RL_HIP(trk->gxy_span.alloc(first.size()));
  RL_HIP(hipMemcpyAsync(trk->gxy_span.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  // chunks: the samples of a span in pieces of <= CL samples.  The adaptive knots give spans of very different lengths (Monza
  // s = 100, N = 2000: 2 .. 281 samples), and a task per span waits for the longest.  The shortest CL whose chunk sums fit LDS.
  std::vector<int> cf, sc0(np + 1, 0);
  for (int CL = 33;; CL = (CL + CL / 2) | 1) {   // (odd: the chunks of a long span then start on different LDS banks)
    cf.clear();
    for (int s = 0; s < np; ++s) {
      sc0[s] = (int)cf.size();
      for (int m = first[s]; m < first[s + 1]; m += CL) cf.push_back(m);
    }
    sc0[np] = (int)cf.size();
    cf.push_back(N);
    const size_t lds = (size_t)rl::global_xy_layout(k, n, np, N, sc0[np]).total * sizeof(double);
    if (lds <= (size_t)ctx->max_lds || CL >= N) break;
  }
  trk->gxy_nch = sc0[np];
  RL_HIP(trk->gxy_chunk.alloc(cf.size())); RL_HIP(trk->gxy_sch0.alloc(sc0.size()));
  RL_HIP(hipMemcpyAsync(trk->gxy_chunk.p, cf.data(), cf.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(hipMemcpyAsync(trk->gxy_sch0.p, sc0.data(), sc0.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const int K1 = k + 1;
  RL_HIP(trk->gxy_bbx.alloc((size_t)N * (K1 * (K1 + 1) / 2 + K1)));
  const rl::TrackDev td = trk->dev();
  if (int rc = by_degree(k, [&](auto kc) {
        return launch(ctx, rl::k_global_xy_pairs<RL_DEGREE(kc)>, dim3((N + 127) / 128), dim3(128), 0, td, trk->gxy_bbx.p);
      }))
    return rc;
  RL_HIP(hipStreamSynchronize(ctx->stream));  // `first`, `cf`, `sc0` are host vectors
  trk->gxy_valid = true;
  return RL_OK;
}

int global_xy_common(rl_ctx* ctx, const rl_track* trk, const double* widths, int B, double margin, double lon, int n_outer,
                     double* out_ctrl, double* out_xy, double* out_z, double* out_stats, rl_stats* stats) {
  if (!ctx || !trk || !widths || !out_ctrl || !out_stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  if (n_outer < 0 || n_outer > 64) return fail(RL_ERR_ARG, "n_outer out of range");
  if (!(lon > 0.0)) return fail(RL_ERR_ARG, "the longitudinal bound must be positive");
  if (!degree_supported(trk->k)) return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
  RL_HIP(hipSetDevice(ctx->device));
  if (int rc = global_xy_tables(ctx, trk)) return rc;
  rl::GlobalXYArgs a;
  a.trk = trk->dev();
  a.span_first = trk->gxy_span.p; a.chunk_first = trk->gxy_chunk.p; a.span_chunk0 = trk->gxy_sch0.p; a.nch = trk->gxy_nch;
  a.bbx = trk->gxy_bbx.p; a.np = trk->n - trk->k;
  a.widths = widths; a.margin = margin; a.lon = lon; a.n_outer = n_outer; a.max_ipm = 80; a.last_as_mid = ctx->global_last_as_mid;
  a.out_ctrl = out_ctrl; a.out_xy = out_xy; a.out_z = out_z; a.out_stats = out_stats;
  const int block = trk->N <= 512 * rl::kXYRows ? 512 : 1024;
  if (trk->N > block * rl::kXYRows) return fail(RL_ERR_UNSUPPORTED, "global QP (dof 2): more than 4096 samples");
  const size_t lds = (size_t)rl::global_xy_layout(trk->k, trk->n, a.np, trk->N, a.nch).total * sizeof(double);
  if (lds > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "global QP (dof 2) does not fit LDS");
  if (stats) { stats->lds_bytes = (int)lds; stats->block_threads = block; stats->rings_in_lds = 0; }
  return by_degree(trk->k, [&](auto kc) {
    constexpr int K = RL_DEGREE(kc);
    return block == 512 ? launch(ctx, rl::k_global_xy<K, 512>, dim3(B), dim3(512), lds, a) : launch(ctx, rl::k_global_xy<K, 1024>, dim3(B), dim3(1024), lds, a);
  });
}

// An empty corridor (w_left + w_right - 2 margin < 0 at a sample) has no feasible line: the kernels run every linearisation to
// its iteration cap and return a line outside, with stats[3] as the only report.  The `_host` entries can read the widths and
// refuse such a batch before anything is staged (the `_dev` entries cannot: there stats[3] is the report).
int corridor_check(const double* widths, int B, int N, double margin) {
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < N; ++i) {
      const double* w = widths + ((size_t)b * N + i) * 2;
      if (w[0] + w[1] - 2.0 * margin < 0.0) {
        char msg[160];
        snprintf(msg, sizeof msg, "empty corridor: instance %d, sample %d has w_left + w_right - 2 margin = %g < 0", b, i,
                 w[0] + w[1] - 2.0 * margin);
        return fail(RL_ERR_ARG, msg);
      }
    }
  return RL_OK;
}

// The two global QPs with host buffers: the same staging around their table builder and their `_common` call.  `opt_width`:
// doubles per free control point of the optional third output (a [B, n-k]: 1, z [B, n-k, 2]: 2).  `weights`: the optional
// second input [B, N] (null: none), refused here like an empty corridor.  The table build stays in front of the timed region.
template <typename Tables, typename Common>
int global_batch_host(rl_ctx* ctx, const rl_track* trk, const double* widths, const double* weights, int B, double margin,
                      int opt_width, double* out_ctrl, double* out_xy, double* out_opt, double* out_stats, rl_stats* stats,
                      Tables tables, Common common) {
  if (!ctx || !trk || !widths || !out_ctrl || !out_stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  const int n = trk->n, N = trk->N;
  for (int b = 0; weights && b < B; ++b)   // before anything is staged or enqueued
    if (!weights_ok(weights + (size_t)b * N, N)) {
      char msg[96];
      snprintf(msg, sizeof msg, "weights of instance %d must be finite and within [2^-30, 2^30]", b);
      return fail(RL_ERR_ARG, msg);
    }
  if (int rc = corridor_check(widths, B, N, margin)) return rc;   // the same
  Staging sg(ctx);
  const double *dw = sg.in(widths, (size_t)B * N * 2), *dwt = sg.in(weights, (size_t)B * N);
  double *dctrl = sg.out(out_ctrl, (size_t)B * n * 2), *dxy = sg.out(out_xy, (size_t)B * N * 2);
  double *dopt = sg.out(out_opt, (size_t)B * (n - trk->k) * opt_width), *dst = sg.out(out_stats, (size_t)B * 8);
  sg.run([&] { return tables(ctx, trk); });
  sg.run_timed([&] { return common(dw, dwt, dctrl, dxy, dopt, dst); });
  return sg.finish(stats);
}

}  // namespace
}  // extern "C++"

int rl_mincurv_global_xy_batch_dev(rl_ctx* ctx, const rl_track* trk, const double* widths, int B, double margin, double lon,
                                   int n_outer, double* out_ctrl, double* out_xy, double* out_z, double* out_stats,
                                   rl_stats* stats) {
  return global_xy_common(ctx, trk, widths, B, margin, lon, n_outer, out_ctrl, out_xy, out_z, out_stats, stats);
}

int rl_mincurv_global_xy_batch_host(rl_ctx* ctx, const rl_track* trk, const double* widths, int B, double margin, double lon,
                                    int n_outer, double* out_ctrl, double* out_xy, double* out_z, double* out_stats,
                                    rl_stats* stats) {
  return global_batch_host(ctx, trk, widths, nullptr, B, margin, 2, out_ctrl, out_xy, out_z, out_stats, stats, global_xy_tables,
                           [&](const double* w, const double*, double* c, double* xy, double* z, double* st) {
                             return global_xy_common(ctx, trk, w, B, margin, lon, n_outer, c, xy, z, st, stats);
                           });
}

int rl_mincurv_global_batch_dev(rl_ctx* ctx, const rl_track* trk, const double* widths, int B,
                                double margin, int n_outer, double* out_ctrl, double* out_xy,
                                double* out_a, double* out_stats, rl_stats* stats) {
  return global_common(ctx, trk, widths, nullptr, B, margin, n_outer, out_ctrl, out_xy, out_a, out_stats, stats);
}

int rl_mincurv_global_batch_host(rl_ctx* ctx, const rl_track* trk, const double* widths, int B,
                                 double margin, int n_outer, double* out_ctrl, double* out_xy,
                                 double* out_a, double* out_stats, rl_stats* stats) {
  return global_batch_host(ctx, trk, widths, nullptr, B, margin, 1, out_ctrl, out_xy, out_a, out_stats, stats, global_tables,
                           [&](const double* w, const double*, double* c, double* xy, double* a, double* st) {
                             return global_common(ctx, trk, w, nullptr, B, margin, n_outer, c, xy, a, st, stats);
                           });
}

int rl_mincurv_global_weighted_batch_dev(rl_ctx* ctx, const rl_track* trk, const double* widths, const double* weights, int B,
                                         double margin, int n_outer, double* out_ctrl, double* out_xy, double* out_a,
                                         double* out_stats, rl_stats* stats) {
  return global_common(ctx, trk, widths, weights, B, margin, n_outer, out_ctrl, out_xy, out_a, out_stats, stats);
}

int rl_mincurv_global_weighted_batch_host(rl_ctx* ctx, const rl_track* trk, const double* widths, const double* weights, int B,
                                          double margin, int n_outer, double* out_ctrl, double* out_xy, double* out_a,
                                          double* out_stats, rl_stats* stats) {
  if (!weights) return rl_mincurv_global_batch_host(ctx, trk, widths, B, margin, n_outer, out_ctrl, out_xy, out_a, out_stats, stats);
  return global_batch_host(ctx, trk, widths, weights, B, margin, 1, out_ctrl, out_xy, out_a, out_stats, stats, global_tables,
                           [&](const double* w, const double* wt, double* c, double* xy, double* a, double* st) {
                             return global_common(ctx, trk, w, wt, B, margin, n_outer, c, xy, a, st, stats);
                           });
}

int rl_mincurv_sweep(rl_ctx* ctx, rl_track* trk, const int* i_start, int max_iter,
                     double* cx, double* cy, double* points, int* n_success, rl_stats* stats) {
  return sweep_single(ctx, trk, i_start, max_iter, cx, cy, points, n_success, stats, false);
}

int rl_mincurv_sweep_joint(rl_ctx* ctx, rl_track* trk, const int* i_start, int max_iter,
                           double* cx, double* cy, double* points, int* n_success, rl_stats* stats) {
  return sweep_single(ctx, trk, i_start, max_iter, cx, cy, points, n_success, stats, true);
}

// ------------------------------------------------------------------------------------------------
// Trajectory.fill_region (csrc/rl_region.hpp)
static int region_check(const double* verts, const int* offsets, int R) {
  if (R > 0 && (!offsets || !verts)) return fail(RL_ERR_ARG, "null argument");
  if (R > 0 && offsets[0] != 0) return fail(RL_ERR_ARG, "region offsets must start at 0");
  for (int r = 0; r < R; ++r)
    if (offsets[r + 1] - offsets[r] < 3) return fail(RL_ERR_ARG, "a region needs at least 3 vertices (bad offsets)");
  return RL_OK;
}

// The region tables (checked by region_check) get their boxes on the host and are staged through the context's arena
// with pageable copies (the runtime has read them when the copy call returns), then one launch of k_region_index.
static int region_launch(rl_ctx* ctx, const double* xy, long long stride, long long n, const double* verts,
                         const int* offsets, int R, const int* codes, int* out, double* tag, long long tag_stride) {
  const int V = offsets[R];
  std::vector<double> box((size_t)4 * R);
  for (int r = 0; r < R; ++r) {
    double x0 = verts[2 * offsets[r]], y0 = verts[2 * offsets[r] + 1], x1 = x0, y1 = y0;
    bool finite = true;
    for (int v = offsets[r]; v < offsets[r + 1]; ++v) {
      const double x = verts[2 * v], y = verts[2 * v + 1];
      finite = finite && std::isfinite(x) && std::isfinite(y);
      x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
    }
    if (!finite) { x0 = y0 = 1.0; x1 = y1 = -1.0; }   // an empty box: the region contains nothing
    box[4 * r] = x0; box[4 * r + 1] = y0; box[4 * r + 2] = x1; box[4 * r + 3] = y1;
  }
  Arena ar(ctx);
  double *dbox = nullptr, *dv = nullptr;
  int *doff = nullptr, *dcode = nullptr;
  RL_HIP(ar.carve([&](Arena& x) {
    dbox = x.take<double>(box.size()); dv = x.take<double>((size_t)2 * V);
    doff = x.take<int>(R + 1); dcode = x.take<int>(R);
  }));
  RL_HIP(hipMemcpyAsync(dbox, box.data(), box.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(hipMemcpyAsync(dv, verts, (size_t)2 * V * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  RL_HIP(hipMemcpyAsync(doff, offsets, (size_t)(R + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (codes) RL_HIP(hipMemcpyAsync(dcode, codes, (size_t)R * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  rl::RegionArgs a;
  a.xy = xy; a.stride = stride; a.n = n;
  a.verts = reinterpret_cast<const double2*>(dv); a.offsets = doff; a.box = reinterpret_cast<const double4*>(dbox); a.R = R;
  a.out = out; a.codes = dcode; a.tag = tag; a.tag_stride = tag_stride;
  RL_TRY(launch(ctx, rl::k_region_index, dim3((unsigned)((n + rl::kRegionBlock - 1) / rl::kRegionBlock)),
                dim3(rl::kRegionBlock), 0, a));
  RL_HIP(ar.end());
  return RL_OK;
}

int rl_fill_region(rl_ctx* ctx, double* points, int B, int N, const double* verts, const int* offsets, int R,
                   const int* codes) {
  if (!ctx) return fail(RL_ERR_ARG, "null argument");
  if (B < 0 || N < 0 || R < 0) return fail(RL_ERR_ARG, "bad sizes");
  if (int rc = region_check(verts, offsets, R)) return rc;
  if (R == 0 || B == 0 || N == 0) return RL_OK;
  if (!points || !codes) return fail(RL_ERR_ARG, "null argument");
  const long long n = (long long)B * N;
  Staging sg(ctx);
  double* dpts = sg.inout(points, (size_t)n * RL_NCOL);
  // REGION is column 8 (models/trajectory.py)
  sg.run([&] { return region_launch(ctx, dpts, RL_NCOL, n, verts, offsets, R, codes, nullptr, dpts + 8, RL_NCOL); });
  return sg.finish();
}

int rl_region_index_dev(rl_ctx* ctx, const double* xy, int B, int N, int stride, const double* verts, const int* offsets,
                        int R, int* out) {
  if (!ctx) return fail(RL_ERR_ARG, "null argument");
  if (B < 0 || N < 0 || R < 0 || stride < 2) return fail(RL_ERR_ARG, "bad sizes");
  if (int rc = region_check(verts, offsets, R)) return rc;
  if (B == 0 || N == 0) return RL_OK;
  if (!xy || !out) return fail(RL_ERR_ARG, "null argument");
  RL_HIP(hipSetDevice(ctx->device));
  const long long n = (long long)B * N;
  if (R == 0) {   // no region contains anything
    RL_HIP(hipMemsetAsync(out, 0xff, (size_t)n * sizeof(int), ctx->stream));
    return RL_OK;
  }
  return region_launch(ctx, xy, stride, n, verts, offsets, R, nullptr, out, nullptr, 0);
}

// The body of rl_qss_sim_dev and rl_qss_sim_vehicles_dev.  per_instance: the five vehicle arrays are DEVICE arrays with a leading
// batch dimension and every workgroup reads its own rows (QssArgs::veh); otherwise small host arrays of one vehicle.
static int qss_sim_enqueue(rl_ctx* ctx, double* points, int B, int N, const double* acc_x, const double* acc_c,
                           int acc_m, const double* dcc_x, const double* dcc_c, int dcc_m, const double* params,
                           int* iters, bool per_instance) {
  if (!ctx || !points || !acc_x || !acc_c || !dcc_x || !dcc_c || !params || !iters)
    return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 2 || acc_m < 1 || dcc_m < 1) return fail(RL_ERR_ARG, "bad sizes");
  if (N >= 65535) return fail(RL_ERR_UNSUPPORTED, "qss: owner indices are 16 bits");
  RL_HIP(hipSetDevice(ctx->device));
  const int cap = 4 * N + 16;
  const size_t lds = ((size_t)2 * N + 5 * (acc_m + dcc_m) + 2) * sizeof(double) + (size_t)rl::kQssStamp * sizeof(int) +
                     (((size_t)N * sizeof(unsigned short) + 7) & ~(size_t)7);  // speed, lon acc, tables, stamp buckets, owner
  if (lds > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "qss: trajectory too long for the LDS-resident profile");
  // The lookup tables are tiny host arrays (scipy CubicSpline pieces).  When they fit they travel BY VALUE in the kernel
  // arguments, so the call is asynchronous and keeps no pointer to caller memory; longer tables are staged through the arena
  // with pageable copies (the runtime then blocks the host until it has read them).
  const int tab_n = (acc_m + 1) + 4 * acc_m + (dcc_m + 1) + 4 * dcc_m;
  const bool by_value = !per_instance && tab_n <= rl::kQssTabMax;
  const bool staged = !per_instance && !by_value;
  Arena ar(ctx);
  double *dax = nullptr, *dac = nullptr, *ddx = nullptr, *ddc = nullptr, *dcst = nullptr;
  int *dfl = nullptr, *dnw = nullptr;
  RL_HIP(ar.carve([&](Arena& x) {
    if (staged) {
      dax = x.take<double>(acc_m + 1); dac = x.take<double>((size_t)4 * acc_m);
      ddx = x.take<double>(dcc_m + 1); ddc = x.take<double>((size_t)4 * dcc_m);
    }
    dfl = x.take<int>((size_t)B * cap * 5); dnw = x.take<int>((size_t)B * cap);
    dcst = x.take<double>((size_t)B * 3 * N);
  }));
  if (staged) {
    RL_HIP(hipMemcpyAsync(dax, acc_x, (acc_m + 1) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    RL_HIP(hipMemcpyAsync(dac, acc_c, (size_t)4 * acc_m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    RL_HIP(hipMemcpyAsync(ddx, dcc_x, (dcc_m + 1) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    RL_HIP(hipMemcpyAsync(ddc, dcc_c, (size_t)4 * dcc_m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  rl::QssArgs a;
  a.points = points; a.B = B; a.N = N;
  a.acc_x = dax; a.acc_c = dac; a.acc_m = acc_m;
  a.dcc_x = ddx; a.dcc_c = ddc; a.dcc_m = dcc_m;
  a.veh = nullptr;
  if (per_instance) {   // the kernels' prologue reads the scalars and the rows of its instance
    a.acc_x = acc_x; a.acc_c = acc_c; a.dcc_x = dcc_x; a.dcc_c = dcc_c; a.veh = params;
    a.max_lon_acc = a.max_lon_dcc = a.max_left_acc = a.max_right_acc = a.max_speed = a.max_jerk = 0.0;
  } else {
    a.max_lon_acc = params[0]; a.max_lon_dcc = params[1]; a.max_left_acc = params[2];
    a.max_right_acc = params[3]; a.max_speed = params[4]; a.max_jerk = params[5];
  }
  a.flags = dfl; a.fresh = dnw; a.cst = dcst; a.cap = cap; a.iters = iters;
  a.tab_n = 0; a.redo = 0; a.dbg = nullptr; a.df_bail_at = ctx->qss_df_bail_at; a.df_report = ctx->qss_df_redo ? 0 : 1;
  if (by_value) {
    double* q = a.tab;
    for (int i = 0; i <= acc_m; ++i) *q++ = acc_x[i];
    for (int i = 0; i < 4 * acc_m; ++i) *q++ = acc_c[i];
    for (int i = 0; i <= dcc_m; ++i) *q++ = dcc_x[i];
    for (int i = 0; i < 4 * dcc_m; ++i) *q++ = dcc_c[i];
    a.tab_n = tab_n;
  }
  // The dataflow kernel takes the sizes its LDS tables hold; what it hands back (iters = -2: front or iteration counts beyond its
  // tables) is re-run by the list-order kernel right behind it, which returns at once for every other instance.
  // Which kernel: the dataflow kernel finishes an instance 2 - 4.5 times sooner but its tables fill the LDS (one instance per CU at
  // N = 2000, three at N = 500), the list-order kernel holds four and more per CU.  Compare the number of ROUNDS the batch
  // takes on the chip (measured, DESIGN_HISTORY.md 3c); RL_QSS_DF=1 / 0 forces one or the other (tests run both).
  bool use_df = rl::df_supported(N, acc_m, dcc_m, (size_t)ctx->max_lds);
  if (use_df) {
    const long long per_cu_df = (long long)((size_t)ctx->max_lds / rl::df_layout(N, acc_m, dcc_m).bytes);
    long long per_cu_list = (long long)((size_t)ctx->max_lds / lds);
    per_cu_list = per_cu_list > 8 ? 8 : per_cu_list;
    const long long cus = ctx->num_cu > 0 ? ctx->num_cu : 1;
    const long long rounds_df = (B + per_cu_df * cus - 1) / (per_cu_df * cus), rounds_list = (B + per_cu_list * cus - 1) / (per_cu_list * cus);
    // a round of the dataflow kernel takes from 1/5 (N = 2000: 29 against 168 ms) to 1/2 (N = 500: 4.4 against 9.3 ms) of a
    // list-order round (DESIGN_HISTORY.md 3c): the ratio the comparison allows grows with N between those two measurements
    const double ratio = N <= 500 ? 2.0 : (N >= 2000 ? 5.0 : 2.0 + 3.0 * (double)(N - 500) / 1500.0);
    use_df = (double)rounds_df <= ratio * (double)rounds_list;
  }
  if (ctx->qss_kernel == 0) use_df = false;
  if (ctx->qss_kernel == 1) use_df = rl::df_supported(N, acc_m, dcc_m, (size_t)ctx->max_lds);
  if (use_df) {
    const size_t lds_df = rl::df_layout(N, acc_m, dcc_m).bytes;
    int* ddbg = nullptr;
#ifdef RL_ABLATION
    if (const char* dbg = getenv("RL_QSS_DEBUG")) if (dbg[0] == '1') { RL_HIP(hipMalloc(&ddbg, (size_t)B * 12 * sizeof(int))); a.dbg = ddbg; }
#endif
    // waves of the (one) workgroup an instance's tables leave room for: four is the fastest at every size measured
    // (DESIGN_HISTORY.md 3c); one and two exist for the tests (rl_ctx_set_option "qss_df_waves")
    RL_TRY(ctx->qss_df_waves == 1   ? launch(ctx, rl::k_qss_dfw<1>, dim3(B), dim3(64), lds_df, a)
           : ctx->qss_df_waves == 2 ? launch(ctx, rl::k_qss_dfw<2>, dim3(B), dim3(128), lds_df, a)
                                    : launch(ctx, rl::k_qss_dfw<4>, dim3(B), dim3(256), lds_df, a));
    if (ddbg) {   // diagnostic build only: synchronous
      std::vector<int> hd((size_t)B * 12);
      RL_HIP(hipStreamSynchronize(ctx->stream));
      const hipError_t ce = hipMemcpy(hd.data(), ddbg, hd.size() * sizeof(int), hipMemcpyDeviceToHost);
      (void)hipFree(ddbg);
      RL_HIP(ce);
      long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int handed = 0;
      for (int i = 0; i < B; ++i) { for (int q = 0; q < 8; ++q) tot[q] += hd[(size_t)i * 12 + q]; handed += hd[(size_t)i * 12 + 7] != 0; }
      fprintf(stderr, "k_qss_dfw: B=%d N=%d lds=%zu  per instance: passes %.0f chunks %.0f examinations %.0f steps %.0f longest queue %.0f numberings %.0f spawned %.0f; handed back %d (reason of instance 0: %d)\n",
              B, N, lds_df, (double)tot[0] / B, (double)tot[1] / B, (double)tot[2] / B, (double)tot[3] / B, (double)tot[4] / B, (double)tot[5] / B, (double)tot[6] / B, handed, hd[7]);
      fprintf(stderr, "k_qss_dfw: thread 0 of instance 0, thousands of clock64 ticks: examination + step %d, records (+ waits) %d, list lane + next agents + wake-ups %d, end of pass %d\n", hd[8], hd[9], hd[10], hd[11]);
      a.dbg = nullptr;
    }
    a.redo = 1;
  }
  // (test hook "qss_df_redo" = 0: what the dataflow kernel handed back stays handed back, iters = RL_QSS_HANDED_BACK - reason)
  if (!use_df || ctx->qss_df_redo) RL_TRY(launch(ctx, rl::k_qss_sim, dim3(B), dim3(64), lds, a));
  RL_HIP(ar.end());
  return RL_OK;
}

int rl_qss_sim_dev(rl_ctx* ctx, double* points, int B, int N, const double* acc_x, const double* acc_c,
                   int acc_m, const double* dcc_x, const double* dcc_c, int dcc_m, const double* params,
                   int* iters) {
  return qss_sim_enqueue(ctx, points, B, N, acc_x, acc_c, acc_m, dcc_x, dcc_c, dcc_m, params, iters, false);
}

int rl_qss_sim_vehicles_dev(rl_ctx* ctx, double* points, int B, int N, const double* acc_x, const double* acc_c,
                            int acc_m, const double* dcc_x, const double* dcc_c, int dcc_m, const double* params,
                            int* iters) {
  return qss_sim_enqueue(ctx, points, B, N, acc_x, acc_c, acc_m, dcc_x, dcc_c, dcc_m, params, iters, true);
}

int rl_qss_sim_vehicles_host(rl_ctx* ctx, double* points, int B, int N, const double* acc_x, const double* acc_c,
                             int acc_m, const double* dcc_x, const double* dcc_c, int dcc_m, const double* params,
                             int* iters) {
  if (!ctx || !points || !acc_x || !acc_c || !dcc_x || !dcc_c || !params || !iters)
    return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 2 || acc_m < 1 || dcc_m < 1) return fail(RL_ERR_ARG, "bad sizes");
  Staging sg(ctx);
  double* dpts = sg.inout(points, (size_t)B * N * RL_NCOL);
  const double* dax = sg.in(acc_x, (size_t)B * (acc_m + 1));
  const double* dac = sg.in(acc_c, (size_t)B * 4 * acc_m);
  const double* ddx = sg.in(dcc_x, (size_t)B * (dcc_m + 1));
  const double* ddc = sg.in(dcc_c, (size_t)B * 4 * dcc_m);
  const double* dpr = sg.in(params, (size_t)B * 6);
  int* dit = sg.out(iters, B);
  sg.run([&] { return rl_qss_sim_vehicles_dev(ctx, dpts, B, N, dax, dac, acc_m, ddx, ddc, dcc_m, dpr, dit); });
  return sg.finish();
}

int rl_qss_sim(rl_ctx* ctx, double* points, int B, int N, const double* acc_x, const double* acc_c,
               int acc_m, const double* dcc_x, const double* dcc_c, int dcc_m, const double* params,
               int* iters) {
  if (!ctx || !points || !iters) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 2) return fail(RL_ERR_ARG, "bad sizes");
  Staging sg(ctx);
  double* dpts = sg.inout(points, (size_t)B * N * RL_NCOL);
  int* dit = sg.out(iters, B);
  sg.run([&] { return rl_qss_sim_dev(ctx, dpts, B, N, acc_x, acc_c, acc_m, dcc_x, dcc_c, dcc_m, params, dit); });
  return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// tables of a solved batch and their summary (csrc/rl_tables.hpp)
int rl_tables_batch_dev(rl_ctx* ctx, const rl_track* trk, const double* ctrl, int B, int bounds_form, const double* bounds,
                        double length, const double* bank, int bank_per_instance, double* points) {
  if (!ctx || !trk || !ctrl || !points) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  if (!degree_supported(trk->k)) return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
  const int n = trk->n, N = trk->N, k = trk->k;
  rl::TablesArgs a;
  std::memset(&a, 0, sizeof(a));
  a.ctrl = ctrl; a.B = B; a.form = bounds_form; a.in = bounds;
  Bounds bd;
  if (int rc = resolve_bounds(trk, bounds_form, bounds, bd)) return rc;
  a.ringL = bd.ringL; a.ringR = bd.ringR; a.nL = bd.nL; a.nR = bd.nR;
  RL_HIP(hipSetDevice(ctx->device));
  // width-form rings in the arithmetic the sweep of this context builds them with: the reference-order tables where that
  // arithmetic exists (degree 5) and was not switched off, the fast tables elsewhere
  if (bounds_form == RL_BOUNDS_WIDTHS && k == 5 && ctx->arith != RL_ARITH_FAST) {
    if (int rc = ensure_strict_tables(ctx, trk)) return rc;
    a.strict_rings = 1;
  }
  a.tr = trk->dev();
  a.search = ctx->tables_search;
  a.max_dist = 100.0;   // race_track.py:104
  a.length = length;
  a.bank = bank; a.bank_per_instance = bank_per_instance;
  a.points = points;
  bool rings_lds = !ctx->tables_rings_global;
  size_t lds = rl::tables_lds_layout(trk->nt, n, N, a.nL, a.nR, true).total * sizeof(double);
  if (lds > (size_t)ctx->max_lds) rings_lds = false;
  if (!rings_lds) lds = rl::tables_lds_layout(trk->nt, n, N, a.nL, a.nR, false).total * sizeof(double);
  if (lds > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "tables: the instance does not fit LDS");
  Arena ar(ctx);
  if (!rings_lds) {
    a.gscratch_stride = rl::tables_ring_scratch_doubles(a.nL, a.nR);
    RL_HIP(ar.carve([&](Arena& x) { a.gscratch = x.take<double>(a.gscratch_stride * (size_t)B); }));
  }
  RL_TRY(by_degree(k, [&](auto kc) {
    constexpr int K = RL_DEGREE(kc);
    const dim3 grid(B), block(rl::kTablesThreads);
    return rings_lds ? launch(ctx, rl::k_tables<K, true>, grid, block, lds, a) : launch(ctx, rl::k_tables<K, false>, grid, block, lds, a);
  }));
  if (!rings_lds) RL_HIP(ar.end());
  return RL_OK;
}

int rl_tables_batch_host(rl_ctx* ctx, const rl_track* trk, const double* ctrl, int B, int bounds_form, const double* bounds,
                         double length, const double* bank, int bank_per_instance, double* points) {
  if (!ctx || !trk || !ctrl || !points) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0) return fail(RL_ERR_ARG, "B <= 0");
  const int cols = bounds_cols(bounds_form);
  if (cols && !bounds) return fail(RL_ERR_ARG, "bounds input is null");
  const int n = trk->n, N = trk->N;
  Staging sg(ctx);
  const double* dctrl = sg.in(ctrl, (size_t)B * n * 2);
  double* dpts = sg.out(points, (size_t)B * N * RL_NCOL);
  const double* din = cols ? sg.in(bounds, (size_t)B * N * cols) : nullptr;
  const double* dbank = sg.in(bank, (size_t)(bank_per_instance ? B : 1) * N);
  sg.run([&] { return rl_tables_batch_dev(ctx, trk, dctrl, B, bounds_form, din, length, dbank, bank_per_instance, dpts); });
  return sg.finish();
}

// tables of a batch of poses: the tail of the reference's min-time pipeline (csrc/rl_pose_tables.hpp)
static int pose_tables_check(const rl_ctx* ctx, const rl_track* trk, int form, const double* X, int B, int N, const double* ss,
                             const double* cxs, const double* cys, int M, int bounds_form, const double* bounds,
                             const double* points) {
  if (!ctx || !trk || !X || !points) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 2) return fail(RL_ERR_ARG, "bad sizes");
  if (form != RL_POSE_FRENET && form != RL_POSE_GLOBAL) return fail(RL_ERR_ARG, "bad pose form");
  if (form == RL_POSE_FRENET && (!ss || !cxs || !cys || M < 1)) return fail(RL_ERR_ARG, "RL_POSE_FRENET needs the centre line's pieces");
  if (bounds_form != RL_BOUNDS_SHARED_RINGS && bounds_form != RL_BOUNDS_WIDTHS && bounds_form != RL_BOUNDS_POINTS)
    return fail(RL_ERR_ARG, "bad bounds_form");
  if (bounds_cols(bounds_form) && !bounds) return fail(RL_ERR_ARG, "bounds input is null");
  return RL_OK;
}

int rl_pose_tables_batch_dev(rl_ctx* ctx, const rl_track* trk, int form, const double* X, int B, int N, const double* ss,
                             const double* cxs, const double* cys, int M, int bounds_form, const double* bounds,
                             const double* base, int base_per_instance, const double* T, double* points) {
  RL_TRY(pose_tables_check(ctx, trk, form, X, B, N, ss, cxs, cys, M, bounds_form, bounds, points));
  rl::PoseTablesArgs a;
  std::memset(&a, 0, sizeof(a));
  a.form = form; a.X = X; a.B = B; a.N = N;
  a.ss = ss; a.cxs = cxs; a.cys = cys; a.M = M;
  a.bounds_form = bounds_form; a.in = bounds;
  Bounds bd;
  if (int rc = resolve_bounds(trk, bounds_form, bounds, bd)) return rc;
  a.ringL = bd.ringL; a.ringR = bd.ringR; a.nL = bd.nL; a.nR = bd.nR;
  RL_HIP(hipSetDevice(ctx->device));
  if (bounds_form == RL_BOUNDS_WIDTHS) {   // the rings rl_tables_batch_dev builds from the same widths
    if (!degree_supported(trk->k)) return fail(RL_ERR_UNSUPPORTED, "spline degree must be 3 or 5");
    if (trk->k == 5 && ctx->arith != RL_ARITH_FAST) {
      if (int rc = ensure_strict_tables(ctx, trk)) return rc;
      a.strict_rings = 1;
    }
  }
  a.tr = trk->dev();
  a.search = ctx->tables_search;
  a.max_dist = 100.0;   // race_track.py: fill_trajectory_boundaries
  a.base = base; a.base_per_instance = base_per_instance;
  a.T = T;
  a.points = points;
  bool rings_lds = !ctx->tables_rings_global;
  size_t lds = rl::pose_lds_layout(N, a.nL, a.nR, true).total * sizeof(double);
  if (lds > (size_t)ctx->max_lds) rings_lds = false;
  if (!rings_lds) lds = rl::pose_lds_layout(N, a.nL, a.nR, false).total * sizeof(double);
  if (lds > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "pose tables: the instance's poses do not fit LDS");
  Arena ar(ctx);
  if (!rings_lds) {
    a.gscratch_stride = rl::tables_ring_scratch_doubles(a.nL, a.nR);
    RL_HIP(ar.carve([&](Arena& x) { a.gscratch = x.take<double>(a.gscratch_stride * (size_t)B); }));
  }
  const dim3 grid(B), block(rl::kTablesThreads);
  RL_TRY(rings_lds ? launch(ctx, rl::k_pose_tables<true>, grid, block, lds, a) : launch(ctx, rl::k_pose_tables<false>, grid, block, lds, a));
  if (!rings_lds) RL_HIP(ar.end());
  return RL_OK;
}

int rl_pose_tables_batch_host(rl_ctx* ctx, const rl_track* trk, int form, const double* X, int B, int N, const double* ss,
                              const double* cxs, const double* cys, int M, int bounds_form, const double* bounds,
                              const double* base, int base_per_instance, const double* T, double* points) {
  RL_TRY(pose_tables_check(ctx, trk, form, X, B, N, ss, cxs, cys, M, bounds_form, bounds, points));
  const int cols = bounds_cols(bounds_form);
  const bool frenet = form == RL_POSE_FRENET;
  Staging sg(ctx);
  const double* dX = sg.in(X, (size_t)B * N * (frenet ? 6 : 5));
  const double* dss = frenet ? sg.in(ss, (size_t)M + 1) : nullptr;
  const double* dcx = frenet ? sg.in(cxs, (size_t)4 * M) : nullptr;
  const double* dcy = frenet ? sg.in(cys, (size_t)4 * M) : nullptr;
  const double* din = cols ? sg.in(bounds, (size_t)B * trk->N * cols) : nullptr;
  const double* dbase = sg.in(base, (size_t)(base_per_instance ? B : 1) * N * RL_NCOL);
  const double* dT = sg.in(T, (size_t)B * N);
  double* dpts = sg.out(points, (size_t)B * N * RL_NCOL);
  sg.run([&] {
    return rl_pose_tables_batch_dev(ctx, trk, form, dX, B, N, dss, dcx, dcy, M, bounds_form, din, dbase, base_per_instance, dT, dpts);
  });
  return sg.finish();
}

// ---- global -> Frenet: projection of lines onto the centre line, and their coordinates at node abscissae (rl_frenet.hpp)
static int frenet_check(const rl_ctx* ctx, const double* points, int B, int P, int stride, const double* ss, const double* cxs,
                        const double* cys, int M, const double* out, size_t& lds_bytes) {
  if (!ctx || !points || !ss || !cxs || !cys || !out) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || P < 1) return fail(RL_ERR_ARG, "frenet: B >= 1 and P >= 1");
  if (M < 3) return fail(RL_ERR_ARG, "frenet: at least 3 pieces");
  if (stride != 2 && stride != RL_NCOL) return fail(RL_ERR_ARG, "frenet: stride 2 (points) or 19 (tables)");
  lds_bytes = rl::frenet_lds_layout(M).total_bytes;
  if (lds_bytes > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "frenet: the table of the pieces does not fit LDS");
  return RL_OK;
}

int rl_frenet_batch_dev(rl_ctx* ctx, const double* points, int B, int P, int stride, const double* yaw, const double* ss,
                        const double* cxs, const double* cys, int M, double* out, int* status, double* stats) {
  size_t lds = 0;
  RL_TRY(frenet_check(ctx, points, B, P, stride, ss, cxs, cys, M, out, lds));
  RL_HIP(hipSetDevice(ctx->device));
  rl::FrenetArgs a;
  a.points = points; a.B = B; a.P = P; a.stride = stride; a.yaw = yaw;
  a.ss = ss; a.cxs = cxs; a.cys = cys; a.M = M;
  a.search = ctx->frenet_search;
  a.out = out; a.status = status; a.stats = stats;
  return launch(ctx, rl::k_frenet, dim3(B), dim3(rl::kFrenetThreads), lds, a);
}

int rl_frenet_batch_host(rl_ctx* ctx, const double* points, int B, int P, int stride, const double* yaw, const double* ss,
                         const double* cxs, const double* cys, int M, double* out, int* status, double* stats) {
  size_t lds = 0;
  RL_TRY(frenet_check(ctx, points, B, P, stride, ss, cxs, cys, M, out, lds));
  Staging sg(ctx);
  const double* dpts = sg.in(points, (size_t)B * P * stride);
  const double* dyaw = sg.in(yaw, (size_t)B * P);
  const double* dss = sg.in(ss, (size_t)M + 1);
  const double* dcx = sg.in(cxs, (size_t)4 * M);
  const double* dcy = sg.in(cys, (size_t)4 * M);
  double* dout = sg.out(out, (size_t)B * P * 4);
  int* dst = sg.out(status, (size_t)B * P);
  double* dstats = sg.out(stats, (size_t)B * 4);
  sg.run([&] { return rl_frenet_batch_dev(ctx, dpts, B, P, stride, dyaw, dss, dcx, dcy, M, dout, dst, dstats); });
  return sg.finish();
}

static int frenet_resample_check(const rl_ctx* ctx, const double* fr, int C, int B, int P, const double* s_nodes, int Nn, double L,
                                 const double* out, const int* status) {
  if (!ctx || !fr || !s_nodes || !out || !status) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || P < 1 || Nn < 1 || C < 0) return fail(RL_ERR_ARG, "frenet resample: B >= 1, P >= 1, Nn >= 1, C >= 0");
  if (!(L > 0.0)) return fail(RL_ERR_ARG, "frenet resample: the track length must be positive");
  return RL_OK;
}

int rl_frenet_resample_dev(rl_ctx* ctx, const double* fr, const double* vals, int C, int B, int P, const double* s_nodes, int Nn,
                           double L, double* out, int* status) {
  RL_TRY(frenet_resample_check(ctx, fr, C, B, P, s_nodes, Nn, L, out, status));
  if (C > 0 && !vals) return fail(RL_ERR_ARG, "frenet resample: C channels without vals");
  RL_HIP(hipSetDevice(ctx->device));
  return launch(ctx, rl::k_frenet_resample, dim3(B), dim3(rl::kResampleThreads), (size_t)16, fr, vals, C, P, s_nodes, Nn, L, out, status);
}

int rl_frenet_resample_host(rl_ctx* ctx, const double* fr, const double* vals, int C, int B, int P, const double* s_nodes, int Nn,
                            double L, double* out, int* status) {
  RL_TRY(frenet_resample_check(ctx, fr, C, B, P, s_nodes, Nn, L, out, status));
  if (C > 0 && !vals) return fail(RL_ERR_ARG, "frenet resample: C channels without vals");
  Staging sg(ctx);
  const double* dfr = sg.in(fr, (size_t)B * P * 4);
  const double* dvals = C > 0 ? sg.in(vals, (size_t)B * P * C) : nullptr;
  const double* dnodes = sg.in(s_nodes, (size_t)Nn);
  double* dout = sg.out(out, (size_t)B * Nn * (2 + C));
  int* dst = sg.out(status, (size_t)B);
  sg.run([&] { return rl_frenet_resample_dev(ctx, dfr, dvals, C, B, P, dnodes, Nn, L, dout, dst); });
  return sg.finish();
}

int rl_table_summary_dev(rl_ctx* ctx, const double* points, int B, int N, const int* iters, double* out) {
  if (!ctx || !points || !out) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N <= 0) return fail(RL_ERR_ARG, "bad sizes");
  const size_t lds = (size_t)N * sizeof(double);
  if (lds > (size_t)ctx->max_lds) return fail(RL_ERR_UNSUPPORTED, "table summary: trajectory too long for the LDS-resident TIME column");
  RL_HIP(hipSetDevice(ctx->device));
  return launch(ctx, rl::k_table_summary, dim3(B), dim3(rl::kWave), lds, points, N, iters, out);
}

int rl_table_summary_host(rl_ctx* ctx, const double* points, int B, int N, const int* iters, double* out) {
  if (!ctx || !points || !out) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N <= 0) return fail(RL_ERR_ARG, "bad sizes");
  Staging sg(ctx);
  const double* dpts = sg.in(points, (size_t)B * N * RL_NCOL);
  double* dout = sg.out(out, (size_t)B * 8);
  const int* dit = sg.in(iters, B);
  sg.run([&] { return rl_table_summary_dev(ctx, dpts, B, N, dit, dout); });
  return sg.finish();
}

// rl_dt_eval_nodes / rl_dt_eval_jac: the checks of what they share, then its staging and the DtArgs fill
static int dt_check(const rl_ctx* ctx, const double* model, int B, int N, const double* s, const double* kappa, const double* left,
                    const double* right, double track_length, const double* X, const double* U, const double* T, bool outputs) {
  static_assert((int)RL_DT_NPARAM == (int)rl::DT_NPARAM, "parameter tables out of step");
  if (!ctx || !model || !s || !kappa || !left || !right || !X || !U || !T || !outputs) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 2 || !(track_length > 0.0)) return fail(RL_ERR_ARG, "bad sizes");
  return RL_OK;
}

static rl::DtArgs dt_stage(Staging& sg, const double* model, int B, int N, const double* s, const double* kappa, const double* left,
                           const double* right, double margin, double track_length, const double* X, const double* U,
                           const double* T) {
  const size_t bn = (size_t)B * N;
  rl::DtArgs a;
  for (int i = 0; i < rl::DT_NPARAM; ++i) a.p[i] = model[i];
  a.B = B; a.N = N; a.margin = margin; a.track_length = track_length;
  a.s = sg.in(s, N); a.kappa = sg.in(kappa, N); a.left = sg.in(left, N); a.right = sg.in(right, N);
  a.X = sg.in(X, bn * 6); a.U = sg.in(U, bn * 4); a.T = sg.in(T, bn);
  a.eq = nullptr; a.ineq = nullptr; a.cost_part = nullptr;
  return a;
}

int rl_dt_eval_nodes(rl_ctx* ctx, const double* model, int B, int N, const double* s, const double* kappa,
                     const double* left, const double* right, double margin, double track_length,
                     const double* X, const double* U, const double* T, double* eq, double* ineq,
                     double* cost) {
  if (int rc = dt_check(ctx, model, B, N, s, kappa, left, right, track_length, X, U, T, eq && ineq && cost)) return rc;
  const size_t bn = (size_t)B * N;
  std::vector<double> part(bn);
  Staging sg(ctx);
  rl::DtArgs a = dt_stage(sg, model, B, N, s, kappa, left, right, margin, track_length, X, U, T);
  a.eq = sg.out(eq, bn * rl::kDtNeq); a.ineq = sg.out(ineq, bn * rl::kDtNineq); a.cost_part = sg.out(part.data(), bn);
  sg.run([&] { return launch(ctx, rl::k_dt_eval_nodes, dim3((N + 127) / 128, B), dim3(128), 0, a); });
  if (int rc = sg.finish()) return rc;
  for (int b = 0; b < B; ++b) {  // the objective is a plain sum over the nodes, in node order
    double c = 0.0;
    for (int j = 0; j < N; ++j) c += part[(size_t)b * N + j];
    cost[b] = c;
  }
  return RL_OK;
}

int rl_dt_eval_jac(rl_ctx* ctx, const double* model, int B, int N, const double* s, const double* kappa,
                   const double* left, const double* right, double margin, double track_length,
                   const double* X, const double* U, const double* T, double* jac_eq, double* jac_ineq,
                   double* grad_cost) {
  if (int rc = dt_check(ctx, model, B, N, s, kappa, left, right, track_length, X, U, T, jac_eq && jac_ineq && grad_cost)) return rc;
  const size_t bn = (size_t)B * N;
  Staging sg(ctx);
  rl::DtJacArgs ja;
  ja.f = dt_stage(sg, model, B, N, s, kappa, left, right, margin, track_length, X, U, T);
  ja.jac_eq = sg.out(jac_eq, bn * rl::kDtNeq * rl::kDtNvar); ja.jac_ineq = sg.out(jac_ineq, bn * rl::kDtNineq * rl::kDtNvar);
  ja.grad_cost = sg.out(grad_cost, bn * rl::kDtNvar);
  const int slices = (rl::kDtNvar + rl::kDtJacND - 1) / rl::kDtJacND;
  sg.run([&] { return launch(ctx, rl::k_dt_eval_jac, dim3((N + 127) / 128, B, slices), dim3(128), 0, ja); });
  return sg.finish();
}

// ---- the min-time double-track NLP (rl_mintime.hpp)
// One text of the driver for the three problem types (rl_mintime.hpp: <MtProblem> shared model, <MtProblemV> one vehicle, <MtProblemT>
// one centre line per instance as well): the bit-equality of the forms rests on the launch sequences being the same.
namespace {
extern "C++" {
// A sub-batch: its stream, its two views of the problem, the state and the caller's arrays, the grids most kernels share (y: the
// instance).  P goes to the kernels that never read the model, M to the <PT> instance of the ones that do; for PT = MtProblem the two are
// equal.  In a table call M carries the group's slice of the table and P.p / sw / se are NaN: a kernel that read them would not go unnoticed.
template <typename PT> struct MtGroup { hipStream_t q; rl::MtProblem P; PT M; rl::MtState st; double *X, *U, *T, *stats; dim3 rows, per_node, per_inst; };
// M from the group's P and its slice of the table (row0: the row of the group's first instance), as of left / right
inline void mt_set_model(rl::MtProblem& M, const rl::MtProblem& P, const double*) { M = P; }
template <typename PT> void mt_set_model(PT& M, const rl::MtProblem& P, const double* row0) {
  M.p = (rl::MtTab)row0; M.sw = (rl::MtTab)(row0 + rl::kMtRowSw); M.se = (rl::MtTab)(row0 + rl::kMtRowSe);
  M.N = P.N; M.s = P.s; M.kappa = P.kappa; M.left = P.left; M.right = P.right;
  M.bounds_per_instance = P.bounds_per_instance; M.margin = P.margin; M.track_length = P.track_length;
}

// a launch on the group's stream: of a kernel that never reads the model, of one that does, of the two that also take the caller's arrays
template <typename PT> int mt_run(const rl_ctx* ctx, const MtGroup<PT>& G, void (*kernel)(rl::MtProblem, rl::MtState), dim3 grid, int threads) { return launch(ctx, G.q, kernel, grid, dim3(threads), 0, G.P, G.st); }
template <typename PT> int mt_run_model(const rl_ctx* ctx, const MtGroup<PT>& G, void (*kernel)(PT, rl::MtState), dim3 grid, int threads) { return launch(ctx, G.q, kernel, grid, dim3(threads), 0, G.M, G.st); }
template <typename PT> int mt_pack(const rl_ctx* ctx, const MtGroup<PT>& G) { return launch(ctx, G.q, rl::k_mt_pack<PT>, G.rows, dim3(64), 0, G.M, G.st, G.X, G.U, G.T); }
template <typename PT> int mt_unpack(const rl_ctx* ctx, const MtGroup<PT>& G) { return launch(ctx, G.q, rl::k_mt_unpack<PT>, G.rows, dim3(64), 0, G.M, G.st, G.X, G.U, G.T); }

// One iteration of one group on its stream; finished instances return at once from every kernel.  Three pipelines: the
// default (k_mt_node), and the cross-checks RL_MT_HES_SWEEP=1 / RL_MT_UNFUSED=1 with the separate assembly kernels.
template <typename PT> int mt_enqueue_iteration(const rl_ctx* ctx, const MtGroup<PT>& G) {
  const int N = G.P.N, nb = G.st.B;
  if (ctx->mt_hes_sweep) {   // cross-check: forward (over forward) duals through the whole pair function
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_derivs<0, PT>, G.rows, 64));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_derivs<1, PT>, dim3(G.rows.x, nb, rl::kMtJacSlices), 64));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_derivs<2, PT>, dim3(G.rows.x, nb, rl::kMtHesSlices), 64));
  } else {
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_values<PT>, G.rows, 64));   // functions; values of the dynamics at the two ends -> midpoint
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_jac_dirs<PT>, dim3(rl::mt_jac_blocks(N), nb, 3), 64));
    if (ctx->mt_unfused) RL_TRY(mt_run_model(ctx, G, rl::k_mt_jac_assemble<PT>, G.per_node, 64));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_hes_point<0, PT>, dim3(rl::mt_hes_blocks(N), nb, 1), 64));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_hes_point<1, PT>, dim3(rl::mt_hes_blocks(N), nb, 2), 64));
    if (ctx->mt_unfused) {
      RL_TRY(mt_run_model(ctx, G, rl::k_mt_hes_assemble<PT>, G.per_node, 64));
    } else {   // Jacobian, Hessian, blocks and right-hand side in one pass over the pairs
      RL_TRY(mt_run_model(ctx, G, rl::k_mt_node<PT>, dim3(rl::mt_node_blocks(N), nb), 64));
      RL_TRY(mt_run_model(ctx, G, rl::k_mt_prepare2<PT>, G.per_inst, 256));
    }
  }
  if (ctx->mt_hes_sweep || ctx->mt_unfused) {
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_prepare<PT>, G.per_inst, 64));
    RL_TRY(mt_run(ctx, G, rl::k_mt_assemble, G.per_node, 64));
    RL_TRY(mt_run(ctx, G, rl::k_mt_gc_pack, G.per_node, 64));
  }
  if (ctx->mt_kkt4 && N >= 64) RL_TRY(mt_run(ctx, G, rl::k_mt_kkt4, G.per_inst, 256));
  else RL_TRY(mt_run(ctx, G, rl::k_mt_kkt, G.per_inst, 128));
  RL_TRY(mt_run(ctx, G, rl::k_mt_dir, dim3(rl::kMtDirBlocks(N), nb), 64));
  RL_TRY(mt_run_model(ctx, G, rl::k_mt_trial<PT>, G.rows, 64));
  RL_TRY(mt_run(ctx, G, rl::k_mt_step, G.per_inst, 256));
  RL_TRY(mt_run_model(ctx, G, rl::k_mt_trial_b<PT>, G.rows, 64));        // halvings of the instances whose first trial point was rejected
  return mt_run_model(ctx, G, rl::k_mt_step_b<PT>, G.per_inst, 256);
}

// the closing pass of one group: final residuals of the instances still running (status 0 = iteration limit), the caller's arrays, the report
template <typename PT> int mt_enqueue_closing(const rl_ctx* ctx, const MtGroup<PT>& G) {
  const int N = G.P.N, nb = G.st.B;
  RL_TRY(mt_run_model(ctx, G, rl::k_mt_derivs<0, PT>, G.rows, 64));
  if (ctx->mt_hes_sweep) {
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_derivs<1, PT>, dim3(G.rows.x, nb, rl::kMtJacSlices), 64));
  } else {
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_hes_values<PT>, G.rows, 64));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_jac_dirs<PT>, dim3(rl::mt_jac_blocks(N), nb, 3), 64));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_jac_assemble<PT>, G.per_node, 64));
  }
  RL_TRY(mt_run_model(ctx, G, rl::k_mt_residuals<PT>, G.per_inst, 64));
  RL_TRY(mt_unpack(ctx, G));
  return launch(ctx, G.q, rl::k_mt_stats, dim3((nb + 63) / 64), dim3(64), 0, G.st, G.stats);
}
}  // extern "C++"

// min_time_optimizer.py:109-113: scale_x = (1, average_track_width, 1, 1, 0.5, speed_cap),
// scale_u = (Fd_max, |Fb_max|, delta_max, 50 mass), scale_t = 1  ->  sw [9], se [7] of one model (MtProblem).  The one
// statement of the scales: the shared-model call and every row of a vehicles call go through it.
void mt_scales(const double* model, double average_track_width, double speed_cap, double* sw, double* se) {
  const double sx[6] = {1.0, average_track_width, 1.0, 1.0, 0.5, speed_cap};
  const double su[4] = {model[RL_DT_FD_MAX], std::fabs(model[RL_DT_FB_MAX]), model[RL_DT_DELTA_MAX], model[RL_DT_MASS] * 50.0};
  for (int c = 0; c < 5; ++c) sw[c] = sx[1 + c];
  sw[5] = su[0]; sw[6] = su[2]; sw[7] = su[3]; sw[8] = 1.0;
  for (int c = 0; c < 6; ++c) se[c] = 1.0 / sx[c];
  se[6] = 1.0 / su[3];
}

// a vehicles call checks every row before anything is enqueued: what the scales divide by and what the rows of the NLP divide by
int mt_check_models(const double* models, int B) {
  static const struct { int slot; const char* name; } positive[] = {
      {RL_DT_FD_MAX, "Fd_max"}, {RL_DT_DELTA_MAX, "delta_max"}, {RL_DT_MASS, "mass"}, {RL_DT_PMAX, "Pmax"}, {RL_DT_MU, "mu"},
      {RL_DT_TD, "Td"}, {RL_DT_TB, "Tb"}, {RL_DT_TDELTA, "Tdelta"}};
  for (int b = 0; b < B; ++b) {
    const double* m = models + (size_t)b * RL_DT_NPARAM;
    for (int i = 0; i < RL_DT_NPARAM; ++i)
      if (!std::isfinite(m[i])) return fail(RL_ERR_ARG, "models: instance " + std::to_string(b) + ": parameter " + std::to_string(i) + " is not finite");
    if (!(std::fabs(m[RL_DT_FB_MAX]) > 0.0)) return fail(RL_ERR_ARG, "models: instance " + std::to_string(b) + ": |Fb_max| must be > 0");
    for (const auto& q : positive)
      if (!(m[q.slot] > 0.0)) return fail(RL_ERR_ARG, "models: instance " + std::to_string(b) + ": " + q.name + " must be > 0");
  }
  return RL_OK;
}

// What a tracks call (rl_mintime_solve_tracks*) has per track or per instance, all HOST arrays: checked by mt_check_tracks.
struct MtTracks { int T; const int* track_of; const double *track_length, *average_track_width, *speed_cap; };

// One call of any of the six entries, as its entry filled it: mt_check_call refuses what is wrong with it, the driver reads it.
// The form of the solve follows from it: a tracks call and a call with B model rows take the model from a table (mt_build_rows).
struct MtCall {
  const double* model; bool model_rows;   // HOST: one row [RL_DT_NPARAM] for all instances, or B rows
  int B, N; const double *s, *kappa, *left, *right; int bounds_per_instance; double margin;
  double *X, *U, *T, *stats; int max_iter; double tol;
  // one centre line for all instances: its three scalars -- or a tracks call: s, kappa are [T,N] and the scalars stay NaN
  static constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();
  double track_length = kNaN, average_track_width = kNaN, speed_cap = kNaN;
  const MtTracks* tr = nullptr;
  bool poll = false;   // stop enqueueing once every instance has finished (the host entries, which synchronise anyway)
  bool table() const { return tr || model_rows; }
};

int mt_check_tracks(const MtTracks& tr, const double* models, bool model_rows, int B) {
  if (tr.T <= 0 || !tr.track_length || !tr.average_track_width || !tr.speed_cap) return fail(RL_ERR_ARG, "tracks: T >= 1 and the three arrays [T]");
  if (!tr.track_of && tr.T != B) return fail(RL_ERR_ARG, "track_of: NULL is the identity and needs T == B");
  RL_TRY(mt_check_models(models, model_rows ? B : 1));
  for (int b = 0; tr.track_of && b < B; ++b)
    if (tr.track_of[b] < 0 || tr.track_of[b] >= tr.T)
      return fail(RL_ERR_ARG, "track_of: instance " + std::to_string(b) + ": track " + std::to_string(tr.track_of[b]) + " outside [0, " + std::to_string(tr.T) + ")");
  for (int t = 0; t < tr.T; ++t) {
    const struct { const double* v; const char* name; } positive[] = {
        {tr.track_length, "track_length"}, {tr.average_track_width, "average_track_width"}, {tr.speed_cap, "speed_cap"}};
    for (const auto& q : positive)
      if (!std::isfinite(q.v[t]) || !(q.v[t] > 0.0)) return fail(RL_ERR_ARG, "tracks: track " + std::to_string(t) + ": " + q.name + " must be finite and > 0");
  }
  return RL_OK;
}

// The table of a vehicles or a tracks call: row b = p | sw | se of instance b, and in a tracks call the length and the index
// of its track (rl_mintime.hpp: kMtRowLen, kMtRowTrack).  `rows` [B, kMtRow] arrives zeroed; the call is checked.
void mt_build_rows(double* rows, const MtCall& c) {
  const MtTracks* tr = c.tr;
  for (int b = 0; b < c.B; ++b) {
    const double* m = c.model + (c.model_rows ? (size_t)b * RL_DT_NPARAM : 0);
    double* r = rows + (size_t)b * rl::kMtRow;
    for (int i = 0; i < rl::DT_NPARAM; ++i) r[i] = m[i];
    if (tr) {   // the instance's track: its scales, its length, its index (an int in the low word of the slot)
      const int t = tr->track_of ? tr->track_of[b] : b;
      mt_scales(m, tr->average_track_width[t], tr->speed_cap[t], r + rl::kMtRowSw, r + rl::kMtRowSe);
      r[rl::kMtRowLen] = tr->track_length[t];
      std::memcpy(r + rl::kMtRowTrack, &t, sizeof(int));
    } else {
      mt_scales(m, c.average_track_width, c.speed_cap, r + rl::kMtRowSw, r + rl::kMtRowSe);
    }
  }
}

// The one check of a call, before anything is staged or enqueued.  mt_check_table: the rows a table is built from, also what
// rl_debug_mt_rows checks.  host_arrays: s, kappa, left, right can be read here, so the host entries also look at them.
int mt_check_table(const MtCall& c) {
  if (c.tr) return mt_check_tracks(*c.tr, c.model, c.model_rows, c.B);
  return c.model_rows ? mt_check_models(c.model, c.B) : RL_OK;
}
int mt_check_call(const rl_ctx* ctx, const MtCall& c, bool host_arrays) {
  if (!ctx || !c.model || !c.s || !c.kappa || !c.left || !c.right || !c.X || !c.U || !c.T || !c.stats) return fail(RL_ERR_ARG, "null argument");
  if (c.B <= 0 || c.N < 8 || !(c.tr || c.track_length > 0.0) || c.max_iter < 1 || !(c.tol > 0.0)) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes)");
  if (!c.tr && (!(c.average_track_width > 0.0) || !(c.speed_cap > 0.0))) return fail(RL_ERR_ARG, "bad scales");
  RL_TRY(mt_check_table(c));
  if (!host_arrays) return RL_OK;
  const int N = c.N;
  for (int t = 0; c.tr && t < c.tr->T; ++t) {
    const double *st = c.s + (size_t)t * N, *kt = c.kappa + (size_t)t * N;
    for (int j = 0; j < N; ++j) {
      if (!std::isfinite(kt[j])) return fail(RL_ERR_ARG, "tracks: track " + std::to_string(t) + ": kappa is not finite at node " + std::to_string(j));
      if (!(st[j] >= 0.0 && st[j] < c.tr->track_length[t] && (j == 0 || st[j] > st[j - 1])))
        return fail(RL_ERR_ARG, "tracks: track " + std::to_string(t) + ": s must increase strictly within [0, track_length) (node " + std::to_string(j) + ")");
    }
  }
  const size_t nb_ = c.bounds_per_instance ? (size_t)c.B * N : (size_t)N;
  for (size_t i = 0; i < nb_; ++i)
    if (!(c.right[i] + c.margin < c.left[i] - c.margin)) return fail(RL_ERR_ARG, "track narrower than the vehicle plus margins (min_time_optimizer.py:135)");
  return RL_OK;
}

// The solve of a checked call on device pointers, for one problem type.  P: the problem as the model-blind kernels take it;
// rows: the table [B, kMtRow] of a table call, else empty.  With c.poll the call stops enqueueing once every instance has
// finished; without it all max_iter iterations are enqueued and the call does not wait.
extern "C++" {
template <typename PT> int mt_solve_as(rl_ctx* ctx, const MtCall& c, const rl::MtProblem& P, const std::vector<double>& rows) {
  const int B = c.B, N = c.N;
  RL_HIP(hipSetDevice(ctx->device));
  Arena ar(ctx);
  rl::MtState st;
  double* table = nullptr;
  RL_HIP(ar.carve([&](Arena& x) {
    rl::carve(x, st, rl::kMtArrays, B, N);
    if (!rows.empty()) table = x.take<double>(rows.size());
  }));
  // a pageable copy on the context's stream (the runtime has read `rows` when it returns, as for the long tables of
  // qss_sim_enqueue); the sub-batch streams fork behind it
  if (!rows.empty()) RL_HIP(hipMemcpyAsync(table, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  st.tol = c.tol;
  // Strategy constants of the line search / barrier update.  Measured on 1024 width-perturbed MGKT tracks:
  // (d_up, a_lo, mu_kappa) = (5, 0.3, 10) 96.5 iterations on average, (3, 0.2, 30) 77.8 (round 2).  Round 4: the damping
  // delta came down only after a step longer than a_hi = 0.9 -- but for dozens of iterations per barrier problem the
  // step is cut by the fraction-to-the-boundary rule to 0.3 .. 0.5 and accepted without a halving (iteration history,
  // tools/mintime_history.py), so delta stayed at 0.5 and the iteration crawled.  (a_hi, a_lo) = (0.25, 0.1): 82.1 -> 55.9
  // iterations on the benchmark batch, the same optima (lap times equal to 1e-12), 89.4 -> 66.8 on the 768 instances of
  // tools/mintime_robustness.py, all converged; a plateau: a_hi 0.11 .. 0.25, a_lo 0.05 .. 0.1, d_down 0.2 .. 0.5, d_up 2 .. 3 all
  // give 55 .. 57.  mu_kappa 60 or mu0 0.05 would take off three more; left alone.  They are COMPILE-TIME constants of the
  // product; only a diagnostic build (hipcc -DRL_ABLATION) reads RL_MT_* overrides from the environment.
#ifdef RL_ABLATION
  auto knob = [](const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; };
#else
  auto knob = [](const char*, double dflt) { return dflt; };
#endif
  st.d_down = knob("RL_MT_D_DOWN", 0.4); st.d_up = knob("RL_MT_D_UP", 3.0);
  st.a_hi = knob("RL_MT_A_HI", 0.25); st.a_lo = knob("RL_MT_A_LO", 0.1);
  st.mu_fac = knob("RL_MT_MU_FAC", 0.2); st.mu_pow = knob("RL_MT_MU_POW", 1.5); st.mu_kappa = knob("RL_MT_MU_KAPPA", 30.0);
  // dual step length <= dual_cap x primal step length (0 = uncoupled): with 1 all 768 instances of tools/mintime_robustness.py
  // converge (750 uncoupled: the multipliers ran away while the primal step was cut to a few per cent), at 82 instead of 78
  // iterations on the benchmark batch
  st.dual_cap = knob("RL_MT_DUAL_CAP", 1.0);
  st.th_filter = knob("RL_MT_TH_FILTER", 1e-4);   // 2e-5 .. 1e-3 all converge for mu0 = 0.05, 0.1, 0.2; 1e-2 blocks the early phase
  const double mt_mu0 = knob("RL_MT_MU0", 1e-1), mt_delta0 = knob("RL_MT_DELTA0", 1e-4);
  const size_t nscal = (size_t)B * rl::kMtScal;
  RL_HIP(hipMemsetAsync(st.scal, 0, nscal * sizeof(double), ctx->stream));
  if (ctx->mt_hes_sweep) RL_HIP(hipMemsetAsync(st.hes, 0, (size_t)B * N * rl::kMtLoc * rl::kMtLoc * sizeof(double), ctx->stream));
  // A few sub-batches on as many streams: the KKT elimination is one wave per instance and latency bound (its time
  // does not depend on the batch), the derivative kernels are throughput bound -- with the sub-batches offset by the
  // in-order queues one's elimination runs beside another's derivatives.  Instances are independent, so the split
  // changes no result.  The extra streams fork from / join into the context's stream with events:
  // for the caller everything is still "enqueued on the context's stream".
  const int ngrp = B >= 4 * ctx->mt_groups ? ctx->mt_groups : 1;
  auto stream = [](hipStream_t& q) { return q ? hipSuccess : hipStreamCreateWithFlags(&q, hipStreamNonBlocking); };
  auto event = [](hipEvent_t& e) { return e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming); };
  for (int g = 0; g + 1 < ngrp; ++g) { RL_HIP(stream(ctx->aux_stream[g])); RL_HIP(event(ctx->ev_join[g])); }
  if (ngrp > 1) RL_HIP(event(ctx->ev_fork));
  if (c.poll) {   // what the poll keeps on the context: its stream, its events, the pinned buffer of two slots
    RL_HIP(stream(ctx->poll_stream));
    for (int g = 0; g < ngrp; ++g) RL_HIP(event(ctx->ev_chunk[g]));
    for (auto& e : ctx->ev_poll) RL_HIP(event(e));
    if (ctx->poll_cap < nscal) {
      if (ctx->poll_host) RL_HIP(hipHostFree(ctx->poll_host));
      ctx->poll_host = nullptr; ctx->poll_cap = 0;
      RL_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->poll_host), 2 * nscal * sizeof(double), hipHostMallocDefault));
      ctx->poll_cap = nscal;
    }
  }
  StreamFork fork{ctx, ngrp};   // after `ar`: joined before the arena's event is recorded, on every exit
  MtGroup<PT> grp[rl_ctx::kMaxGroups];
  for (int g = 0; g < ngrp; ++g) {
    const int b0 = (int)((long long)B * g / ngrp), nb = (int)((long long)B * (g + 1) / ngrp) - b0;
    const size_t o = (size_t)b0 * N;
    MtGroup<PT>& G = grp[g];
    G.q = fork_stream(ctx, g); G.P = P; G.st = rl::slice(st, rl::kMtArrays, b0, nb);
    if (P.bounds_per_instance) { G.P.left = c.left + o; G.P.right = c.right + o; }
    mt_set_model(G.M, G.P, table ? table + (size_t)b0 * rl::kMtRow : nullptr);
    G.X = c.X + o * 6; G.U = c.U + o * 4; G.T = c.T + o; G.stats = c.stats + (size_t)b0 * rl::kMtStats;
    G.rows = dim3(rl::mt_row_blocks(N), nb); G.per_node = dim3(N, nb); G.per_inst = dim3(nb);
  }
  if (ngrp > 1) RL_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));   // the auxiliary streams start behind what is already enqueued
  for (int g = 1; g < ngrp; ++g) RL_HIP(hipStreamWaitEvent(grp[g].q, ctx->ev_fork, 0));
  for (int g = 0; g < ngrp; ++g) {
    const MtGroup<PT>& G = grp[g];
    RL_TRY(mt_pack(ctx, G));
    RL_TRY(mt_run_model(ctx, G, rl::k_mt_derivs<0, PT>, G.rows, 64));
    RL_TRY(launch(ctx, G.q, rl::k_mt_init, dim3(rl::mt_init_blocks(N), G.st.B), dim3(256), 0, G.P, G.st, mt_mu0, mt_delta0));
  }
  for (int it = 0; it < c.max_iter; ++it) {
    for (int g = 0; g < ngrp; ++g) RL_TRY(mt_enqueue_iteration(ctx, grp[g]));
    if (c.poll && (it & 7) == 7) {   // host entry point only: stop once every instance has finished
      const int chunk = it >> 3, slot = chunk & 1;
      fork.polled = true;
      for (int g = 0; g < ngrp; ++g) {
        RL_HIP(hipEventRecord(ctx->ev_chunk[g], grp[g].q));
        RL_HIP(hipStreamWaitEvent(ctx->poll_stream, ctx->ev_chunk[g], 0));
      }
      // The copy is ordered after THIS chunk's kernels only; the next chunk's kernels, enqueued below, may already be writing
      // `scal` while it runs -- an unsynchronised read, deliberately: the host looks at nothing but word 5 of every instance
      // (status: 0 -> 1 / 2, written once, never back; an aligned 8-byte word is copied whole), so a stale value can only
      // delay the early exit by one chunk and a fresh one cannot end it early: `all` needs EVERY instance finished, and a
      // finished instance's kernels return at their first line.
      RL_HIP(hipMemcpyAsync(ctx->poll_host + (size_t)slot * ctx->poll_cap, st.scal, nscal * sizeof(double), hipMemcpyDeviceToHost, ctx->poll_stream));
      RL_HIP(hipEventRecord(ctx->ev_poll[slot], ctx->poll_stream));
      if (chunk >= 1) {   // the chunk before this one: its copy is done, or nearly, while this chunk keeps the GPU busy
        RL_HIP(hipEventSynchronize(ctx->ev_poll[slot ^ 1]));
        const double* h = ctx->poll_host + (size_t)(slot ^ 1) * ctx->poll_cap;
        bool all = true;
        for (int b = 0; b < B && all; ++b) all = h[(size_t)b * rl::kMtScal + rl::kMtStatus] != 0.0;
        if (all) break;
      }
    }
  }
  if (c.poll) { fork.polled = false; RL_HIP(hipStreamSynchronize(ctx->poll_stream)); }   // no copy in flight into the pinned buffer when the call returns
  for (int g = 0; g < ngrp; ++g) RL_TRY(mt_enqueue_closing(ctx, grp[g]));
  RL_HIP(join_streams(ctx, std::exchange(fork.n, 1)));
  RL_HIP(ar.end());
  return RL_OK;
}
}  // extern "C++"

// A checked call on device pointers: the problem as the model-blind kernels take it, the table of a table call -- and the one
// place where the form of the solve is chosen.
int mt_solve(rl_ctx* ctx, const MtCall& c) {
  rl::MtProblem P;
  P.N = c.N; P.bounds_per_instance = c.bounds_per_instance ? 1 : 0;
  P.margin = c.margin; P.track_length = c.track_length;   // NaN in a tracks call: the kernels take it from the instance's row
  P.s = c.s; P.kappa = c.kappa; P.left = c.left; P.right = c.right;
  std::vector<double> rows;   // a table call: p | sw | se (| track_length | track), kMtRow doubles per instance
  if (c.table()) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (double& v : P.p) v = nan;
    for (double& v : P.sw) v = nan;
    for (double& v : P.se) v = nan;
    rows.assign((size_t)c.B * rl::kMtRow, 0.0);
    mt_build_rows(rows.data(), c);
  } else {
    for (int i = 0; i < rl::DT_NPARAM; ++i) P.p[i] = c.model[i];
    mt_scales(c.model, c.average_track_width, c.speed_cap, P.sw, P.se);
  }
  if (c.tr) return mt_solve_as<rl::MtProblemT>(ctx, c, P, rows);
  return c.model_rows ? mt_solve_as<rl::MtProblemV>(ctx, c, P, rows) : mt_solve_as<rl::MtProblem>(ctx, c, P, rows);
}

// the host entries: stage the arrays of a checked call, solve with the poll, bring the results down
int mt_stage_and_solve(rl_ctx* ctx, MtCall c) {
  const size_t bn = (size_t)c.B * c.N, nb_ = c.bounds_per_instance ? bn : (size_t)c.N, ns = (size_t)(c.tr ? c.tr->T : 1) * c.N;
  Staging sg(ctx);
  c.s = sg.in(c.s, ns); c.kappa = sg.in(c.kappa, ns); c.left = sg.in(c.left, nb_); c.right = sg.in(c.right, nb_);
  c.X = sg.inout(c.X, bn * 6); c.U = sg.inout(c.U, bn * 4); c.T = sg.inout(c.T, bn);
  c.stats = sg.out(c.stats, (size_t)c.B * rl::kMtStats);
  c.poll = true;
  sg.run([&] { return mt_solve(ctx, c); });
  return sg.finish();
}

}  // namespace

// The six entries: fill the record (the arguments in the record's order), check it, then solve (device pointers) or stage and
// solve (host pointers).  model_rows is what tells a vehicles entry from its shared-model twin.
int rl_mintime_solve_batch_dev(rl_ctx* ctx, const double* model, int B, int N, const double* s, const double* kappa, const double* left,
                               const double* right, int bounds_per_instance, double margin, double track_length, double average_track_width,
                               double speed_cap, double* X, double* U, double* T, int max_iter, double tol, double* stats) {
  const MtCall c{model, false, B, N, s, kappa, left, right, bounds_per_instance, margin, X, U, T, stats, max_iter, tol, track_length, average_track_width, speed_cap};
  RL_TRY(mt_check_call(ctx, c, false));
  return mt_solve(ctx, c);
}

int rl_mintime_solve_vehicles_dev(rl_ctx* ctx, const double* models, int B, int N, const double* s, const double* kappa, const double* left,
                                  const double* right, int bounds_per_instance, double margin, double track_length, double average_track_width,
                                  double speed_cap, double* X, double* U, double* T, int max_iter, double tol, double* stats) {
  const MtCall c{models, true, B, N, s, kappa, left, right, bounds_per_instance, margin, X, U, T, stats, max_iter, tol, track_length, average_track_width, speed_cap};
  RL_TRY(mt_check_call(ctx, c, false));
  return mt_solve(ctx, c);
}

int rl_mintime_solve_batch(rl_ctx* ctx, const double* model, int B, int N, const double* s, const double* kappa, const double* left,
                           const double* right, int bounds_per_instance, double margin, double track_length, double average_track_width,
                           double speed_cap, double* X, double* U, double* T, int max_iter, double tol, double* stats) {
  const MtCall c{model, false, B, N, s, kappa, left, right, bounds_per_instance, margin, X, U, T, stats, max_iter, tol, track_length, average_track_width, speed_cap};
  RL_TRY(mt_check_call(ctx, c, true));
  return mt_stage_and_solve(ctx, c);
}

int rl_mintime_solve_vehicles(rl_ctx* ctx, const double* models, int B, int N, const double* s, const double* kappa, const double* left,
                              const double* right, int bounds_per_instance, double margin, double track_length, double average_track_width,
                              double speed_cap, double* X, double* U, double* T, int max_iter, double tol, double* stats) {
  const MtCall c{models, true, B, N, s, kappa, left, right, bounds_per_instance, margin, X, U, T, stats, max_iter, tol, track_length, average_track_width, speed_cap};
  RL_TRY(mt_check_call(ctx, c, true));
  return mt_stage_and_solve(ctx, c);
}

// The host half of a vehicles (T = 0: the scalars average_track_width[0], speed_cap[0]) or a tracks call (T >= 1) without a
// device: the checks, then the table [B,48] the call would copy.  What the CPU tests compare with the shared entries' scales.
int rl_debug_mt_rows(const double* models, int models_per_instance, int B, int T, const int* track_of, const double* track_length,
                     const double* average_track_width, const double* speed_cap, double* rows) {
  if (!models || !rows || !average_track_width || !speed_cap || B <= 0 || T < 0) return fail(RL_ERR_ARG, "null argument or bad sizes");
  const MtTracks tr{T, track_of, track_length, average_track_width, speed_cap};
  MtCall c{models, T == 0 || models_per_instance, B};
  c.average_track_width = average_track_width[0]; c.speed_cap = speed_cap[0]; c.tr = T > 0 ? &tr : nullptr;
  RL_TRY(mt_check_table(c));
  std::fill(rows, rows + (size_t)B * rl::kMtRow, 0.0);
  mt_build_rows(rows, c);
  return RL_OK;
}

// One centre line per instance: s, kappa [T,N]; everything per track or per instance that the host reads (models, track_of,
// the three arrays [T]) is a HOST array in both entries.  The bounds are per instance.
int rl_mintime_solve_tracks_dev(rl_ctx* ctx, const double* models, int models_per_instance, int B, int N, int T, const int* track_of,
                                const double* s, const double* kappa, const double* left, const double* right, double margin,
                                const double* track_length, const double* average_track_width, const double* speed_cap, double* X,
                                double* U, double* Tn, int max_iter, double tol, double* stats) {
  const MtTracks tr{T, track_of, track_length, average_track_width, speed_cap};
  MtCall c{models, models_per_instance != 0, B, N, s, kappa, left, right, 1, margin, X, U, Tn, stats, max_iter, tol};
  c.tr = &tr;
  RL_TRY(mt_check_call(ctx, c, false));
  return mt_solve(ctx, c);
}

int rl_mintime_solve_tracks(rl_ctx* ctx, const double* models, int models_per_instance, int B, int N, int T, const int* track_of,
                            const double* s, const double* kappa, const double* left, const double* right, double margin,
                            const double* track_length, const double* average_track_width, const double* speed_cap, double* X,
                            double* U, double* Tn, int max_iter, double tol, double* stats) {
  const MtTracks tr{T, track_of, track_length, average_track_width, speed_cap};
  MtCall c{models, models_per_instance != 0, B, N, s, kappa, left, right, 1, margin, X, U, Tn, stats, max_iter, tol};
  c.tr = &tr;
  RL_TRY(mt_check_call(ctx, c, true));
  return mt_stage_and_solve(ctx, c);
}

// ---- the bicycle min-time NLP (rl_bicycle.hpp)
// what the kernels divide by and what makes the box bounds a box: the one statement of the checks on a model, for the
// shared-model entries (`who` = "bicycle model") and for every row of a per-instance call ("models: instance b")
static int bk_check_model(const double* model, const std::string& who) {
  for (int i = 0; i < rl::BK_NPARAM; ++i)
    if (!std::isfinite(model[i])) return fail(RL_ERR_ARG, who + ": non-finite parameter");
  if (!(model[RL_BK_L] > 0.0) || !(model[RL_BK_DELTA_MAX] > 0.0) || !(model[RL_BK_V_MAX] > 0.0) ||
      !(model[RL_BK_A_LON_MAX] > model[RL_BK_A_LON_MIN]) || !(model[RL_BK_DELTA_DOT_MAX] > 0.0) || !(model[RL_BK_ACC_MAX] > 0.0))
    return fail(RL_ERR_ARG, who + ": L, delta_max, v_max, delta_dot_max, acc_max > 0 and a_lon_max > a_lon_min");
  return RL_OK;
}

static int bk_problem(const double* model, int N, rl::BkProblem& P) {
  if (int rc = bk_check_model(model, "bicycle model")) return rc;
  for (int i = 0; i < rl::BK_NPARAM; ++i) P.m[i] = model[i];
  P.N = N;
  return RL_OK;
}

// a per-instance call checks every row before anything is staged or enqueued; RL_ERR_ARG names the first bad instance
static int bk_check_models(const double* models, int models_per_instance, int B) {
  for (int b = 0; b < (models_per_instance ? B : 1); ++b)
    if (int rc = bk_check_model(models + (size_t)b * RL_BK_NPARAM, "models: instance " + std::to_string(b))) return rc;
  return RL_OK;
}

// One text of the device work for both problem types (<BkProblem>: the shared-model entries, <BkProblemV>: the per-instance
// entries): the bit-equality of the two rests on the launch sequences being the same.
extern "C++" {
inline void bk_set_table(rl::BkProblem&, const double*) {}
inline void bk_set_table(rl::BkProblemV& P, const double* table) { P.m = (rl::BkTab)table; }

// the solve on device pointers: state (and the model table `rows`, if any) from the context's scratch, the launches
template <typename PT>
int bk_solve_dev(rl_ctx* ctx, PT P, const std::vector<double>& rows, int B, int N, double* X, double* U, double* T, int max_iter, double* stats) {
  RL_HIP(hipSetDevice(ctx->device));
  Arena ar(ctx);
  rl::BkState st;
  double* table = nullptr;
  RL_HIP(ar.carve([&](Arena& x) {
    rl::carve(x, st, rl::kBkArrays, B, N);
    if (!rows.empty()) table = x.take<double>(rows.size());
  }));
  // a pageable copy on the context's stream, before the first launch: the runtime has read `rows` when it returns (as for
  // the model table of rl_mintime_solve_vehicles*)
  if (!rows.empty()) RL_HIP(hipMemcpyAsync(table, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  bk_set_table(P, table);
  const dim3 grid(B), block(rl::kBkThreads);
  RL_TRY(launch(ctx, rl::k_bk_init<PT>, grid, block, 0, P, st, X, U, T));
  // exactly max_iter iterations are enqueued; an instance that has converged or failed returns from each at once
  for (int it = 0; it < max_iter; ++it) RL_TRY(launch(ctx, rl::k_bk_iter<PT>, grid, block, 0, P, st, 0));
  RL_TRY(launch(ctx, rl::k_bk_iter<PT>, grid, block, 0, P, st, 1));
  RL_TRY(launch(ctx, rl::k_bk_unpack<PT>, dim3((N + 63) / 64, B), dim3(64), 0, P, st, X, U, T, stats));
  RL_HIP(ar.end());
  return RL_OK;
}

// the function evaluation on host pointers; nl: doubles of yaw (N shared, B N per instance)
template <typename PT>
int bk_eval_host(rl_ctx* ctx, PT P, const std::vector<double>& rows, int B, int N, const double* P0, const double* yaw, size_t nl,
                 const double* X, const double* U, const double* T, double* eq, double* ineq, double* cost) {
  const size_t bn = (size_t)B * N;
  Staging sg(ctx);
  bk_set_table(P, sg.in(rows.empty() ? nullptr : rows.data(), rows.size()));
  P.P0 = sg.in(P0, 2 * nl); P.yaw = sg.in(yaw, nl);
  const double *dX = sg.in(X, bn * 5), *dU = sg.in(U, bn * 2), *dT = sg.in(T, bn);
  double *deq = sg.out(eq, bn * rl::kBkNe), *din = sg.out(ineq, bn * 2);
  sg.run([&] { return launch(ctx, rl::k_bk_eval<PT>, dim3((N + 63) / 64, B), dim3(64), 0, P, B, dX, dU, dT, deq, din); });
  if (int rc = sg.finish()) return rc;
  for (int b = 0; b < B; ++b) {   // min_time_cost (:9-10), summed in node order
    double c = 0.0;
    for (int j = 0; j < N; ++j) c += T[(size_t)b * N + j];
    cost[b] = c;
  }
  return RL_OK;
}
}  // extern "C++"

// the table [B, RL_BK_NPARAM] the <BkProblemV> kernels read: the caller's rows, or its one row B times
static std::vector<double> bk_table(const double* models, int models_per_instance, int B) {
  std::vector<double> rows((size_t)B * RL_BK_NPARAM);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < RL_BK_NPARAM; ++i) rows[(size_t)b * RL_BK_NPARAM + i] = models[(models_per_instance ? (size_t)b * RL_BK_NPARAM : 0) + i];
  return rows;
}

int rl_bicycle_eval_nodes(rl_ctx* ctx, const double* model, int B, int N, const double* P0, const double* yaw,
                          const double* X, const double* U, const double* T, double* eq, double* ineq, double* cost) {
  if (!ctx || !model || !P0 || !yaw || !X || !U || !T || !eq || !ineq || !cost) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 8) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes)");
  rl::BkProblem P{};
  if (int rc = bk_problem(model, N, P)) return rc;
  return bk_eval_host(ctx, P, {}, B, N, P0, yaw, (size_t)N, X, U, T, eq, ineq, cost);
}

int rl_bicycle_solve_batch_dev(rl_ctx* ctx, const double* model, int B, int N, const double* P0, const double* yaw,
                               const double* dl, const double* dr, int bounds_per_instance, double* X, double* U, double* T,
                               int max_iter, double tol, double* stats) {
  if (!ctx || !model || !P0 || !yaw || !dl || !dr || !X || !U || !T || !stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 8 || max_iter < 1 || !(tol > 0.0)) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes, max_iter >= 1, tol > 0)");
  rl::BkProblem P{};
  if (int rc = bk_problem(model, N, P)) return rc;
  P.per = bounds_per_instance ? 1 : 0;
  P.P0 = P0; P.yaw = yaw; P.dl = dl; P.dr = dr; P.tol = tol;
  return bk_solve_dev(ctx, P, {}, B, N, X, U, T, max_iter, stats);
}

int rl_bicycle_solve_batch(rl_ctx* ctx, const double* model, int B, int N, const double* P0, const double* yaw,
                           const double* dl, const double* dr, int bounds_per_instance, double* X, double* U, double* T,
                           int max_iter, double tol, double* stats) {
  if (!ctx || !model || !P0 || !yaw || !dl || !dr || !X || !U || !T || !stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 8) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes)");
  const size_t bn = (size_t)B * N, nb_ = bounds_per_instance ? bn : (size_t)N;
  for (size_t i = 0; i < nb_; ++i)
    if (!(dr[i] < dl[i])) return fail(RL_ERR_ARG, "bounds: need dr < dl at every node (min_time_optimizer.py:66-68)");
  Staging sg(ctx);
  const double *dP0 = sg.in(P0, (size_t)2 * N), *dyaw = sg.in(yaw, N), *ddl = sg.in(dl, nb_), *ddr = sg.in(dr, nb_);
  double *dX = sg.inout(X, bn * 5), *dU = sg.inout(U, bn * 2), *dT = sg.inout(T, bn);
  double* dst = sg.out(stats, (size_t)B * rl::kBkStats);
  sg.run([&] {
    return rl_bicycle_solve_batch_dev(ctx, model, B, N, dP0, dyaw, ddl, ddr, bounds_per_instance, dX, dU, dT, max_iter, tol, dst);
  });
  return sg.finish();
}

int rl_bicycle_eval_nodes_lines(rl_ctx* ctx, const double* models, int models_per_instance, int B, int N, const double* P0,
                                const double* yaw, int lines_per_instance, const double* X, const double* U, const double* T,
                                double* eq, double* ineq, double* cost) {
  if (!ctx || !models || !P0 || !yaw || !X || !U || !T || !eq || !ineq || !cost) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 8) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes)");
  if (int rc = bk_check_models(models, models_per_instance, B)) return rc;
  const std::vector<double> rows = bk_table(models, models_per_instance, B);
  rl::BkProblemV P{};
  P.N = N; P.lines = lines_per_instance ? 1 : 0;
  return bk_eval_host(ctx, P, rows, B, N, P0, yaw, lines_per_instance ? (size_t)B * N : (size_t)N, X, U, T, eq, ineq, cost);
}

int rl_bicycle_solve_lines_dev(rl_ctx* ctx, const double* models, int models_per_instance, int B, int N, const double* P0,
                               const double* yaw, int lines_per_instance, const double* dl, const double* dr,
                               int bounds_per_instance, double* X, double* U, double* T, int max_iter, double tol, double* stats) {
  if (!ctx || !models || !P0 || !yaw || !dl || !dr || !X || !U || !T || !stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 8 || max_iter < 1 || !(tol > 0.0)) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes, max_iter >= 1, tol > 0)");
  if (lines_per_instance && !bounds_per_instance)
    return fail(RL_ERR_ARG, "lines_per_instance needs bounds_per_instance: dl / dr are distances from the instance's own line");
  if (int rc = bk_check_models(models, models_per_instance, B)) return rc;
  const std::vector<double> rows = bk_table(models, models_per_instance, B);
  rl::BkProblemV P{};
  P.N = N; P.per = bounds_per_instance ? 1 : 0; P.lines = lines_per_instance ? 1 : 0;
  P.P0 = P0; P.yaw = yaw; P.dl = dl; P.dr = dr; P.tol = tol;
  return bk_solve_dev(ctx, P, rows, B, N, X, U, T, max_iter, stats);
}

int rl_bicycle_solve_lines(rl_ctx* ctx, const double* models, int models_per_instance, int B, int N, const double* P0,
                           const double* yaw, int lines_per_instance, const double* dl, const double* dr,
                           int bounds_per_instance, double* X, double* U, double* T, int max_iter, double tol, double* stats) {
  if (!ctx || !models || !P0 || !yaw || !dl || !dr || !X || !U || !T || !stats) return fail(RL_ERR_ARG, "null argument");
  if (B <= 0 || N < 8 || max_iter < 1 || !(tol > 0.0)) return fail(RL_ERR_ARG, "bad sizes (N >= 8 nodes, max_iter >= 1, tol > 0)");
  if (lines_per_instance && !bounds_per_instance)
    return fail(RL_ERR_ARG, "lines_per_instance needs bounds_per_instance: dl / dr are distances from the instance's own line");
  if (int rc = bk_check_models(models, models_per_instance, B)) return rc;   // before anything is staged
  const size_t bn = (size_t)B * N, nb_ = bounds_per_instance ? bn : (size_t)N, nl = lines_per_instance ? bn : (size_t)N;
  for (size_t i = 0; i < nb_; ++i)
    if (!(dr[i] < dl[i]))
      return fail(RL_ERR_ARG, "bounds: instance " + std::to_string(bounds_per_instance ? i / N : 0) + ": need dr < dl at every node (min_time_optimizer.py:66-68)");
  Staging sg(ctx);
  const double *dP0 = sg.in(P0, 2 * nl), *dyaw = sg.in(yaw, nl), *ddl = sg.in(dl, nb_), *ddr = sg.in(dr, nb_);
  double *dX = sg.inout(X, bn * 5), *dU = sg.inout(U, bn * 2), *dT = sg.inout(T, bn);
  double* dst = sg.out(stats, (size_t)B * rl::kBkStats);
  sg.run([&] {
    return rl_bicycle_solve_lines_dev(ctx, models, models_per_instance, B, N, dP0, dyaw, lines_per_instance, ddl, ddr,
                                      bounds_per_instance, dX, dU, dT, max_iter, tol, dst);
  });
  return sg.finish();
}

}  // extern "C"

static int sweep_single(rl_ctx* ctx, rl_track* trk, const int* i_start, int max_iter, double* cx, double* cy,
                        double* points, int* n_success, rl_stats* stats, bool joint) {
  if (!ctx || !trk || !cx || !cy) return fail(RL_ERR_ARG, "null argument");
  const int n = trk->n, N = trk->N;
  if (int rc = rl_track_set_control_points(trk, cx, cy)) return rc;
  std::vector<double> ctrl((size_t)2 * n);
  std::vector<int> ns_host((size_t)2 * (max_iter > 0 ? max_iter : 1));
  Staging sg(ctx);
  double* dctrl = sg.out(ctrl.data(), ctrl.size());
  double* dpts = sg.out_optional(points, (size_t)N * RL_NCOL);
  int* dns = sg.out(ns_host.data(), ns_host.size());
  int* dst = sg.scratch<int>(1);
  sg.run([&]() -> int {
    RL_HIP(hipMemsetAsync(dpts, 0, (size_t)N * RL_NCOL * sizeof(double), ctx->stream));
    return RL_OK;
  });
  sg.run_timed([&] {
    return solve_batch_common(ctx, trk, RL_BOUNDS_SHARED_RINGS, nullptr, 1, i_start, max_iter, RL_SEARCH_WINDOWED, dctrl, nullptr, dpts,
                              dns, dst, stats, nullptr, joint);
  });
  if (points && trk->length > 0.0) {
    // DIST_TO_SF_BWD / _FWD of the final table (models/trajectory.py:283-289): GK21 segment lengths of the
    // optimised spline, accumulated in the reference's order; DIST_FWD uses the length the spline object
    // was CONSTRUCTED with (set_control_point never updates _length, trajectory.py:296-298)
    double *dseg = sg.scratch<double>(N), *dcx = sg.scratch<double>((size_t)2 * n);
    sg.run([&] {
      if (int rc = launch(ctx, rl::k_split_ctrl, dim3((n + 63) / 64), dim3(64), 0, dctrl, n, dcx)) return rc;
      if (int rc = by_degree(trk->k, [&](auto kc) {
            return launch(ctx, rl::k_sample_geometry<RL_DEGREE(kc)>, dim3((N + 127) / 128), dim3(128), 0, trk->t.p, trk->nt, dcx, dcx + n,
                          nullptr, N, nullptr, dseg);
          }))
        return rc;
      return launch(ctx, rl::k_sample_cumsum, dim3(1), dim3(64), 0, dseg, N, trk->length, dpts);
    });
  }
  if (int rc = sg.finish(stats)) return rc;
  for (int j = 0; j < n; ++j) { cx[j] = ctrl[2 * j]; cy[j] = ctrl[2 * j + 1]; }
  if (n_success) {  // sweep: [max_iter][fwd,bwd]; sliding window: [max_iter]
    if (joint) for (int j = 0; j < max_iter; ++j) n_success[j] = ns_host[2 * j];
    else for (int j = 0; j < 2 * max_iter; ++j) n_success[j] = ns_host[j];
  }
  if (points) {
    for (int i = 0; i < N; ++i) { points[(size_t)i * RL_NCOL + 17] = (double)i; points[(size_t)i * RL_NCOL + 18] = -1.0; }
  }
  return RL_OK;
}

#ifdef RL_MT_HIST
extern "C" int rl_debug_mt_hist(unsigned long long* out) {   // diagnostic build only
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(rl::g_mt_hist), 16 * sizeof(unsigned long long));
}
#endif
