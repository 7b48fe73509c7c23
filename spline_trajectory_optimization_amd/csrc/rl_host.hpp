// rl_host.hpp -- host plumbing of rl_mincurv.hip: error reporting, device buffers, the context, and the two helpers every
// entry point goes through: launch() for one kernel, Staging for the device copies of a host-pointer call.
//
// The rules they keep -- when a block or the arena is free again, nothing enqueued after a failure, what the timed events
// bracket, forked streams joined on every exit -- are stated once, in DESIGN section 2 ("Boundary").
#pragma once

#include "../../include/rl_mincurv.h"

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define RL_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      return fail(RL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
    }                                                                                     \
  } while (0)
#define RL_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)   // a step that returns an rl status: the first failure returns

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

}  // namespace

struct rl_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int max_lds = 65536;
  int num_cu = 0;
  bool force_global_v1 = false;  // test hook: RL_GLOBAL_V1=1 keeps the generic kernel
  int arith = RL_ARITH_REFERENCE;   // rl_ctx_set_arith: arithmetic of the sweep; the reference-order arithmetic since round 6
  bool arith_explicit = false;      // set by rl_ctx_set_arith / RL_ARITH: an explicit choice fails where it does not exist, the default follows
  int np_raise_at_start = 0;     // rl_ctx_set_numpy_raise: the reference-order sweep starts with np.seterr(all='raise') in effect
  // test hooks of the QSS simulator (rl_ctx_set_option; defaults from RL_QSS_DF / RL_QSS_V1 / RL_QSS_DF_WAVES / RL_QSS_DF_BAIL_AT, read
  // once in rl_ctx_create): which kernel (-1 = by the rounds the batch takes, 0 = list order, 1 = dataflow), waves per instance of
  // the dataflow kernel, the iteration at which it hands every instance back (0 = never), whether the list-order kernel re-runs
  // what it handed back (1; 0 = no: such an instance returns iters = RL_QSS_HANDED_BACK - reason and keeps its input rows)
  int qss_kernel = -1, qss_df_waves = 4, qss_df_bail_at = 0, qss_df_redo = 1;
  int global_last_as_mid = 0;  // test hook: the global QPs' last linearisation leaves at the intermediate tolerance
  int sweep_bracket = 1;   // the sweep's window scan may bracket the crossing around its hint (test hook "sweep_bracket" = 0: always the full sign pass)
  // test hooks of rl_tables_batch_*: ring search (RL_SEARCH_*), 1 = ring vertices in the arena even where they fit LDS
  int tables_search = RL_SEARCH_WINDOWED, tables_rings_global = 0;
  int frenet_search = 1;         // test hook of rl_frenet_batch_*: 0 = every point from the table's own bound, 1 = from the previous point's piece
  // Device scratch owned by the context (grow-only): the *_dev entry points of the QSS simulator and the
  // min-time solve carve their work arrays out of it, so that steady-state calls allocate nothing.
  void* arena = nullptr;
  size_t arena_cap = 0;
  // The arena is handed out from offset 0 by every *_dev call, so two calls may only overlap in time if they are
  // ordered on the device: each call records `arena_ev` behind its last use, and a call made after
  // rl_ctx_set_stream switched to another stream first makes that stream wait for the event (Arena::carve).
  hipEvent_t arena_ev = nullptr;
  hipStream_t arena_stream = nullptr;
  bool arena_busy = false;       // arena_ev has been recorded at least once
  // second in-order queue of the min-time solve (half batches side by side), forked from / joined into `stream`
  static constexpr int kMaxGroups = 8;
  hipStream_t aux_stream[kMaxGroups - 1] = {};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxGroups - 1] = {};
  // the poll never drains the queues: the status words of a chunk of 8 iterations are copied by a side stream into pinned
  // memory while the next chunk is already enqueued, and looked at one chunk later
  hipStream_t poll_stream = nullptr;
  hipEvent_t ev_chunk[kMaxGroups] = {}, ev_poll[2] = {nullptr, nullptr};
  double* poll_host = nullptr;   // pinned, 2 x poll_cap doubles
  size_t poll_cap = 0;
  bool mt_hes_sweep = false;     // RL_MT_HES_SWEEP=1: the Hessian by k_mt_derivs<2> instead of the chain-rule kernels
  bool mt_kkt4 = true;           // RL_MT_KKT4=0: the elimination with two fronts per instance (k_mt_kkt) instead of four (k_mt_kkt4, N >= 64)
  bool mt_unfused = false;       // RL_MT_UNFUSED=1: Jacobian / Hessian / block assembly by the four separate kernels instead of k_mt_node
  int mt_groups = 3;             // RL_MT_GROUPS=1..8 (round 3, 1024 instances: 1 / 2 / 3 / 4 / 8 streams 1.23 / 1.29 / 1.21 / 1.19 / 1.19 s)
  // Device staging blocks of the HOST-pointer entry points (PoolBuf): handed out best-fit, returned at the end of
  // the call, freed with the context -- a second call of the same shape allocates nothing.
  struct PoolBlock { void* p; size_t cap; bool used; };
  std::vector<PoolBlock> pool;
};

namespace {
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the FUNCTION on a device, shared by every context of the
// process: one process-wide table per (device, kernel) that only ever raises the value, instead of one call per launch
// (a per-context cache would go stale as soon as a second context asked for less).
hipError_t grant_dyn_lds(const rl_ctx* ctx, const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::vector<std::pair<std::pair<int, const void*>, size_t>> granted;
  std::lock_guard<std::mutex> lock(mu);
  const std::pair<int, const void*> key(ctx->device, fn);
  for (auto& e : granted)
    if (e.first == key) {
      if (e.second >= bytes) return hipSuccess;
      const hipError_t r = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (r == hipSuccess) e.second = bytes;
      return r;
    }
  const hipError_t r = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (r == hipSuccess) granted.emplace_back(key, bytes);
  return r;
}

// One kernel on `stream`: the dynamic-LDS grant where the launch asks for any, the launch, its error.  The
// arguments are converted to the kernel's parameter types (a double* for a const double*, nullptr for a pointer).
template <typename... P, typename... A>
int launch(const rl_ctx* ctx, hipStream_t stream, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, A&&... args) {
  if (lds_bytes > 0) RL_HIP(grant_dyn_lds(ctx, reinterpret_cast<const void*>(kernel), lds_bytes));
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, static_cast<P>(std::forward<A>(args))...);
  RL_HIP(hipGetLastError());
  return RL_OK;
}
template <typename... P, typename... A>
int launch(const rl_ctx* ctx, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, A&&... args) {   // on the context's stream
  return launch(ctx, ctx->stream, kernel, grid, block, lds_bytes, std::forward<A>(args)...);
}

// one device staging block from the context's pool (Staging below hands them out)
template <typename T>
struct PoolBuf {
  rl_ctx* ctx = nullptr;
  T* p = nullptr;
  size_t n = 0;
  int slot = -1;
  PoolBuf() = default;
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    int best = -1;
    for (int i = 0; i < (int)ctx->pool.size(); ++i)
      if (!ctx->pool[i].used && ctx->pool[i].cap >= bytes && ctx->pool[i].cap <= 4 * bytes + 4096 &&   // never park a small request on a huge block
          (best < 0 || ctx->pool[i].cap < ctx->pool[best].cap)) best = i;
    if (best < 0) {
      if (ctx->pool.size() >= 96) {   // shapes keep changing: drop what is idle before growing further
        for (auto& blk : ctx->pool)
          if (!blk.used && blk.p) { (void)hipFree(blk.p); blk.p = nullptr; blk.cap = 0; }
      }
      void* q = nullptr;
      hipError_t e = hipMalloc(&q, bytes);
      if (e != hipSuccess) {          // out of memory: give back what is idle, then try once more
        (void)hipGetLastError();
        for (auto& blk : ctx->pool)
          if (!blk.used && blk.p) { (void)hipFree(blk.p); blk.p = nullptr; blk.cap = 0; }
        e = hipMalloc(&q, bytes);
      }
      if (e != hipSuccess) return e;
      for (int i = 0; i < (int)ctx->pool.size() && best < 0; ++i)
        if (!ctx->pool[i].p) { ctx->pool[i] = {q, bytes, false}; best = i; }
      if (best < 0) { ctx->pool.push_back({q, bytes, false}); best = (int)ctx->pool.size() - 1; }
    }
    ctx->pool[best].used = true;
    slot = best;
    p = static_cast<T*>(ctx->pool[best].p);
    return hipSuccess;
  }
  void release() {
    if (slot >= 0) ctx->pool[slot].used = false;
    slot = -1; p = nullptr; n = 0;
  }
  // Success paths end with a stream synchronisation, so the block is idle here.  An early error return does not: wait for
  // whatever was already enqueued (copies into / out of this block) before the block can be handed to the next call.
  ~PoolBuf() {
    if (slot >= 0 && hipStreamQuery(ctx->stream) == hipErrorNotReady) (void)hipStreamSynchronize(ctx->stream);
    release();
  }
  PoolBuf(const PoolBuf&) = delete;
  PoolBuf& operator=(const PoolBuf&) = delete;
};

// The device side of one host-pointer call.  in / out / inout / scratch hand out pool blocks (doubles or ints; a host
// destination may be a std::vector's storage that lives until finish), run / run_timed enqueue the device work, finish
// brings the outputs down and waits.  The first failure of any step is latched: every later step is skipped and finish
// returns it -- RL_ERR_HIP for a step of this object, the device work's own code otherwise.
class Staging {
 public:
  explicit Staging(rl_ctx* ctx) : ctx_(ctx) { hip(hipSetDevice(ctx->device), "hipSetDevice"); }
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;

  template <typename T> T* scratch(size_t count) {
    if (rc_ != RL_OK || count == 0) return nullptr;
    if (nblk_ == kMaxBlocks) { rc_ = fail(RL_ERR_HIP, "staging: more blocks than one call may hold"); return nullptr; }
    PoolBuf<char>& b = blk_[nblk_];
    b.ctx = ctx_;
    if (!hip(b.alloc(count * sizeof(T)), "staging block")) return nullptr;
    ++nblk_;
    return reinterpret_cast<T*>(b.p);
  }
  // an input: the block and its copy to the device; a null `host` gives a null device pointer and no block
  template <typename T> T* in(const T* host, size_t count) {
    T* d = host ? scratch<T>(count) : nullptr;
    if (d) hip(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, ctx_->stream), "copy to the device");
    return d;
  }
  // an output the device work writes only when asked: a null `host` gives a null device pointer and no block
  template <typename T> T* out(T* host, size_t count) { return host ? out_optional(host, count) : nullptr; }
  // an output the device work always writes: the block is made either way, the copy at finish only for a non-null `host`
  template <typename T> T* out_optional(T* host, size_t count) {
    T* d = scratch<T>(count);
    if (d && host) down_[ndown_++] = {host, d, count * sizeof(T)};
    return d;
  }
  template <typename T> T* inout(T* host, size_t count) {
    T* d = in(host, count);
    if (d) down_[ndown_++] = {host, d, count * sizeof(T)};
    return d;
  }

  // the device work of the call: launches or a *_dev entry point, returning an rl status
  template <typename F> void run(F&& work) {
    if (rc_ == RL_OK) rc_ = work();
  }
  // the same between the context's two timing events (finish then fills rl_stats.kernel_ms)
  template <typename F> void run_timed(F&& work) {
    if (rc_ == RL_OK) hip(hipEventRecord(ctx_->ev0, ctx_->stream), "hipEventRecord");
    run(work);
    if (rc_ == RL_OK) timed_ = hip(hipEventRecord(ctx_->ev1, ctx_->stream), "hipEventRecord");
  }
  // the queued copies to the host in the order they were registered, one synchronisation, the elapsed time
  int finish(rl_stats* stats = nullptr) {
    for (int i = 0; i < ndown_ && rc_ == RL_OK; ++i)
      hip(hipMemcpyAsync(down_[i].host, down_[i].dev, down_[i].bytes, hipMemcpyDeviceToHost, ctx_->stream), "copy to the host");
    if (rc_ == RL_OK) hip(hipStreamSynchronize(ctx_->stream), "hipStreamSynchronize");
    if (rc_ == RL_OK && timed_ && stats) {
      float ms = 0.f;
      if (hip(hipEventElapsedTime(&ms, ctx_->ev0, ctx_->ev1), "hipEventElapsedTime")) stats->kernel_ms = ms;
    }
    // the stream is idle: the blocks go back at once.  After a failure they stay with their PoolBuf, whose destructor
    // waits for whatever was enqueued before it returns them.
    if (rc_ == RL_OK) for (int i = 0; i < nblk_; ++i) blk_[i].release();
    return rc_;
  }

 private:
  static constexpr int kMaxBlocks = 16;
  struct Down { void* host; const void* dev; size_t bytes; };
  bool hip(hipError_t e, const char* what) {
    if (e != hipSuccess && rc_ == RL_OK) rc_ = fail(RL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return e == hipSuccess;
  }
  rl_ctx* ctx_;
  int rc_ = RL_OK;
  bool timed_ = false;
  int nblk_ = 0, ndown_ = 0;
  PoolBuf<char> blk_[kMaxBlocks];
  Down down_[kMaxBlocks];
};

// Sequential carve-out of the context's scratch arena.  carve() takes the layout as a callable that only calls take(): it runs once to
// measure (integer offsets, null pointers) and, the total reserved, once to hand out.  From then on leaving the scope records `arena_ev` unless end() already has.
struct Arena {
  rl_ctx* ctx; size_t off = 0; bool open = false;   // open: handing out; before, take() only measures
  explicit Arena(rl_ctx* c) : ctx(c) {}
  Arena(const Arena&) = delete;
  ~Arena() { if (open) (void)end(); }
  template <typename T> T* take(size_t count) {
    T* p = open ? reinterpret_cast<T*>(static_cast<char*>(ctx->arena) + off) : nullptr;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  template <typename F> hipError_t carve(F&& layout) {
    layout(*this);   // then: behind the previous user of the arena if that one ran on another stream, the block grown if need be
    hipError_t e = ctx->arena_ev ? hipSuccess : hipEventCreateWithFlags(&ctx->arena_ev, hipEventDisableTiming);
    if (e == hipSuccess && ctx->arena_busy && ctx->arena_stream != ctx->stream) e = hipStreamWaitEvent(ctx->stream, ctx->arena_ev, 0);
    if (e == hipSuccess && off > ctx->arena_cap) {
      if (ctx->arena_busy) e = hipEventSynchronize(ctx->arena_ev);   // the last user, whatever its stream
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);    // nothing in flight may still use the old block
      if (e != hipSuccess) return e;
      if (ctx->arena) (void)hipFree(ctx->arena);
      ctx->arena = nullptr; ctx->arena_cap = 0;
      if ((e = hipMalloc(&ctx->arena, off)) == hipSuccess) ctx->arena_cap = off;
    }
    if (e != hipSuccess) return e;
    off = 0; open = true;
    layout(*this);
    return hipSuccess;
  }
  hipError_t end() {   // record "the arena is free again once everything enqueued so far on the context's stream has run"
    open = false;
    const hipError_t e = hipEventRecord(ctx->arena_ev, ctx->stream);
    if (e == hipSuccess) { ctx->arena_busy = true; ctx->arena_stream = ctx->stream; }
    return e;
  }
};

// The context's stream (g = 0) and the auxiliary streams a call forked from it: join_streams() makes the context's stream
// continue behind everything enqueued on them; every stream is tried once, the first error returned.
inline hipStream_t fork_stream(const rl_ctx* ctx, int g) { return g == 0 ? ctx->stream : ctx->aux_stream[g - 1]; }
inline hipError_t join_streams(rl_ctx* ctx, int n) {
  hipError_t first = hipSuccess;
  for (int g = 1; g < n; ++g) {
    hipError_t e = hipEventRecord(ctx->ev_join[g - 1], fork_stream(ctx, g));
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_join[g - 1], 0);
    if (first == hipSuccess) first = e;
  }
  return first;
}
// After a fork every exit joins and waits for the poll stream if a copy into the pinned buffer may be in flight; the success
// path does both itself and clears the members.  Declared AFTER the Arena, so that the arena's event is recorded behind all of it.
struct StreamFork {
  rl_ctx* ctx; int n = 1; bool polled = false;
  StreamFork(const StreamFork&) = delete;
  ~StreamFork() { (void)join_streams(ctx, n); if (polled) (void)hipStreamSynchronize(ctx->poll_stream); }
};
}  // namespace
