// svsdf_ctx.hpp -- internal state of the C-ABI host layer, shared by its translation units (round 4 split of svsdf_api.hip):
//   svsdf_pipeline.hip  device pipeline of ONE device: launchers, trajectory upload, evaluation, point upload / sort / stripes
//   svsdf_group.hip     in-process multi-GPU group: worker threads, host / RCCL combine
//   svsdf_capi.hip      the C ABI of include/svsdf_c.h for the hot path: contexts, points, evaluation, plan, full callback
//   svsdf_extras.hip    C ABI of the rows around the path: front end, map / mesh helpers, swept outline, L-BFGS driver
// Memory: every device and pinned allocation of the library is a Buf (below) -- the one place that allocates and frees.
// A Buf frees in its destructor, on the device it allocated on, so the context, a CloudPlan and a function's scratch
// release what they hold by going out of scope; no function keeps a list of pointers to free.  Structs that kernels take
// by value (GsipState, AstarDev, FrontMapDev) stay raw views; their owners sit beside them (gs_own, FrontMap).
// Nothing here is part of the public interface.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/svsdf_c.h"
#include "svsdf_launch.hpp"
#include "svsdf_layout.hpp"
#include "svsdf_minco.hpp"
#include "svsdf_traj_host.hpp"

// One host thread per device of an in-process multi-GPU context.
struct Worker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::function<int()> job;
  bool has_job = false, done = true, quit = false;
  int rc = 0;
  Worker() {
    th = std::thread([this] {
      std::unique_lock<std::mutex> lk(m);
      for (;;) {
        cv.wait(lk, [this] { return has_job || quit; });
        if (quit) return;
        std::function<int()> f = std::move(job);
        has_job = false;
        lk.unlock();
        const int r = f();
        lk.lock();
        rc = r;
        done = true;
        cv.notify_all();
      }
    });
  }
  void post(std::function<int()> f) {
    std::lock_guard<std::mutex> lk(m);
    job = std::move(f);
    has_job = true;
    done = false;
    cv.notify_all();
  }
  int wait() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [this] { return done; });
    return rc;
  }
  ~Worker() {
    { std::lock_guard<std::mutex> lk(m); quit = true; cv.notify_all(); }
    if (th.joinable()) th.join();
  }
};

struct svsdf_ctx;

namespace svsdf_impl {

extern thread_local std::string g_last_error;
int fail(svsdf_ctx *ctx, int code, const std::string &msg);

// early return of a failed HIP call through fail(); HIPCHK names the call, HIPCHK_AS names what the caller says
#define HIPCHK_AS(what, expr)                                                                     \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(ctx, SVSDF_ERR_HIP_BASE + (int)e_, std::string(what) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define HIPCHK(expr) HIPCHK_AS(#expr, expr)

// allocations of this library that are live in this process, and their bytes (svsdf_debug_live_allocations)
inline std::atomic<long long> g_live_allocs{0}, g_live_bytes{0};

// Move-only owner of one device (PINNED: pinned host) allocation.  Reads as a T* at its use sites.
template <typename T, bool PINNED = false>
struct Buf {
  T *p = nullptr;
  size_t bytes = 0;
  int dev = 0;   // device that was current at alloc(): the memory is freed there
  Buf() = default;
  Buf(Buf &&o) noexcept : p(o.p), bytes(o.bytes), dev(o.dev) { o.p = nullptr; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) { reset(); p = o.p; bytes = o.bytes; dev = o.dev; o.p = nullptr; }
    return *this;
  }
  ~Buf() { reset(); }
  operator T *() const { return p; }
  T *operator->() const { return p; }
  T *get() const { return p; }   // (where a template or a reinterpret_cast needs the pointer itself)
  void reset() {
    if (!p) return;
    int cur = dev;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    if (PINNED) (void)hipHostFree(p); else (void)hipFree(p);
    if (cur != dev) (void)hipSetDevice(cur);
    p = nullptr;
    --g_live_allocs;
    g_live_bytes -= (long long)bytes;
  }
  // replace with `count` elements (at least one) on the current device; `view`: a raw copy of the new address, for the
  // structs that kernels take by value
  int alloc(svsdf_ctx *ctx, size_t count, T **view = nullptr) { return alloc_bytes(ctx, std::max<size_t>(count, 1) * sizeof(T), view); }
  int alloc_bytes(svsdf_ctx *ctx, size_t n, T **view = nullptr) {   // (for a T with a tail behind it)
    reset();
    if (view) *view = nullptr;
    (void)hipGetDevice(&dev);
    if (PINNED) HIPCHK(hipHostMalloc((void **)&p, n, hipHostMallocDefault));
    else HIPCHK_AS("hipMalloc((void **)p, count * sizeof(T))", hipMalloc((void **)&p, n));   // (dev_alloc's text, kept)
    bytes = n;
    ++g_live_allocs;
    g_live_bytes += (long long)bytes;
    if (view) *view = p;
    return SVSDF_OK;
  }
};
template <typename T> using PinBuf = Buf<T, true>;

// device buffer + pinned mirror, grown together (cap: elements; reserve below it is free)
template <typename T>
struct Staged {
  Buf<T> d;
  PinBuf<T> h;
  size_t cap = 0;
  int reserve(svsdf_ctx *ctx, size_t n) {
    if (n <= cap) return SVSDF_OK;
    cap = 0;
    int rc = d.alloc(ctx, n);
    if (rc == SVSDF_OK) rc = h.alloc(ctx, n);
    if (rc == SVSDF_OK) cap = n;
    return rc;
  }
};

// ---- Front-end state, all of it svsdf_extras.hip's.  The packed buffers are laid out in svsdf_layout.hpp.
// The resident map (svsdf_frontend_set_map) and what belongs to it.  Releasing it is assigning a fresh one.
struct FrontMap {
  bool set = false;
  svsdf::FrontMapDev dev{};                   // what the kernels take: views of the three buffers below + geometry
  Buf<unsigned long long> d_occ, d_free;      // inflated occupancy bitmap, yaw-free table
  Buf<double> d_kt;
  int Z = 0;                                  // layers of the map's grid (the search stays in layer 0)
  // svsdf_astar_search: one device blob (svsdf_layout::astar_layout) that `astar` views; sized for this map at the first
  // search on it
  Buf<unsigned char> d_astar;
  svsdf::AstarDev astar{};
  bool searched = false;                      // the node records hold a search on this map
};
// The device-resident occupancy map (svsdf_map_build_device; svsdf_mapdev.hpp) and the last gather from it.  It lives on a
// multi-device context's first device.  Releasing it is assigning a fresh one.
struct ResidentMap {
  bool set = false;
  int dims[3] = {0, 0, 0};
  double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0}, res = 1.0;
  int sta_threshold = 0;
  size_t n_cloud = 0, cells = 0, occupied = 0, gathered = 0;
  double build_ms = 0.0, gather_ms = 0.0;
  Buf<unsigned char> d_occ;                   // cells bytes, [(i * Y + j) * Z + k]
  Buf<double> d_pts;                          // the last gather: 3 * gathered doubles, ascending unified voxel id
};
// Staging that outlives a map change, grown on demand
struct FrontStaging {
  Staged<double> edges;                       // svsdf_check_sub_sw_collision: svsdf_layout::subsw_layout
  Buf<int> d_flag;                            // ... its hit flags, flag_cap entries, and their host copy
  std::vector<int> h_flag;
  size_t flag_cap = 0;
  Staged<unsigned char> succ;                 // svsdf_astar_successors: svsdf_layout::succ_layout (97 bytes per parent)
  PinBuf<svsdf::AstarState> h_astar;          // pinned: the search state goes up once per search and comes back once per launch
};
// svsdf_swept_outline: the last result, so that the documented query-then-fill protocol runs the extraction once
struct OutlineCache {
  std::vector<double> key, xy;
  std::vector<int> loops;
  svsdf_outline_stats stats{};
  bool valid = false;
};

// Streams come from a process-wide pool and go back to it (svsdf_pipeline.hip, acquire_streams)
struct StreamSet { hipStream_t main = nullptr; hipStream_t batch[svsdf::kMaxBatches] = {}; int slot = -1; };

}  // namespace svsdf_impl

struct svsdf_ctx {
  template <typename T> using Buf = svsdf_impl::Buf<T>;
  template <typename T> using PinBuf = svsdf_impl::PinBuf<T>;
  svsdf_config cfg{};
  int device = 0;
  svsdf_impl::StreamSet streams;              // the set of the process-wide stream pool the two below are copies of
  hipStream_t stream = nullptr;               // main stream: upload, prep, assemble, readback
  hipStream_t bstream[svsdf::kMaxBatches] = {};      // one stream per point batch
  hipEvent_t ev_prep = nullptr, ev_done[svsdf::kMaxBatches] = {};
  svsdf::ShapeParams sp{};
  bool poly_lds = false;             // Polygon: k_solve / k_round run their kPolygonLds variants (edges at the start of LDS)
  Buf<unsigned char> d_poly;         // Polygon: one device blob, svsdf_layout::poly_layout
  std::vector<double> poly_xy;       // Polygon: the outline as given (host copy)
  std::vector<int> poly_loops;       // Polygon: vertices per closed loop (empty: one loop)
  std::string err;

  // points: this rank's shard, Morton-sorted, split into nbatch contiguous batches
  size_t P = 0;
  bool points_set = false;           // svsdf_set_points was called (P may be 0: an obstacle-free window)
  std::vector<long long> shard_idx;  // original index of shard element j
  Buf<double> d_px, d_py;
  int nbatch = 1;
  int bstart[svsdf::kMaxBatches] = {}, bcount[svsdf::kMaxBatches] = {};
  Buf<svsdf::BatchCtl> d_ctl;

  // trajectory
  Buf<svsdf::TrajDev> d_traj;
  svsdf_impl::Staged<double> in;   // staging, device + pinned mirror, laid out by svsdf::TrajInput
  Buf<svsdf::Pose> d_pose;
  Buf<svsdf::Chunk> d_chunks;
  size_t pose_cap = 0;
  // pose tables of scan layers 2 and 3 (k_layer_tables): layer 2's K x 21 poses, layer 3's K x 22 x 21 behind them
  Buf<svsdf::Pose> d_ltab;
  size_t ltab_cap = 0;         // seeds (K) the buffer holds; grown on demand, never per evaluation
  double r_bound = 0.0;    // shape bound radius for the layer-1 chunk pruning (analytic circumradius + offset)
  double r_bound_sampled = 0.0;  // max over a polar grid of |q| - sdf(q): self-check, must not exceed r_bound
  double lipschitz_excess = 0.0; // largest |f(q') - f(q)| - |q' - q| found by the same grid (k_rbound); must be <= 0
  bool lipschitz_ok = true;      // false: the shape SDF is not 1-Lipschitz -> no value-based cull, no anchor bound mode
  double traj_duration = 0.0;
  bool have_duration = false;
  bool host_only = false;  // SVSDF_FLAG_HOST_ONLY: MINCO / callback host logic only, no device
  int N = 0, K = 0;
  int piece_time_mode = 0;     // this trajectory: 0 cumulative form (exactly equivalent here), 1 / 2 faithful chain
  int stats_piece_time = 0;
  int n_cu = 256;
  double wall_clock_khz = 100000.0;   // hipDeviceAttributeWallClockRate: rate of the constant counter of the clock probe

  // ---- The launch plan: what decides which kernels an evaluation launches and how; every choice gives the same bits.
  // (Measured constants that nothing sets are constexprs next to their use in svsdf_pipeline.hip, not fields.)
  // (1) Pinned by the caller: an environment variable read at svsdf_create, or svsdf_set_plan.
  int prune = 1;               // exact chunk pruning in the layer-1 scans (env SVSDF_PRUNE=0: off; same results)
  int G_env = 0, G_late_env = 0;   // env SVSDF_G / SVSDF_G_LATE, svsdf_set_plan(lanes_per_query): a pinned width (0: by rule)
  int want_batches = 0;        // env SVSDF_BATCHES, svsdf_set_plan(batches): > 0 pinned, 0 by rule, -1 measured
  int round_blocks_per_cu = 4;   // k_round: blocks per CU the grid is capped at (its blocks fetch further iterations themselves); env SVSDF_ROUND_BPC
  bool ub_env = false;         // env SVSDF_UB_FULL=0/1/2/3 or svsdf_set_plan(bound_mode) pins the bound mode, otherwise run_pipeline_leaf decides after one evaluation
  int layer_tables = -1;       // -1 by the previous evaluation's solve count, 0 off, 2 layer 2 only, 3 layers 2 and 3 (env SVSDF_LAYER_TABLES; same results)
  int tail_mode = -1;          // fused GSIP tail (k_tail): -1 by the previous evaluation's active counts, -2 off (launch chain only), >= 0 pinned (env SVSDF_TAIL)
  bool tail_duo = true;        // k_tail with one point per wave: both half-waves own the point and share its seed scans (env SVSDF_TAIL_DUO=0: off)
  bool tail_latency = true;    // small launches of k_tail (a wave slot per point at two waves per SIMD) use the instantiation that keeps its ~ 240 VGPRs (env SVSDF_TAIL_LATENCY=0: the 168-VGPR one everywhere; same results)
  bool tail_local = true;      // k_tail from iteration 0 keeps its points' GSIP state and samples in the wave's LDS (env SVSDF_TAIL_LOCAL=0: global arrays)
  bool scan_anchors = true;    // seed scans of k_round / k_tail evaluate the anchors of the circle test's survivors first (ChunkAnchor; env SVSDF_SCAN_ANCHORS=0: off; needs lipschitz_ok; same results)
  bool cull = true, cull2 = true;   // exact culls of provably inactive main points: by the chunk circles; the value-based second one after the table scan (env SVSDF_CULL: 0 neither, 1 the first alone, 2 both)
  bool select_env = false;     // env SVSDF_SELECT_DELTA set select_delta: it then holds in every bound mode
  double select_delta = 0.1;   // k_round: solve the samples whose upper bound is within this of the best one first
  // (2) Decided by rule, from the point set and the first evaluations on it (take_stripe, run_pipeline_leaf).
  int G = 0 /* 0 = by shard size */, G_late = 8;   // lanes per query of the main solve / of the late GSIP iterations (default_lanes)
  // GSIP bound mode as stored (the kernels' MODE, svsdf_plan::bound_mode; in force: bound_mode_of): 0 cheap bound, 1 full --
  // k_round scans every new GSIP sample (seed = tightest layer-1 bound, reused by k_solve) --, 2 lazy -- only the samples in
  // the cheap-bound band are scanned --, 3 anchor -- every third sample scanned, the rest by their Lipschitz bound
  int bound_mode = 0;
  int ub_tune = 0;             // evaluations since the point set changed that took part in the decision (0 or 1)
  double ub_ratio = 0.0;       // GSIP solves / GSIP samples of the deciding (cheap-bound) evaluation
  int an_state = 0;            // anchor trial: 0 decided / idle, 1 next evaluation counts the full mode's table evaluations, 2 the anchor mode's
  int lz_state = 0;            // lazy-scan trial of a small cloud: 0 idle, 1 the next evaluation runs in the lazy mode and is judged by its GSIP solves
  unsigned long long an_full_evals = 0, lz_cheap_solves = 0;   // what each trial compares against
  // batch count of a large shard in the scanning bound modes: chosen by timing real evaluations (any split gives the
  // same bits): 0 idle / done, 1 next evaluation learns the launch plan with one batch, 2.. timing candidate bt_k
  int bt_state = 0, bt_k = 0, bt_rep = 0, bt_ncand = 0, bt_cand[3] = {1, 1, 1};
  double bt_ms[3] = {0, 0, 0}, bt_samples[3] = {0, 0, 0};
  // (3) Learned from the previous evaluation of this point set (finish).  first_iters alone survives a new point set.
  int first_iters = 12, it_done = 0;   // iterations the launch chain enqueues up front (the previous evaluation's count + 1) / enqueued so far in this evaluation
  long long prev_nsolve[svsdf::kMaxIter] = {}, prev_solves = 0;   // solves per GSIP iteration / in all (valid with have_prev_nsolve)
  long long prev_nactive[svsdf::kMaxIter] = {}; // active GSIP points per iteration, up to its tail
  int prev_tail_iter = -1;     // iteration the previous evaluation's tail started at
  bool have_prev_nsolve = false, have_prev_nactive = false;
  int ltab_mode = 0, tail_iter = -1;   // this evaluation, what the plan came to: layer tables built (0 none, 2 / 3 as layer_tables); iteration the fused tail starts at (-1: none)
  bool cull_ok = false;        // this trajectory: duration not stale, slack table valid
  double slack_max = 0.0;      // max over the chunks of the linear continuous-path allowance
  // time-varying robot scale (svsdf_set_scale): the scaled kernels, launch chain only, no culls, every GSIP
  // sample requested
  bool scaled = false;
  svsdf::ScaleDev scale{};

  // per-point / per-sub-query buffers
  Buf<double> d_sdf, d_t;
  Buf<double> d_res_sdf, d_res_t, d_res_gx, d_res_gy;
  svsdf::GsipState gs{};          // what the kernels take: raw views of the arrays that gs_own holds
  struct {
    Buf<int> pt, iter, nsamp, phase, list[2], solve, sq_k;
    Buf<unsigned> req;
    Buf<double> r, theta0, theta_res, sqx, sqy, sqth, sq_ub, sq_sdf, sq_t;
  } gs_own;
  size_t icap = 0;                // interior capacity: entries of the per-interior-point arrays, stride of the sample arrays
  bool icap_fitted = false;       // capacity already fitted to a measured interior count of this point set
  Buf<double> d_block_partials;
  size_t block_partials_cap = 0;  // doubles
  Buf<double> d_sums;             // kOutPartial
  Buf<double> d_out;              // [partial (kOutPartial) | svsdf::EvalCounters]
  PinBuf<double> h_out;           // pinned mirror
  double *h_out_dev = nullptr;    // the same buffer as the device addresses it (k_reduce writes the result there); null: copy
  Buf<unsigned> d_ticket;         // k_reduce: finished-block counter (zero between launches)
  Buf<int> d_nonfinite;
  size_t e_end = 0;

  // front end (row f3; svsdf_extras.hip alone): the resident map, and the staging that outlives it
  svsdf_impl::FrontMap fmap;
  svsdf_impl::FrontStaging fstage;
  svsdf_impl::ResidentMap rmap;     // svsdf_map_build_device (svsdf_extras.hip alone)

  // profiling
  bool profile = false;  // per-launch HIP events (env SVSDF_PROFILE=1 or svsdf_set_profiling)
  bool profile_span = false;     // svsdf_set_profiling(ctx, 3): device_ms only -- the span between the evaluation's first and last event, no per-launch events
  int saved_nbatch = 0;  // svsdf_set_profiling(ctx, 2): the batch split to restore
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<std::pair<size_t, size_t>> refine_events;  // k_solve launches: (start, stop) indices into ev_pool
  std::vector<std::pair<size_t, size_t>> round_events;   // k_round launches
  std::vector<std::pair<size_t, size_t>> tail_events;    // k_tail launches
  svsdf_stats stats{};
  svsdf_launch_rec launches[SVSDF_LAUNCH_REC_CAP];   // launch record of the last evaluation (svsdf_last_launches)
  int n_launches = 0;                                // launches of the last evaluation (beyond the array: counted only)

  // in-process multi-GPU group (svsdf_config::n_devices > 1): this context then owns no device state of its
  // own, only the host-side callback state below; subs[k] is the single-device context of stripe k
  std::vector<svsdf_ctx *> subs;
  std::vector<std::unique_ptr<Worker>> workers;   // one host thread per sub-context
  int combine = 0;                  // SVSDF_COMBINE_HOST / SVSDF_COMBINE_RCCL (resolved)
  std::vector<void *> comms;        // ncclComm_t per sub-context (RCCL combine)
  std::vector<Buf<double>> d_red;   // per sub-context all-reduce output (RCCL combine)
  PinBuf<double> h_red;             // pinned: reduced partial read back from subs[0]
  std::vector<double> comb;         // host-combined [cost | gradC | gradT]
  const double *h_partial = nullptr;  // where the last evaluation's summed partial lives on the host
  double combine_ms = 0.0, setup_ms = 0.0, fanout_ms = 0.0;
  bool group_serial = false;        // svsdf_set_group_serial: the stripes' evaluations one after the other (diagnostic)

  svsdf_impl::OutlineCache outline;   // svsdf_swept_outline's last result
  size_t lds_limit = 65536;         // dynamic LDS a block may ask for on this device
  std::string launch_err;           // a launch that could not be made (LDS budget, shape not compiled); reported by join_batches

  // full-callback state (TrajOptimizer members BEO:44-60)
  svsdf_host::MincoS3 minco;
  std::vector<double> T, pgC, pgT, cm, gC, gradq, gradT, xlast;
  double energy_cost = 0.0;
  double costs3[3] = {0, 0, 0};
};

namespace svsdf_impl {

constexpr size_t kOutPartial = 19 * svsdf::kMaxPieces + 1;
constexpr size_t kOutDoubles = kOutPartial + sizeof(svsdf::EvalCounters) / sizeof(double);   // partial | counters row
// the control block allocation: the batches' BatchCtl, then bytes that nothing addresses (kept: allocation sizes do not change)
constexpr size_t kCtlUnusedTail = 8 * 8 * (svsdf::kMaxIter + 4);
constexpr size_t kCtlBytes = svsdf::kMaxBatches * sizeof(svsdf::BatchCtl) + kCtlUnusedTail;
constexpr int kRepeat = -12345;   // finish(): more interior points than capacity -- the arrays were grown, repeat the evaluation

extern const char *kShapeNames[SVSDF_SHAPE_COUNT];

// ---- The prologue of a device entry point.  A multi-device context owns no device state: its first stripe's context stands in.
inline svsdf_ctx *leaf_of(svsdf_ctx *c) { return c->subs.empty() ? c : c->subs[0]; }
// What an entry that reads the resident cloud needs: a device, and svsdf_set_points before it.
inline int require_resident(svsdf_ctx *ctx) {
  if (ctx->host_only) return fail(ctx, SVSDF_ERR_NO_DEVICE, "host-only context: no device entry points");
  if (!ctx->points_set) return fail(ctx, SVSDF_ERR_NO_POINTS, "svsdf_set_points has not been called");
  return SVSDF_OK;
}
// `body(leaf)` on a context that has a device; the leaf's error string becomes the group's when the body fails on it.
// `name`: the entry point, for "<name>: no device context".
template <typename Body>
int on_device(svsdf_ctx *ctx, const char *name, const Body &body) {
  if (!ctx || ctx->host_only) return fail(ctx, SVSDF_ERR_NO_DEVICE, std::string(name) + ": no device context");
  svsdf_ctx *leaf = leaf_of(ctx);
  if (leaf == ctx) return body(ctx);
  const int r = on_device(leaf, name, body);
  if (r) ctx->err = leaf->err;
  return r;
}

// ---- The plan's helpers.  The bound mode in force: the stored one, except that the anchor mode needs a 1-Lipschitz shape SDF and runs as the full
// mode without one (the only place that demotes).  In force (this function) is what svsdf_get_plan, fill_mode_stats
// (svsdf_stats::gsip_bound_mode), launch_round and launch_tail see; stored (ctx->bound_mode) what enqueue_solve_round's seed
// hand-off (any scanning mode: != 0), run_pipeline_leaf's decision and trials and svsdf_set_plan's change test see.
inline int bound_mode_of(const svsdf_ctx *c) { return (c->bound_mode == 3 && !c->lipschitz_ok) ? 1 : c->bound_mode; }
// Forgetting what the previous evaluation taught: the solve counts (launch widths, layer tables) alone, or with them the active counts (fused tail)
inline void forget_solve_counts(svsdf_ctx *c) { c->have_prev_nsolve = false; }
inline void forget_launch_history(svsdf_ctx *c) { c->have_prev_nsolve = false; c->have_prev_nactive = false; }
inline void stop_trials(svsdf_ctx *c) { c->an_state = 0; c->lz_state = 0; }
// A new point set: nothing learned or decided on the old one holds (a pinned bound mode stays; so does first_iters).
inline void reset_plan(svsdf_ctx *c) {
  forget_launch_history(c); stop_trials(c);
  c->prev_tail_iter = -1; c->ub_tune = 0; c->bt_state = 0; c->ub_ratio = 0.0;
  if (!c->ub_env) c->bound_mode = 0;
}
// nothing left to decide, try or measure, and the launch widths are on record (svsdf_plan::settled, svsdf_stats::plan_settled)
inline bool plan_settled(const svsdf_ctx *c) { return (c->ub_env || c->ub_tune > 0) && !c->bt_state && !c->an_state && !c->lz_state && c->have_prev_nsolve; }
inline bool valid_lanes(int g) { return g == 1 || g == 2 || g == 4 || g == 8 || g == 16 || g == 32; }
// Interior points up to which the fused tail owns the whole GSIP loop and a cheap-bound cloud tries the lazy mode: one generation of waves (6144 on 256 CUs)
inline long long tail_interior_limit(const svsdf_ctx *c) { return (long long)c->n_cu * 24; }
// Lanes per query of the main solve by shard size: small shards are latency chains (wide groups shorten them), large ones
// throughput (narrow groups waste fewer lanes; the descent's ladders share the wave anyway).  Crossovers re-measured in
// round 4 after the shared ladders (profiles/r04_lanes_sweep.txt: 100 k points 8 -> 4 lanes - 5 %, 200 k 8 -> 2 lanes - 7 %).
// (Polygon: never below 4 -- its 2-lane kernel spills under the 3-waves register cap.)
inline int default_lanes(const svsdf_ctx *ctx, size_t Ps) {
  const int g = (Ps < 3000) ? 32 : (Ps < 20000) ? 16 : (Ps < 75000) ? 8 : (Ps < 150000) ? 4 : 2;
  return (ctx->cfg.shape_id == (int)svsdf::kPolygon) ? std::max(g, 4) : g;
}

// ---- svsdf_pipeline.hip
// Streams come from a process-wide pool and go back to it (round 5).  A context used to create its 9 streams and destroy
// them with itself; the NEXT context of the process then ran its concurrent point batches 7 % slower -- same kernels, same
// plan, same serialised times (tools/state_probe.py: a workload after any destroyed context 7.6 - 7.7 ms, beside a live
// one or in a fresh process 7.1 ms): the runtime maps streams to hardware queues when they are created and tears the
// queues down with the last stream, so the second generation of streams overlaps differently.  Pooled streams are created
// once per device in a fixed order and never destroyed: every context that is alone on its device gets set 0, i.e. the
// stream-to-queue mapping of a fresh process.
// Limits: (a) the "fresh process" mapping holds for a context that is ALONE on its device -- two live contexts
// get sets 0 and 1; (b) the pool is process-wide static state and its streams are never destroyed, so it must not be
// relied on across hipDeviceReset(): acquire_streams probes a pooled set with hipStreamQuery and re-creates a dead one,
// which covers a reset BETWEEN contexts, not one under a live context (that invalidates the context itself).
bool acquire_streams(int device, StreamSet &out);
void release_streams(int device, StreamSet &s);
int set_batches(svsdf_ctx *ctx, int nb);
int choose_tail_iter(const svsdf_ctx *ctx);
int swept_field(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, double *sdf_sorted);
int evaluate_points(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, bool allow_cull, bool with_partial);
void fill_mode_stats(svsdf_ctx *ctx);
// launch record: a fresh one per evaluation, one entry per launch (plain stores into the context's fixed array);
// null when the array is full
inline void reset_launches(svsdf_ctx *ctx) { ctx->n_launches = 0; }
inline svsdf_launch_rec *record_launch(svsdf_ctx *ctx, int kernel, int shape, unsigned grid, unsigned block, size_t lds,
                                       long long work, int batch) {
  if (ctx->n_launches >= SVSDF_LAUNCH_REC_CAP) { ++ctx->n_launches; return nullptr; }   // beyond the array: counted only
  svsdf_launch_rec *r = &ctx->launches[ctx->n_launches++];
  *r = svsdf_launch_rec{};
  r->struct_size = (int)sizeof(svsdf_launch_rec);
  r->kernel = kernel; r->shape = shape; r->grid = grid; r->block = block; r->lds_bytes = lds; r->work = work; r->batch = batch;
  return r;
}
int compiled_shape(int shape);
int run_pipeline_leaf(svsdf_ctx *ctx, int N, const double *coeffs, const double *T);
void accumulate(int N, const double *partial, double *cost, double *gradT, double *gradC);
void shard_plan(const double *xyz, size_t P, int rk, int ws, int flags, std::vector<long long> &out);
struct CloudPlan {
  const double *d_xyz = nullptr;
  size_t P = 0;
  Buf<double> d_part;
  Buf<unsigned long long> d_keys, d_keys2;
  const unsigned long long *sorted = nullptr;
  Buf<unsigned char> d_tmp;
};
int plan_cloud(svsdf_ctx *ctx, const double *d_xyz, size_t P, CloudPlan &plan);
int take_stripe(svsdf_ctx *ctx, svsdf_ctx *planner, const CloudPlan &plan, int rk, int ws);
int upload_shard_device(svsdf_ctx *ctx, const double *d_xyz, size_t P, int rk, int ws);
long long sincos_mismatches(svsdf_ctx *ctx, double lo, double hi, int n);
long long sqrt_mismatches(svsdf_ctx *ctx, const double *x, size_t n, int flavour);
int debug_sdf_at(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, size_t n, const double *pxy, const double *t, double *out8);
int site_stats(svsdf_ctx *ctx, unsigned long long out[20]);
// What a trajectory upload is for.  An evaluation (svsdf_debug_sdf_at included) updates the persistent traj_duration, notes
// the piece-time statistic and records the k_prep launch.  A probe (svsdf_min_clearance, which has refused 300 s and more)
// takes the trajectory's own duration and leaves those three alone; it still overwrites N, K, the cull fields (slack_max,
// cull_ok), piece_time_mode, ltab_mode, the staging block and the device tables -- every evaluation rewrites all of these.
enum class TrajUse { evaluation, probe };
int upload_traj(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, TrajUse use, bool clear_nonfinite = false);
// ---- svsdf_clearance.hip
int min_clearance_leaf(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, const svsdf_clearance_params &prm,
                       svsdf_clearance_result *out);
int point_clearance_leaf(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, const svsdf_point_clearance_params &prm,
                         double *lower, double *upper, double *t_witness, unsigned char *state, svsdf_point_clearance_result *out);
// ---- svsdf_group.hip
int upload_group_device(svsdf_ctx *ctx, const double *d_xyz, size_t P);
int group_run(svsdf_ctx *ctx, const std::function<int(int)> &f);
void merge_stats(svsdf_ctx *ctx);
int run_pipeline(svsdf_ctx *ctx, int N, const double *coeffs, const double *T);   // leaf or group
int set_points_host(svsdf_ctx *ctx, const double *xyz, size_t P);
std::string group_init_rccl(svsdf_ctx *g);
svsdf_ctx *create_group(const svsdf_config *cfg, int ndev);
void destroy_group_resources(svsdf_ctx *ctx);
int rccl_comm_count(const svsdf_ctx *ctx);

}  // namespace svsdf_impl
