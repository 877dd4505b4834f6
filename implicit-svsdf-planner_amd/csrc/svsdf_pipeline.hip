// svsdf_pipeline.hip -- device pipeline of ONE device behind the C ABI (include/svsdf_c.h): kernel dispatch, launchers,
// trajectory upload (SweptVolumeManager::updateTraj, SWM:376-385), one evaluation of
// addSaftyPenaOnSweptVolumeParallelTrueSDF (BEO:774-869) as a chain of launches per point batch, launch-plan rules, and
// the query-point upload (sort, stripes).  This translation unit also compiles the shape-independent kernels of
// svsdf_kernels.hpp (SVSDF_API_TU); the shape-templated ones live in svsdf_shape_slice.hip.
#include <hipcub/hipcub.hpp>

#define SVSDF_API_TU
#include "svsdf_ctx.hpp"

using namespace svsdf;

namespace svsdf_impl {

thread_local std::string g_last_error;

int fail(svsdf_ctx *ctx, int code, const std::string &msg) {
  g_last_error = msg;
  if (ctx) ctx->err = msg;
  return code;
}

const char *kShapeNames[SVSDF_SHAPE_COUNT] = {
    "sdUnevenCapsule", "sdCutDisk", "sdTrapezoid", "sdRhombus", "star", "sdTunnel",
    "sdHorseshoe", "sdHeart", "sdOrientedVesica", "sdRoundedCross", "sdRoundedX", "bigX",
    "sdMoon", "sdPie", "sdPie2", "sdArc", "Polygon"};
inline uint32_t part1by1(uint32_t x) {
  x &= 0x0000ffff;
  x = (x ^ (x << 8)) & 0x00ff00ff;
  x = (x ^ (x << 4)) & 0x0f0f0f0f;
  x = (x ^ (x << 2)) & 0x33333333;
  x = (x ^ (x << 1)) & 0x55555555;
  return x;
}

// process-wide stream pool (svsdf_ctx.hpp): per device, sets of 1 + kMaxBatches non-blocking streams
namespace {
struct PoolEntry { StreamSet set; bool in_use = false; };
std::mutex g_pool_mutex;
std::vector<std::vector<PoolEntry>> g_pool;   // [device][slot]
}  // namespace

bool acquire_streams(int device, StreamSet &out) {
  std::lock_guard<std::mutex> lk(g_pool_mutex);
  if (device < 0) return false;
  if ((size_t)device >= g_pool.size()) g_pool.resize((size_t)device + 1);
  std::vector<PoolEntry> &pool = g_pool[(size_t)device];
  for (size_t k = 0; k < pool.size(); ++k)
    if (!pool[k].in_use) {   // lowest free slot first
      // A pooled set outlives its contexts on purpose (never destroyed: see svsdf_ctx.hpp) -- but not a hipDeviceReset(),
      // after which its handles dangle.  An idle stream answers hipStreamQuery with success; anything but
      // success / not-ready means the handle is dead: the slot gets a fresh set, in the same fixed order.
      bool alive = true;
      {
        const hipError_t q = hipStreamQuery(pool[k].set.main);
        if (q != hipSuccess && q != hipErrorNotReady) { alive = false; (void)hipGetLastError(); }
      }
      if (!alive) {
        StreamSet fresh;
        fresh.slot = (int)k;
        bool ok = hipStreamCreateWithFlags(&fresh.main, hipStreamNonBlocking) == hipSuccess;
        for (int b = 0; b < kMaxBatches && ok; ++b) ok = hipStreamCreateWithFlags(&fresh.batch[b], hipStreamNonBlocking) == hipSuccess;
        if (!ok) return false;
        pool[k].set = fresh;
      }
      pool[k].in_use = true; out = pool[k].set; return true;
    }
  PoolEntry e;
  e.set.slot = (int)pool.size();
  bool ok = hipStreamCreateWithFlags(&e.set.main, hipStreamNonBlocking) == hipSuccess;
  for (int b = 0; b < kMaxBatches && ok; ++b) ok = hipStreamCreateWithFlags(&e.set.batch[b], hipStreamNonBlocking) == hipSuccess;
  if (!ok) {
    if (e.set.main) (void)hipStreamDestroy(e.set.main);
    for (int b = 0; b < kMaxBatches; ++b) if (e.set.batch[b]) (void)hipStreamDestroy(e.set.batch[b]);
    return false;
  }
  e.in_use = true;
  pool.push_back(e);
  out = e.set;
  return true;
}

void release_streams(int device, StreamSet &s) {
  std::lock_guard<std::mutex> lk(g_pool_mutex);
  if (device >= 0 && (size_t)device < g_pool.size() && s.slot >= 0 && (size_t)s.slot < g_pool[(size_t)device].size())
    g_pool[(size_t)device][(size_t)s.slot].in_use = false;
  s = StreamSet{};
}

// SVSDF_DEBUG_SYNC=1 (diagnosis only): every launch of the chain is followed by a stream synchronisation and named on stderr
// BEFORE it runs, so that a device fault (which aborts the process at the next synchronisation) is pinned to one launch.
static bool debug_sync_on() { static const bool on = [] { const char *e = std::getenv("SVSDF_DEBUG_SYNC"); return e && std::atoi(e) != 0; }(); return on; }
static void debug_sync(hipStream_t st, const char *what, int a, int b) {
  if (!debug_sync_on()) return;
  std::fprintf(stderr, "[svsdf] launched %s (%d, %d) ... ", what, a, b);
  const hipError_t e = hipStreamSynchronize(st);
  std::fprintf(stderr, "%s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
}

size_t next_event(svsdf_ctx *ctx) {
  if (ctx->ev_used == ctx->ev_pool.size()) {
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    ctx->ev_pool.push_back(e);
  }
  return ctx->ev_used++;
}

// ---- kernel dispatch over the shape id: the shape-templated kernels live in four translation units
// (svsdf_shape_slice.hip, shapes with id % 4 == slice); a development build (-DSVSDF_FAST_BUILD) holds only star /
// sdHorseshoe / sdHeart / Polygon and serves every other id with the Polygon kernels
#define SVSDF_SLICE_DISPATCH(NAME, ...)                      \
  switch (shape % kNSlices) {                                \
    case 0: return NAME##_s0(shape, __VA_ARGS__);            \
    case 1: return NAME##_s1(shape, __VA_ARGS__);            \
    case 2: return NAME##_s2(shape, __VA_ARGS__);            \
    default: return NAME##_s3(shape, __VA_ARGS__);           \
  }
int compiled_shape(int shape) {
#ifdef SVSDF_FAST_BUILD
  return (shape == 4 || shape == 6 || shape == 7 || shape == kPolygonLds) ? shape : 16;
#else
  return shape;
#endif
}
}  // namespace svsdf_impl
namespace svsdf {
bool launch_k_solve(int shape, int G, unsigned grid, unsigned block, size_t lds, hipStream_t st, const SolveLaunch &a) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_solve, G, grid, block, lds, st, a)
}
bool launch_k_round(int shape, int lp, int mode, unsigned grid, size_t lds, hipStream_t st, const RoundLaunch &a) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_round, lp, mode, grid, lds, st, a)
}
bool launch_k_classify(int shape, unsigned grid, size_t lds, hipStream_t st, const ClassifyLaunch &a) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_classify, grid, lds, st, a)
}
bool launch_k_tail(int shape, int mode, unsigned grid, size_t lds, hipStream_t st, const TailLaunch &a) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_tail, mode, grid, lds, st, a)
}
bool launch_k_rbound(int shape, unsigned grid, hipStream_t st, ShapeParams sp, double rmax, int nrad, int nang, double *out) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_rbound, grid, st, sp, rmax, nrad, nang, out)
}
bool launch_k_subsw(int shape, dim3 grid, hipStream_t st, ShapeParams sp, const double *father, const double *child,
                    const unsigned long long *offs, const double *pts, const double *kt, int nkt, int *flag) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_subsw, grid, st, sp, father, child, offs, pts, kt, nkt, flag)
}
bool launch_k_debug_sdf_at(int shape, unsigned grid, size_t lds, hipStream_t st, const TrajDev *traj, ShapeParams sp,
                           const double *pxy, const double *t, int n, double *out, const ScaleDev *scl) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_debug_sdf_at, grid, lds, st, traj, sp, pxy, t, n, out, scl)
}
bool launch_k_shape_kernels(int shape, unsigned grid, hipStream_t st, ShapeParams sp, int ks, int count, double resu,
                            int size_side, double safemargin, const double *yaw, unsigned char *map) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_shape_kernels, grid, st, sp, ks, count, resu, size_side, safemargin, yaw, map)
}
bool launch_k_succ(int shape, unsigned grid, hipStream_t st, ShapeParams sp, const FrontMapDev &fm, const int *parent_ij,
                   const double *parent_yaw, double *yaw_out, unsigned char *stage_out) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_succ, grid, st, sp, fm, parent_ij, parent_yaw, yaw_out, stage_out)
}
bool launch_k_astar(int shape, hipStream_t st, ShapeParams sp, const FrontMapDev &fm, const AstarDev &a, int slice) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_astar, st, sp, fm, a, slice)
}
bool launch_k_clr(int shape, unsigned grid, size_t lds, hipStream_t st, const ClrLaunch &a) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_clr, grid, lds, st, a)
}
bool launch_k_pclr(int shape, unsigned grid, size_t lds, hipStream_t st, const PclrLaunch &a) {
  shape = svsdf_impl::compiled_shape(shape);
  SVSDF_SLICE_DISPATCH(launch_k_pclr, grid, lds, st, a)
}
void launch_k_pack_kernel_rows(hipStream_t st, const unsigned char *map, int ks, int count, unsigned long long *rows) {
  hipLaunchKernelGGL(k_pack_kernel_rows, dim3((unsigned)((ks * count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, map, ks,
                     count, rows);
}
void launch_k_yaw_free(hipStream_t st, const unsigned long long *occ, int row_words, const unsigned long long *krows, int ks,
                       int count, int X, int Y, unsigned long long *free_out) {
  const size_t lds = ((size_t)ks * kYawFreeRowWords + (size_t)ks * count) * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_yaw_free, dim3((unsigned)X, (unsigned)((Y + kYawFreeBlock - 1) / kYawFreeBlock)), dim3(kYawFreeBlock),
                     lds, st, occ, row_words, krows, ks, count, X, Y, free_out);
}
}  // namespace svsdf
namespace svsdf_impl {

// Brackets a launch with a pair of profile events and appends the pair to `list`; nothing without per-launch profiling.
struct ProfileSpan {
  svsdf_ctx *ctx; hipStream_t st; std::vector<std::pair<size_t, size_t>> &list; size_t e0 = 0;
  ProfileSpan(svsdf_ctx *c, hipStream_t s, std::vector<std::pair<size_t, size_t>> &l) : ctx(c), st(s), list(l) {
    if (ctx->profile) { e0 = next_event(ctx); (void)hipEventRecord(ctx->ev_pool[e0], st); }
  }
  ~ProfileSpan() {
    if (ctx->profile) { const size_t e1 = next_event(ctx); (void)hipEventRecord(ctx->ev_pool[e1], st); list.emplace_back(e0, e1); }
  }
};
// a launch that could not be made leaves its text in launch_err (the first one stays; join_batches reports it)
static void launch_result(svsdf_ctx *ctx, bool launched, const char *kernel) {
  if (!launched && ctx->launch_err.empty()) ctx->launch_err = std::string(kernel) + ": shape not compiled into this build";
}
static void lds_too_long(svsdf_ctx *ctx, const std::string &what) {
  if (ctx->launch_err.empty()) ctx->launch_err = "trajectory too long for the LDS pose table (" + what + ")";
}
// GSIP selection of k_round / k_tail: band `sel` below the best bound, every sample from iteration `all_it` on.
// The seed bound of the scanning modes is the sample's own table minimum and tight: a narrow band selects (kScanDelta,
// solve-all from iteration 7); the cheap mode's chunk bound needs 0.1 m / iteration 5.  SVSDF_SELECT_DELTA sets every mode's band.
struct GsipSelect { double sel; int all_it; };
static GsipSelect gsip_select(const svsdf_ctx *ctx, int mode) {
  // round 6 sweep, 0 ... 0.01: sdHeart / anchor mode - 3.5 % at 0.001 - 0.002 m -- 7 % fewer solves --, C3 / NS / C5 / C2 within +- 0.5 %; 0.01 m until round 5
  constexpr double kScanDelta = 0.002; constexpr int kAllIterCheap = 5, kAllIterScans = 7;
  const bool scans = mode != 0;
  return {(scans && !ctx->select_env) ? kScanDelta : ctx->select_delta, scans ? kAllIterScans : kAllIterCheap};
}

// Dynamic LDS of one block (svsdf::block_table_doubles): the tables -- a Polygon's edges in front of them while the block
// still fits, else the kernel variant that reads the edges from global memory (`fall_back`) -- and behind them, 16-byte
// aligned, `per_wave` bytes of state for each wave of the block.  k_solve's block size is chosen here, from the table bytes
// (`block`); k_tail's is fixed.  k_round stages no trajectory, has no per-wave state and < 16 KB of static tables that count
// against the block's budget.
enum class TableUser { Solve, Round, Tail };
struct BlockLds { size_t bytes = 0; int block = 0; bool poly_lds = false, fits = false; };
static BlockLds plan_block_lds(const svsdf_ctx *ctx, TableUser user, size_t per_wave, bool poly_lds, bool fall_back = true) {
  BlockLds r;
  for (r.poly_lds = poly_lds;; r.poly_lds = false) {
    const size_t lds = block_table_doubles(ctx->K, ctx->N, r.poly_lds ? (size_t)svsdf::kPolyEdgeDoubles * (size_t)ctx->sp.nverts : 0,
                                           user != TableUser::Round) * sizeof(double);
    r.block = (user == TableUser::Solve) ? (((lds + per_wave) * 12 <= 160 * 1024) ? 64 : ((lds + 2 * per_wave) * 6 <= 160 * 1024) ? 128 : 256)
              : (user == TableUser::Tail) ? kTailBlock : kRoundBlock;
    r.bytes = (user == TableUser::Round) ? lds : ((lds + 15) & ~(size_t)15) + (size_t)(r.block / 64) * per_wave;
    r.fits = r.bytes + (user == TableUser::Round ? 16384 : 0) <= ctx->lds_limit;
    if (r.fits || !r.poly_lds || !fall_back) return r;
  }
}
// k_tail: a wave's state, with the wave-local copy of the GSIP state or without
static size_t tail_wave_bytes(bool local) { return local ? kTailWaveLds : kTailWaveLds - kTailLocalBytes; }

// Persistent-grid launcher of the argmin kernel.  max_queries bounds the (possibly device-side)
// query count and sizes the grid; surplus blocks exit before touching LDS.
void launch_solve(svsdf_ctx *ctx, int G, hipStream_t st, const QuerySet &qs, long long max_queries, double *out_sdf,
                  double *out_t, BatchCtl *ctl, int work_idx,
                  double cull_thresh = std::numeric_limits<double>::infinity()) {
  const TrajInput in(ctx->in.d, ctx->N, ctx->K);
  if (ctx->scaled) {
    // the scaled path (§4c): its widths only, and no cull -- both culls bound the rigid map, not the scaled descent's value
    G = scaled_lanes(G);
    cull_thresh = std::numeric_limits<double>::infinity();
  }
  // a launch of at most one query per SIMD with 32-lane groups (the main solve of a reference-scale cloud): one query per
  // wave, so that the descents take the fused pass (k_solve, kSolveSolo)
  const bool solo = G == 32 && !ctx->G_env && max_queries <= (long long)ctx->n_cu * 4;
  const long long lanes = std::max<long long>(max_queries * (solo ? 64 : G), 64);
  // Every block stages the pose table + chunk bounds + trajectory into LDS (13 KB at 16 pieces x 2.5 s, 24 KB at 32):
  // with one wave per block that caps the CU at 160 KB / lds waves -- 6 at C3, half of what the kernel's 141 VGPRs
  // allow (3 waves per SIMD) -- so the block grows until LDS no longer binds (measured at C3: 10.7 -> 9.2 ms).
  // A Polygon's edges go in front of the tables while the whole block still fits the device's per-block LDS; a long
  // trajectory (large pose table) falls back to the kernel variant that reads the edges from global memory.
  const size_t wlds = ladder_lds_bytes(G);   // per wave: the descent state of its 64 / G groups
  const BlockLds l = plan_block_lds(ctx, TableUser::Solve, wlds, ctx->poly_lds);
  const int blk = l.block;
  if (!l.fits) return lds_too_long(ctx, std::to_string(l.bytes) + " B of " + std::to_string(ctx->lds_limit) + " B per block");
  constexpr int kSolveGridWaves = 256 * 16;   // the persistent grid's cap: 16 waves for each of 256 CUs
  const unsigned grid = (unsigned)std::min<long long>((lanes + blk - 1) / blk, (long long)(kSolveGridWaves * 64) / blk);
  // (the second, value-based cull runs with the first one: main points of an evaluation that may cull)
  const bool cull2 = std::isfinite(cull_thresh) && ctx->cull2;
  const SolveLaunch a{ctx->d_traj, in.tk(), ctx->d_pose, ctx->d_chunks, ctx->sp, qs, out_sdf, out_t, (ctx->prune ? kSolvePrune : 0) | (solo ? kSolveSolo : 0) | (ctx->ltab_mode >= 2 ? kSolveLayer2 : 0) | (ctx->ltab_mode >= 3 ? kSolveLayer3 : 0), ctl, work_idx, cull_thresh,
                      cull2 ? in.rot() : nullptr, ctx->slack_max, ctx->scaled ? &ctx->scale : nullptr, ctx->d_ltab};
  const int shape = l.poly_lds ? (int)kPolygonLds : ctx->cfg.shape_id;
  {
    const ProfileSpan span(ctx, st, ctx->refine_events);
    launch_result(ctx, launch_k_solve(shape, G, grid, (unsigned)blk, l.bytes, st, a), "k_solve");
    if (svsdf_launch_rec *r = record_launch(ctx, ctx->scaled ? SVSDF_KERNEL_SOLVE_SCALED : SVSDF_KERNEL_SOLVE, compiled_shape(shape), grid, (unsigned)blk, l.bytes, max_queries,
                                            (int)(ctl - ctx->d_ctl))) {
      r->targ[0] = G; r->targ[1] = 1; r->iter = work_idx; r->solo = solo ? 1 : 0;
    }
    debug_sync(st, "k_solve", G, work_idx);
  }
  ctx->stats.solve_launches++;
}

void launch_round(svsdf_ctx *ctx, hipStream_t st, int b, int it) {
  const int mode = bound_mode_of(ctx);   // k_round MODE: cheap / full / lazy / anchor bound
  const long long pts = std::max(1, ctx->bcount[b]);
  const BlockLds l = plan_block_lds(ctx, TableUser::Round, 0, ctx->poly_lds);
  if (!l.fits) return lds_too_long(ctx, "k_round");
  // late iterations hold few points and are latency-bound: request every sample there, which
  // avoids supplementary iterations at no cost in time
  const GsipSelect gsel = gsip_select(ctx, mode);
  // the scaled path (§4c) requests every sample in every iteration: the bounds are values of the RIGID table, and a scaled
  // solve from a rigid seed is bounded by none of them
  const double delta = (it >= gsel.all_it || ctx->scaled) ? 1e300 : gsel.sel;
  const double band_delta = (it >= gsel.all_it || ctx->scaled) ? 1e300 : ctx->select_delta;   // lazy mode: cheap-bound band that gets scanned
  // iterations 0 and 1 are (almost always) GSIP rounds 1 and 2 with 2 and 6 samples: 8 lanes per point; later rounds have
  // 18-21 samples: 32 lanes per point (either handles any count).  Iteration 2 (18 samples, still every interior point
  // active: throughput, not latency) also runs faster with 8 lanes and three sample passes per point -- measured round 3,
  // 8 lanes in the first 2 / 3 / 4 / 6 / all iterations: C3 6.15 / 5.97 / 6.12 / 6.33 / 6.45 ms, NS 7.49 / 7.24 / 7.21 / 7.31 / 7.58
  // (round 6, re-measured with the balanced launches: 2 / 3 / 4 / 6 iterations -- C3 5.80 / 5.63 / 5.67 / 5.87 ms, C4 6.26 / 5.84 /
  // 5.88 / 6.00; the lazy mode, whose launches scan few samples per point, gains from a fourth: NS 7.45 / 7.17 / 7.03 / 7.05)
  constexpr int kRoundLp8Iters = 3;
  const int lp = (it < kRoundLp8Iters + (mode == 2 ? 1 : 0)) ? 8 : 32;
  const unsigned grid = (unsigned)std::min<long long>((pts * lp + kRoundBlock - 1) / kRoundBlock, (long long)ctx->n_cu * ctx->round_blocks_per_cu);
  const RoundLaunch a{ctx->d_traj, ctx->d_pose, ctx->d_chunks, ctx->sp, ctx->d_px, ctx->d_py, ctx->gs, ctx->icap, it, delta,
                      band_delta, ctx->d_res_sdf, ctx->d_res_t, ctx->d_res_gx, ctx->d_res_gy, ctx->d_ctl + b, kListScans | kListCheap | ((ctx->scan_anchors && ctx->lipschitz_ok) ? kScanAnchors : 0)};
  const int shape = l.poly_lds ? (int)kPolygonLds : ctx->cfg.shape_id;
  const ProfileSpan span(ctx, st, ctx->round_events);
  launch_result(ctx, launch_k_round(shape, lp, mode, grid, l.bytes, st, a), "k_round");
  if (svsdf_launch_rec *r = record_launch(ctx, SVSDF_KERNEL_ROUND, compiled_shape(shape), grid, (unsigned)kRoundBlock, l.bytes, pts, b)) {
    r->targ[0] = lp; r->targ[1] = mode; r->iter = it; r->anchors = (a.clist_on & kScanAnchors) ? 1 : 0;
  }
  debug_sync(st, "k_round", lp * 10 + mode, it);
}

// k_tail: every GSIP iteration of batch b from `it0` on, in one launch (two points per wave, solved in the wave).
void launch_tail(svsdf_ctx *ctx, hipStream_t st, int b, int it0) {
  const int mode = bound_mode_of(ctx);
  const GsipSelect gsel = gsip_select(ctx, mode);
  constexpr int kTailAllAfter = 1 << 30;   // steps of a point inside k_tail after which every sample is requested: never
  // the active count lives on the device; the grid is sized by what the previous evaluation had there (surplus blocks
  // exit at once, missing ones are made up for by the waves' work fetch)
  long long pts = std::max(1, ctx->bcount[b]);
  if (ctx->have_prev_nactive && it0 <= ctx->prev_tail_iter && it0 < kMaxIter)
    pts = std::min<long long>(pts, ctx->prev_nactive[it0] / std::max(1, ctx->nbatch) * 5 / 4 + 64);
  // the wave-local copy of the GSIP state only where it is used: the whole loop in the tail (it0 == 0) with the switch on;
  // when it does not fit, the state stays in global memory (same bits) -- that goes first, then the Polygon's edges
  bool local = ctx->tail_local && it0 == 0;
  BlockLds l = plan_block_lds(ctx, TableUser::Tail, tail_wave_bytes(local), ctx->poly_lds, !local);
  if (!l.fits && local) {
    local = false;
    l = plan_block_lds(ctx, TableUser::Tail, tail_wave_bytes(false), ctx->poly_lds);
  }
  if (!l.fits) return lds_too_long(ctx, "k_tail");
  // one point per wave while that still fits the chip's wave slots (3 per SIMD): the launch is a latency chain then
  const int ppw = (pts <= (long long)ctx->n_cu * 12) ? 1 : 2;
  const long long per_block = (kTailBlock / 64) * ppw;
  const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((pts + per_block - 1) / per_block, (long long)ctx->n_cu * 3));
  const TailLaunch a{ctx->d_traj, TrajInput(ctx->in.d, ctx->N, ctx->K).tk(), ctx->d_pose, ctx->d_chunks, ctx->sp, ctx->d_px, ctx->d_py, ctx->gs, ctx->icap, it0, mode,
                     gsel.sel, ctx->select_delta, kTailAllAfter, ppw, ctx->d_res_sdf, ctx->d_res_t, ctx->d_res_gx, ctx->d_res_gy,
                     ctx->d_ctl + b, kListScans | kListCheap | (local ? kTailLocalState : 0) | (ctx->tail_duo ? 0 : kTailNoDuo) | ((ctx->scan_anchors && ctx->lipschitz_ok) ? kScanAnchors : 0), ctx->prune ? kSolvePrune : 0,
                     // a wave slot for every point at two waves per SIMD: the instantiation without scratch (k_tail, kTailLatencyWaves)
                     (ctx->tail_latency && ppw == 1 && pts <= (long long)ctx->n_cu * 4 * svsdf::kTailLatencyWaves) ? 1 : 0};
  const int shape = l.poly_lds ? (int)kPolygonLds : ctx->cfg.shape_id;
  {
    const ProfileSpan span(ctx, st, ctx->tail_events);
    launch_result(ctx, launch_k_tail(shape, mode, grid, l.bytes, st, a), "k_tail");
    if (svsdf_launch_rec *r = record_launch(ctx, SVSDF_KERNEL_TAIL, compiled_shape(shape), grid, (unsigned)kTailBlock, l.bytes, pts, b)) {
      r->targ[0] = mode; r->targ[1] = a.latency ? svsdf::kTailLatencyWaves : SVSDF_TAIL_WAVES; r->iter = it0; r->points_per_wave = ppw;
      r->local_state = (a.clist_on & kTailLocalState) ? 1 : 0; r->duo = (ppw == 1 && !(a.clist_on & kTailNoDuo)) ? 1 : 0; r->anchors = (a.clist_on & kScanAnchors) ? 1 : 0;
    }
    debug_sync(st, "k_tail", mode, it0);
  }
  ctx->stats.tail_launches++;
}

// Iteration the fused tail starts at in this evaluation.  Measured (round 4, profiles/r04_tail_*): the launch chain packs the
// solves of all points 32 to a wave and runs k_round at 4 waves per SIMD -- once a launch holds more points than the chip
// keeps in flight it has several times the tail's throughput, and its last launches take 5 - 50 us each, so placing the tail
// late in the chain of a 100 k - 1 M cloud only costs time (C2 + 6 %, C3 + 2 %, NS + 3 % with a threshold of 4096 points).
// A small cloud is a pure latency chain of ~ 20 launches: there the WHOLE GSIP loop runs in the tail (it0 = 0), as long as
// its interior points fit one generation of waves (two per wave, 12 waves per CU: 6144 on this part).  C1 workload, chain
// -> tail: 3 k points 0.68 -> 0.54 ms, 10 k (4.7 k interior) 0.89 -> 0.71, 13 k (6.1 k) 0.93 -> 0.75, 20 k (9.4 k) 1.09 ->
// 1.06, 30 k (14 k) 1.24 -> 1.56 (tools/tail_scan.py).  SVSDF_TAIL / svsdf_set_plan pin an iteration or turn the tail
// off.  Any choice gives the same bits.
int choose_tail_iter(const svsdf_ctx *ctx) {
  if (ctx->tail_mode == -2 || ctx->scaled) return -1;   // (the scaled path runs the launch chain only, §4c)
  //  a trajectory whose tables leave no room for the tail's per-wave state runs the launch chain, which needs
  // less LDS per block, instead of failing the evaluation (128 pieces on a device with 64 KB per block)
  if (!plan_block_lds(ctx, TableUser::Tail, tail_wave_bytes(false), false).fits) return -1;
  if (ctx->tail_mode >= 0) return std::min(ctx->tail_mode, (int)kMaxIter - 2);
  if (!ctx->have_prev_nactive) return -1;   // first evaluation of a point set: the interior count is not known yet
  return (ctx->prev_nactive[0] <= tail_interior_limit(ctx)) ? 0 : -1;
}

void launch_classify(svsdf_ctx *ctx, hipStream_t st, int b) {
  const unsigned grid = (unsigned)std::min<long long>(((long long)ctx->bcount[b] + kBlock - 1) / kBlock, 2048);
  const size_t lds = (size_t)traj_lds_doubles(ctx->N) * sizeof(double);
  const ClassifyLaunch a{ctx->d_traj, ctx->sp, ctx->d_px, ctx->d_py, ctx->d_sdf, ctx->d_t, ctx->d_res_sdf, ctx->d_res_t,
                         ctx->d_res_gx, ctx->d_res_gy, ctx->gs, ctx->d_ctl + b, &ctx->d_ctl->n_int, (int)ctx->icap,
                         ctx->scaled ? &ctx->scale : nullptr};
  launch_result(ctx, launch_k_classify(ctx->cfg.shape_id, grid, lds, st, a), "k_classify");
  (void)record_launch(ctx, ctx->scaled ? SVSDF_KERNEL_CLASSIFY_SCALED : SVSDF_KERNEL_CLASSIFY, compiled_shape(ctx->cfg.shape_id), grid,
                      (unsigned)kBlock, lds, ctx->bcount[b], b);
  debug_sync(st, "k_classify", b, 0);
}

// Upload (coeffs, T) and build what the kernels read beside them (svsdf_traj_host.hpp): the layer-1 time grid, the exact
// cull's table, the piece-time mode; then k_prep.  An evaluation updates traj_duration first (SWM:376-385).
int upload_traj(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, TrajUse use, bool clear_nonfinite) {
  const svsdf_traj::TrajCheck chk = svsdf_traj::check_traj(N, coeffs, T);
  if (chk.code) return fail(ctx, chk.code, chk.reason);
  if (use == TrajUse::evaluation) svsdf_traj::update_duration(chk.td, ctx->traj_duration, ctx->have_duration);
  const double td = chk.td, dur = (use == TrajUse::probe) ? td : ctx->traj_duration;
  if (!(dur / 0.15 < 16002.0)) return fail(ctx, SVSDF_ERR_INVALID, "trajectory duration out of range for the scan table");
  const size_t room = TrajInput::doubles(N, (int)svsdf_traj::scan_times_room(dur));   // (sized before the grid is counted: it is written as it is counted)
  if (room > ctx->in.cap)
    if (int rc = ctx->in.reserve(ctx, room + 4096)) return rc;
  double *const tk = TrajInputRW(ctx->in.h, N, 0).tk();   // (tk starts behind coeffs and T, whatever K)
  const size_t K = svsdf_traj::scan_times(dur, tk);
  if (K < 1 || K > 16000) return fail(ctx, SVSDF_ERR_INVALID, "trajectory duration out of range for the scan table");
  if (K > ctx->pose_cap) {
    if (int rc = ctx->d_pose.alloc(ctx, K + 1024)) return rc;
    // chunk records, then the anchor table (ChunkAnchor, k_prep)
    if (int rc = ctx->d_chunks.alloc(ctx, 2 * ((K + 1024) / kChunk + 2))) return rc;
    ctx->pose_cap = K + 1024;
  }
  const TrajInputRW in(ctx->in.h, N, (int)K);
  std::memcpy(in.coeffs(), coeffs, sizeof(double) * 18 * N);
  std::memcpy(in.T(), T, sizeof(double) * N);
  const std::vector<double> S = svsdf_traj::prefix_sums(N, T);
  const svsdf_traj::CullTable cull = svsdf_traj::cull_table(N, coeffs, S.data(), tk, K, dur, td, (size_t)kChunk, in.slack(), in.rot());
  ctx->slack_max = cull.slack_max; ctx->cull_ok = cull.ok;
  ctx->piece_time_mode = svsdf_traj::piece_time_mode(ctx->cfg.flags, N, T, dur);
  if (use == TrajUse::evaluation) ctx->stats_piece_time = ctx->piece_time_mode;
  ctx->N = N; ctx->K = (int)K;
  HIPCHK(hipMemcpyAsync(ctx->in.d, ctx->in.h, TrajInput::doubles(N, (int)K) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const size_t lds = (size_t)traj_lds_doubles(N) * sizeof(double);
  // one block of 1024 threads (round 6; 256 before): a pose per thread for the ~ 600 poses of a reference-scale trajectory
  // instead of three one after the other, and four waves per SIMD to hide the chain's latencies behind
  hipLaunchKernelGGL(k_prep, dim3(1), dim3(1024), lds, ctx->stream, ctx->in.d, N, dur, (int)K, ctx->piece_time_mode, ctx->d_traj,
                     ctx->d_pose, ctx->d_chunks, ctx->r_bound, ctx->d_ctl, ctx->nbatch, clear_nonfinite ? ctx->d_nonfinite : nullptr);
  if (use == TrajUse::evaluation) (void)record_launch(ctx, SVSDF_KERNEL_PREP, -1, 1, 1024, lds, (long long)K, 0);
  ctx->ltab_mode = 0;   // (the tables on the device belong to the previous trajectory: build_layer_tables)
  return SVSDF_OK;
}

// Pose tables of scan layers 2 and 3 for this evaluation's argmin solves (k_layer_tables; main stream, after k_prep and
// before the batches fork).  A solve reads 2 x 21 poses from them instead of computing them; building them costs
// K x 23 x 21 pose evaluations and a launch.  Rule (plan field layer_tables, env SVSDF_LAYER_TABLES pin it): build when the
// poses the solves save are at least 16 times the poses the tables hold, with the solve count of the previous
// evaluation of this point set (the point count before there is one) -- 184 K solves, 98 k at 32 pieces, where the
// launch is ~ 2 % of the evaluation.  A reference-scale callback (hundreds of points) never builds them.
int build_layer_tables(svsdf_ctx *ctx) {
  int mode = ctx->layer_tables;
  const size_t K = (size_t)ctx->K;
  if (mode < 0) {
    const long long solves = ctx->have_prev_nsolve ? ctx->prev_solves : (long long)ctx->P;
    mode = (solves * 2 * svsdf::kLayerSteps >= 16ll * (long long)K * svsdf::kLayerRows * svsdf::kLayerSteps) ? 3 : 0;
  }
  if (ctx->cfg.shape_id == (int)svsdf::kPolygon) mode = 0;   // the Polygon kernels compute every layer (descend_from_seed)
  if (mode == 0) return SVSDF_OK;
  if (K > ctx->ltab_cap) {
    const size_t cap = K + 256;
    ctx->ltab_cap = 0;
    int rc = ctx->d_ltab.alloc(ctx, cap * (size_t)svsdf::kLayerRows * svsdf::kLayerSteps);
    if (rc) return rc;
    ctx->ltab_cap = cap;
  }
  const int rows = (mode >= 3) ? svsdf::kLayerRows : 1;
  const size_t lds = (size_t)traj_lds_doubles(ctx->N) * sizeof(double);
  const unsigned grid = (unsigned)((K * (size_t)rows * svsdf::kLayerSteps + 255) / 256);
  hipLaunchKernelGGL(k_layer_tables, dim3(grid), dim3(256), lds, ctx->stream, ctx->d_traj, TrajInput(ctx->in.d, ctx->N, ctx->K).tk(), (int)K, rows, ctx->d_ltab);
  if (svsdf_launch_rec *r = record_launch(ctx, SVSDF_KERNEL_LAYER_TABLES, -1, grid, 256, lds, (long long)(K * rows * svsdf::kLayerSteps), 0)) r->targ[0] = mode;
  ctx->ltab_mode = mode;
  return SVSDF_OK;
}


// The stream batch b's chain runs on: its own, or -- with a single batch -- the main stream (round 5: a one-batch evaluation
// used to hop main -> batch -> main through two events, ~12 us each on the device timeline; a reference-scale callback is
// ~20 launches of a few us)
hipStream_t batch_stream(const svsdf_ctx *ctx, int b) { return ctx->nbatch > 1 ? ctx->bstream[b] : ctx->stream; }

int join_batches(svsdf_ctx *ctx) {
  if (!ctx->launch_err.empty()) {   // a launch that could not be made: a clear error instead of a raw HIP launch failure
    const std::string m = ctx->launch_err;
    ctx->launch_err.clear();
    for (int b = 0; b < ctx->nbatch; ++b) (void)hipStreamSynchronize(batch_stream(ctx, b));
    return fail(ctx, SVSDF_ERR_INVALID, m);
  }
  if (ctx->nbatch > 1)
    for (int b = 0; b < ctx->nbatch; ++b) {
      HIPCHK(hipEventRecord(ctx->ev_done[b], ctx->bstream[b]));
      HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_done[b], 0));
    }
  HIPCHK(hipGetLastError());
  return SVSDF_OK;
}

// GSIP pipeline per batch:  R0 S0 R1 S1 ... S(k-1) Rk   with
//   R_i = k_round(i): close the rounds whose samples S_(i-1) solved, open the next ones, select
//   S_i = k_solve over the samples R_i selected.
// enqueue_solve_round(i) enqueues S_i then R_(i+1).
void enqueue_solve_round(svsdf_ctx *ctx, int it, bool tail_next = false) {
  for (int b = 0; b < ctx->nbatch; ++b) {
    hipStream_t st = batch_stream(ctx, b);
    BatchCtl *ctl = ctx->d_ctl + b;
    QuerySet q{};
    q.qx = ctx->gs.sqx; q.qy = ctx->gs.sqy; q.count_ptr = &ctl->n_solve[it];
    q.slots = ctx->gs.solve + (size_t)ctx->bstart[b] * kMaxSlots; q.n_outer = 1;
    if (ctx->bound_mode != 0) { q.seed_k = ctx->gs.sq_k; q.seed_d = ctx->gs.sq_ub; }   // (the stored mode: any scanning mode leaves seeds)
    // G_late from iteration kLateIter on without counts on record; with them, the iteration's solves below which the groups widen to 32 / 16 / 8 lanes
    constexpr int kLateIter = 4; constexpr long long kWide32Below = 2000, kWide16Below = 5000, kWide8Below = 40000;
    int G = (it >= kLateIter) ? ctx->G_late : ctx->G;
    // Successive callbacks of one optimisation see almost the same trajectory: iteration `it` of the previous
    // evaluation tells how many solves this launch will hold.  Few solves = a latency-bound launch (<= ~1 wave per
    // SIMD): widen the groups to shorten the dependent chain; many solves = throughput: keep the shard's width even
    // in late iterations.  Any width gives the same bits, so a wrong guess only costs time.
    if (!ctx->G_env && !ctx->G_late_env && ctx->have_prev_nsolve) {
      const long long n = ctx->prev_nsolve[it];   // summed over the batches: they run this iteration concurrently
      G = std::max(ctx->G, n < kWide32Below ? 32 : n < kWide16Below ? 16 : n < kWide8Below ? 8 : 1);
    }
    launch_solve(ctx, G, st, q, (long long)ctx->bcount[b] * kMaxSlots, ctx->gs.sq_sdf, ctx->gs.sq_t, ctl, it + 1);
    if (tail_next) launch_tail(ctx, st, b, it + 1);
    else launch_round(ctx, st, b, it + 1);
  }
}

// What every evaluation starts from: no profile events in use, fresh statistics and a fresh launch record.
static void begin_evaluation(svsdf_ctx *ctx) {
  ctx->ev_used = 0;
  ctx->refine_events.clear(); ctx->round_events.clear(); ctx->tail_events.clear();
  ctx->stats = svsdf_stats{}; ctx->stats.points = ctx->P;
  reset_launches(ctx);
}
// The main points of batch b as a query set: the resident cloud itself, one query per point.
static QuerySet main_queries(const svsdf_ctx *ctx, int b) {
  QuerySet qm{};   // (no stride, no count on the device, no list)
  qm.qx = ctx->d_px; qm.qy = ctx->d_py; qm.count_fixed = ctx->bcount[b]; qm.base = ctx->bstart[b]; qm.n_outer = 1;
  return qm;
}
// Enqueue the device pipeline up to the per-point results of getTrueSDFofSweptVolume (res_*).
// No host synchronisation: batches run on their own streams, joined back onto ctx->stream.
int enqueue_queries(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, bool allow_cull) {
  if (int rc = require_resident(ctx)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  begin_evaluation(ctx);
  const size_t e_begin = next_event(ctx);
  (void)hipEventRecord(ctx->ev_pool[e_begin], ctx->stream);
  int rc = upload_traj(ctx, N, coeffs, T, TrajUse::evaluation, /*clear_nonfinite=*/true);   // (k_prep also clears the non-finite counter)
  if (rc) return rc;
  if ((rc = build_layer_tables(ctx))) return rc;
  const bool fork = ctx->nbatch > 1;   // one batch: the whole chain stays on the main stream (no cross-stream hand-offs)
  if (fork) HIPCHK(hipEventRecord(ctx->ev_prep, ctx->stream));
  const int m = ctx->tail_iter = choose_tail_iter(ctx);
  for (int b = 0; b < ctx->nbatch; ++b) {
    hipStream_t st = batch_stream(ctx, b);
    BatchCtl *ctl = ctx->d_ctl + b;
    if (fork) HIPCHK(hipStreamWaitEvent(st, ctx->ev_prep, 0));
    const QuerySet qm = main_queries(ctx, b);
    const double cull_thresh = (allow_cull && ctx->cull && ctx->cull_ok) ? ctx->cfg.safety_hor + 1e-9 : std::numeric_limits<double>::infinity();
    launch_solve(ctx, ctx->G, st, qm, ctx->bcount[b], ctx->d_sdf, ctx->d_t, ctl, 0, cull_thresh);
    launch_classify(ctx, st, b);
    if (m == 0) launch_tail(ctx, st, b, 0);
    else launch_round(ctx, st, b, 0);
  }
  if (m >= 0) {
    // launch chain up to iteration m, everything after it in k_tail: nothing is ever left pending
    for (int it = 0; it < m; ++it) enqueue_solve_round(ctx, it, it == m - 1);
    ctx->it_done = kMaxIter + 1;   // (an index whose pending-solve count is always zero)
  } else {
    for (int it = 0; it < ctx->first_iters; ++it) enqueue_solve_round(ctx, it);
    ctx->it_done = ctx->first_iters;
  }
  return join_batches(ctx);
}

// The swept-volume implicit function alone: getSDFofSweptVolume<false,true> (SWM:844-866) = min over t of the shape SDF,
// for every resident point, in the sorted shard order -- the main solve without cull, classification and GSIP rounds
// (svsdf_swept_outline: the zero set only needs the sign and a Lipschitz value next to it).
int swept_field(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, double *sdf_sorted) {
  if (int rc = require_resident(ctx)) return rc;
  if (ctx->P == 0) return SVSDF_OK;
  HIPCHK(hipSetDevice(ctx->device));
  begin_evaluation(ctx);
  int rc = upload_traj(ctx, N, coeffs, T, TrajUse::evaluation);
  if (rc) return rc;
  if ((rc = build_layer_tables(ctx))) return rc;
  if (ctx->nbatch > 1) HIPCHK(hipEventRecord(ctx->ev_prep, ctx->stream));
  for (int b = 0; b < ctx->nbatch; ++b) {
    hipStream_t st = batch_stream(ctx, b);
    if (ctx->nbatch > 1) HIPCHK(hipStreamWaitEvent(st, ctx->ev_prep, 0));
    launch_solve(ctx, ctx->G, st, main_queries(ctx, b), ctx->bcount[b], ctx->d_sdf, ctx->d_t, ctx->d_ctl + b, 0);
  }
  rc = join_batches(ctx);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(sdf_sorted, ctx->d_sdf, ctx->P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVSDF_OK;
}

// assemble + reduce + k_finish on the main stream, one D2H of [partial | counters], sync.
int reduce_and_read(svsdf_ctx *ctx, bool with_partial) {
  const int N = ctx->N;
  bool host_written = false;
  if (with_partial) {
    const unsigned grid = (unsigned)std::min<size_t>((ctx->P + kBlock - 1) / kBlock, 512);   // (256 / 1024 / 2048 blocks: within 1 %, round 6)
    const size_t plen = (size_t)partial_doubles(N);
    if ((size_t)grid * plen > ctx->block_partials_cap) {
      int rc = ctx->d_block_partials.alloc(ctx, (size_t)grid * plen);
      if (rc) return rc;
      ctx->block_partials_cap = (size_t)grid * plen;
    }
    // one accumulator row per wave; a cloud that fits ONE block keeps its points' terms in LDS instead (assemble_body)
    const size_t lds = ((size_t)traj_lds_doubles(N) + std::max<size_t>((kBlock / 64) * plen, grid == 1 ? svsdf::assemble_small_doubles(N) : 0)) * sizeof(double);
    if (lds > ctx->lds_limit)   // (98 KB at 128 pieces: fits gfx950's 160 KB; a clear error instead of a raw launch failure elsewhere)
      return fail(ctx, SVSDF_ERR_INVALID, "trajectory too long for the reduction's LDS accumulator rows (" + std::to_string(lds) + " B of " +
                  std::to_string(ctx->lds_limit) + " B per block)");
    // small clouds (<= 1024 points): assembly, block reduction, fixed-order final sum, suffix sum and counters in ONE
    // launch whose last block writes the result to the device buffer and straight into the pinned host buffer (k_reduce);
    // larger ones: the assembly, then k_final (one wave per entry) and k_finish as launches of their own
    const int fuse = grid <= 4 ? 1 : 0;
    with_scale(ctx->scaled ? &ctx->scale : nullptr, [&](auto... scl) {   // scaled: the position gradient under S(t*) (§4c)
      hipLaunchKernelGGL((k_reduce<decltype(scl)...>), dim3(grid), dim3(kBlock), lds, ctx->stream, ctx->d_traj, ctx->d_px, ctx->d_py,
                         (int)ctx->P, ctx->d_res_sdf, ctx->d_res_t, ctx->d_res_gx, ctx->d_res_gy,
                         ctx->cfg.safety_hor, ctx->cfg.weight_p, ctx->d_block_partials, ctx->d_nonfinite, ctx->d_out,
                         ctx->d_ctl, ctx->nbatch, ctx->it_done, (int)kOutPartial, (int)kOutDoubles, ctx->d_ticket, ctx->h_out_dev, fuse,
                         scl...);
    });
    if (svsdf_launch_rec *r = record_launch(ctx, ctx->scaled ? SVSDF_KERNEL_REDUCE_SCALED : SVSDF_KERNEL_REDUCE, -1, grid, (unsigned)kBlock, lds,
                                            (long long)ctx->P, 0)) r->fused = fuse;
    if (!fuse) {
      hipLaunchKernelGGL(k_final, dim3((unsigned)plen), dim3(64), 0, ctx->stream, ctx->d_block_partials, (int)grid, ctx->d_sums);
      (void)record_launch(ctx, SVSDF_KERNEL_FINAL, -1, (unsigned)plen, 64, 0, (long long)grid, 0);
      hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->d_sums, N, ctx->d_out, ctx->d_ctl,
                         ctx->nbatch, ctx->it_done, ctx->d_nonfinite,
                         reinterpret_cast<unsigned long long *>(ctx->d_out + kOutPartial), ctx->h_out_dev, (int)kOutDoubles);
      (void)record_launch(ctx, SVSDF_KERNEL_FINISH, -1, 1, (unsigned)kBlock, 0, 0, 0);
    }
    host_written = ctx->h_out_dev != nullptr;
  } else {
    HIPCHK(hipMemsetAsync(ctx->d_sums, 0, kOutPartial * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->d_sums, N, ctx->d_out, ctx->d_ctl,
                       ctx->nbatch, ctx->it_done, ctx->d_nonfinite,
                       reinterpret_cast<unsigned long long *>(ctx->d_out + kOutPartial), ctx->h_out_dev, (int)kOutDoubles);
    (void)record_launch(ctx, SVSDF_KERNEL_FINISH, -1, 1, (unsigned)kBlock, 0, 0, 0);
    host_written = ctx->h_out_dev != nullptr;
  }
  ctx->e_end = next_event(ctx);
  (void)hipEventRecord(ctx->ev_pool[ctx->e_end], ctx->stream);
  if (!host_written) HIPCHK(hipMemcpyAsync(ctx->h_out, ctx->d_out, kOutDoubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  return SVSDF_OK;
}

int alloc_interior_buffers(svsdf_ctx *ctx, size_t cap);   // below

// Finish an evaluation: reduce, read back, and -- rare slow path -- run more GSIP iterations when
// some points needed more than `first_iters` (rounds + supplementary solves), then reduce again.
int finish(svsdf_ctx *ctx, bool with_partial) {
  int rc = reduce_and_read(ctx, with_partial);
  if (rc) return rc;
  const EvalCounters &cnt = *reinterpret_cast<const EvalCounters *>(ctx->h_out + kOutPartial);
  while (cnt.pending > 0 && ctx->it_done < kMaxIter) {  // solves requested by the last k_round are pending
    const int it1 = std::min(ctx->it_done + 3, (int)kMaxIter);
    for (int it = ctx->it_done; it < it1; ++it) enqueue_solve_round(ctx, it);
    ctx->it_done = it1;
    if ((rc = join_batches(ctx))) return rc;
    HIPCHK(hipMemsetAsync(ctx->d_nonfinite, 0, sizeof(int), ctx->stream));
    if ((rc = reduce_and_read(ctx, with_partial))) return rc;
  }
  if (cnt.pending > 0) return fail(ctx, SVSDF_ERR_INVALID, "GSIP iterations exhausted (internal limit)");
  {
    const size_t n_int = (size_t)cnt.n_int;
    if (n_int > ctx->icap) {   // surplus interior points were dropped: grow and repeat (same bits once everything fits)
      rc = alloc_interior_buffers(ctx, std::min(ctx->P, n_int + n_int / 8 + 4096));
      return rc ? rc : kRepeat;
    }
    if (!ctx->icap_fitted && ctx->P >= 100000 && ctx->icap > 2 * (n_int + n_int / 8 + 4096)) {
      // first evaluation of a large cloud: give back what the interior count does not need (contents are per evaluation)
      rc = alloc_interior_buffers(ctx, n_int + n_int / 8 + 4096);
      if (rc) return rc;
    }
    ctx->icap_fitted = true;
  }
  ctx->stats.solves = cnt.solves;
  ctx->stats.sdf_evals = cnt.sdf_evals;
  ctx->stats.scan_evals = cnt.scan_evals;
  ctx->stats.interior_points = cnt.interior_points;
  ctx->stats.gsip_samples = cnt.gsip_samples;
  ctx->stats.gsip_iterations = (unsigned)cnt.gsip_iterations;
  ctx->stats.culled_points = cnt.culled_points;
  ctx->stats.round_scan_evals = cnt.round_scan_evals;
  ctx->stats.speculative_evals = cnt.speculative_evals;
  ctx->stats.batches = ctx->nbatch;
  {
    const unsigned long long c = cnt.clk[0], r = cnt.clk[1];   // clock probe (BatchCtl::clk)
    ctx->stats.shader_clock_mhz = r ? (double)c / (double)r * ctx->wall_clock_khz * 1e-3 : 0.0;
  }
  for (int i = 0; i < kMaxIter; ++i) ctx->prev_nsolve[i] = (long long)cnt.n_solve[i];
  ctx->prev_solves = (long long)cnt.solves;
  ctx->have_prev_nsolve = true;
  for (int i = 0; i < kMaxIter; ++i) ctx->prev_nactive[i] = (long long)cnt.n_active[i];
  ctx->prev_tail_iter = ctx->tail_iter;
  ctx->have_prev_nactive = true;
  ctx->stats.tail_iter = ctx->tail_iter;
  ctx->stats.tail_points = (ctx->tail_iter >= 0 && ctx->tail_iter < kMaxIter) ? cnt.n_active[ctx->tail_iter] : 0ull;
  // next evaluation enqueues as many iterations as this one needed (+1); the slow path above
  // covers an underestimate
  if (ctx->tail_iter < 0) ctx->first_iters = std::max(2, std::min((int)cnt.gsip_iterations + 1, (int)kMaxIter));
  if (ctx->profile_span || ctx->profile) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev_pool[0], ctx->ev_pool[ctx->e_end]);
    ctx->stats.device_ms = ms;
  }
  if (ctx->profile) {
    // k_solve time of the evaluation: the point batches run concurrently on their own streams, so the launches'
    // [start, stop] intervals (device clock, relative to the evaluation's first event) are merged -- solve_ms is the
    // time during which at least one k_solve launch was executing, solve_ms_sum the plain sum of the launch durations
    // (what a kernel trace adds up)
    auto merged = [&](const std::vector<std::pair<size_t, size_t>> &evs, double &uni, double &sum) {
      sum = 0.0;
      std::vector<std::pair<float, float>> iv;
      for (const auto &pr : evs) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, ctx->ev_pool[0], ctx->ev_pool[pr.first]) == hipSuccess &&
            hipEventElapsedTime(&b, ctx->ev_pool[0], ctx->ev_pool[pr.second]) == hipSuccess && b >= a) {
          iv.emplace_back(a, b);
          sum += b - a;
        }
      }
      std::sort(iv.begin(), iv.end());
      uni = 0.0;
      float cur_a = 0.f, cur_b = -1.f;
      for (const auto &x : iv) {
        if (x.first > cur_b) { if (cur_b >= cur_a) uni += cur_b - cur_a; cur_a = x.first; cur_b = x.second; }
        else cur_b = std::max(cur_b, x.second);
      }
      if (cur_b >= cur_a) uni += cur_b - cur_a;
    };
    merged(ctx->refine_events, ctx->stats.solve_ms, ctx->stats.solve_ms_sum);
    merged(ctx->round_events, ctx->stats.round_ms, ctx->stats.round_ms_sum);
    merged(ctx->tail_events, ctx->stats.tail_ms, ctx->stats.tail_ms_sum);
  }
  if (cnt.nonfinite) return fail(ctx, SVSDF_ERR_NONFINITE, "non-finite per-point result on the device");
  return SVSDF_OK;
}


// One evaluation up to the per-point results (and the partial): enqueue, finish.
int evaluate_points(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, bool allow_cull, bool with_partial) {
  for (int attempt = 0; attempt < 3; ++attempt) {
    int rc = enqueue_queries(ctx, N, coeffs, T, allow_cull);
    if (rc) return rc;
    rc = finish(ctx, with_partial);
    if (rc != kRepeat) return rc;   // kRepeat: the interior arrays were too small and have been grown
  }
  return fail(ctx, SVSDF_ERR_INVALID, "interior capacity could not be settled (internal error)");
}

void fill_mode_stats(svsdf_ctx *ctx) {
  ctx->stats.gsip_bound_mode = bound_mode_of(ctx);
  ctx->stats.piece_time_exact = ctx->stats_piece_time;
  ctx->stats.bound_mode_decided = (ctx->ub_env || ctx->ub_tune > 0) ? 1 : 0;
  ctx->stats.plan_settled = plan_settled(ctx) ? 1 : 0;
  ctx->stats.bound_ratio = ctx->ub_ratio;
  ctx->stats.n_devices = 1;
  ctx->stats.combine = SVSDF_COMBINE_HOST;
  ctx->stats.combine_ms = 0.0;
  ctx->stats.setup_ms = ctx->setup_ms;
}

// Whole device pipeline of ONE device; leaves [cost, gradC, gradT] (19N+1 doubles) in d_out / h_out.
int run_pipeline_leaf(svsdf_ctx *ctx, int N, const double *coeffs, const double *T) {
  if (int rc = require_resident(ctx)) return rc;
  if (ctx->P == 0) {
    // an obstacle-free window (or an empty stripe): the reference's loop over parallel_points_num == 0 adds
    // nothing (BEO:785) and the callback returns energy + rho * sum(T).  The trajectory is still validated and
    // traj_duration updated (SWM:376-385); the partial is zero on the host and on the device (collectives).
    const svsdf_traj::TrajCheck chk = svsdf_traj::check_traj(N, coeffs, T);
    if (chk.code) return fail(ctx, chk.code, chk.reason);
    svsdf_traj::update_duration(chk.td, ctx->traj_duration, ctx->have_duration);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(ctx->d_out, 0, kOutDoubles * sizeof(double), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memset(ctx->h_out, 0, kOutDoubles * sizeof(double));
    ctx->N = N;
    ctx->stats = svsdf_stats{};
    reset_launches(ctx);
    fill_mode_stats(ctx);
    ctx->h_partial = ctx->h_out;
    return SVSDF_OK;
  }
  // GSIP upper-bound mode.  The cheap bound (8 table poses of the nearest chunk) is enough for some shapes (star:
  // a quarter of the samples get solved, full scans only add work), useless for others (sdHorseshoe: 87 % of the
  // samples land in the selection band; with the sample's own table scan as the bound 5.3 -> 1.4 solves per
  // point, 2.4x overall).  Both modes return the same bits, so the choice only costs time.  Rule (deterministic,
  // one evaluation): the first evaluation after a new point set runs with the cheap bound; if it had to solve
  // more than half of the GSIP samples it emitted, every later evaluation scans.  (Round 1 timed three
  // evaluations per mode with the wall clock; the rule reproduces its choices on C1-C5 without the five extra
  // evaluations and without depending on the box.)
  const bool deciding = !ctx->ub_env && ctx->ub_tune == 0;
  if (deciding) { ctx->bound_mode = 0; stop_trials(ctx); }
  // Anchor trial (full-scan shapes only): one evaluation in the full mode and one in the anchor mode, compared by their
  // table-evaluation COUNTERS (deterministic: no timing) -- the anchor mode stays when it saves at least 28 % of them
  // (sdHeart - 32 %: k_round - 27 %, evaluation - 12 %; Polygon - 25 %: a wash; sdHorseshoe - 10 %: + 5 %, its extra passes
  // cost more than the skipped scans; profiles/r04_anchor_ab.txt).  Both modes return the same bits.
  const int an_trial = (ctx->ub_env || ctx->saved_nbatch > 0) ? 0 : ctx->an_state;
  // (pending only in the full / anchor pair: started from a decision for mode 1, stopped by whatever stores another mode)
  if (an_trial == 1) ctx->bound_mode = 1;
  if (an_trial == 2) ctx->bound_mode = 3;
  // Lazy trial (round 5; small clouds of a cheap-bound shape only, see the deciding block below): this evaluation runs in
  // the lazy mode and is judged by its GSIP solve COUNT against the cheap bound's (deterministic, no timing).
  const int lz_trial = (ctx->ub_env || ctx->saved_nbatch > 0) ? 0 : ctx->lz_state;
  if (lz_trial == 1) ctx->bound_mode = 2;
  // Batch count (DESIGN.md "concurrent point batches").  Default: a RULE -- 3 batches from 80 k points per device, 1 below
  // (round 5; rounds 3 - 4: from 400 k in a scanning mode only; what the measurements -- 1 / 2 / 3 / 4 at NS, C3, C4 and at
  // 60 k ... 500 k points -- chose on every box; with the main stream that is at most 4 streams, the HIP runtime's default
  // number of hardware queues) -- so that the plan is the same on every run and settled after the deciding evaluation.  svsdf_set_plan
  // (batches = -1) / SVSDF_BATCHES=measure ask for a measurement instead: after one evaluation that learns the launch
  // widths, every candidate count (1, 4 [2 in the lazy mode], 3) runs three evaluations, timed with HIP events on the
  // library's own stream (device time, not the host's wall clock), and the best median stays.  Every count computes the
  // same bits.  While svsdf_set_profiling(ctx, 2) holds the batches serialised, nothing is measured or changed.
  int rc = SVSDF_OK;
  const bool timing = ctx->bt_state >= 2 && ctx->saved_nbatch == 0;
  if (timing) rc = set_batches(ctx, ctx->bt_cand[ctx->bt_k]);
  if (rc == SVSDF_OK) rc = evaluate_points(ctx, N, coeffs, T, /*allow_cull=*/true, /*with_partial=*/true);
  if (rc == SVSDF_OK && ctx->bt_state == 1 && ctx->saved_nbatch == 0) {
    ctx->bt_state = 2;
    ctx->bt_k = 0;
    ctx->bt_rep = 0;
  } else if (rc == SVSDF_OK && timing) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev_pool[0], ctx->ev_pool[ctx->e_end]);
    ctx->bt_samples[ctx->bt_rep++] = ms;
    if (ctx->bt_rep == 3) {
      std::sort(ctx->bt_samples, ctx->bt_samples + 3);
      ctx->bt_ms[ctx->bt_k] = ctx->bt_samples[1];
      ctx->bt_rep = 0;
      if (++ctx->bt_k == ctx->bt_ncand) {
        int best = 0;
        for (int k = 1; k < ctx->bt_ncand; ++k)
          if (ctx->bt_ms[k] < ctx->bt_ms[best]) best = k;
        rc = set_batches(ctx, ctx->bt_cand[best]);
        ctx->bt_state = 0;
      }
    }
  }
  if (rc == SVSDF_OK && an_trial == 1) {
    ctx->an_full_evals = ctx->stats.round_scan_evals;
    ctx->an_state = 2;
  } else if (rc == SVSDF_OK && an_trial == 2) {
    const bool keep = (double)ctx->stats.round_scan_evals <= 0.72 * (double)ctx->an_full_evals;
    if (!keep) { forget_launch_history(ctx); ctx->bound_mode = 1; }   // (the plan on record is the anchor mode's)
    ctx->an_state = 0;
  }
  const unsigned long long main_solves = ctx->stats.points - ctx->stats.culled_points;   // (gs: the GSIP solves of this evaluation)
  const unsigned long long gs = ctx->stats.solves > main_solves ? ctx->stats.solves - main_solves : 0ull;
  if (lz_trial == 1) {
    const bool keep = rc == SVSDF_OK && (double)gs <= 0.76 * (double)ctx->lz_cheap_solves;
    if (!keep) ctx->bound_mode = 0;
    forget_solve_counts(ctx);   // (the widths on record belong to the deciding evaluation / to the rejected mode; the interior count stands)
    ctx->lz_state = 0;
  }
  if (rc == SVSDF_OK && deciding) {
    ctx->ub_ratio = ctx->stats.gsip_samples ? (double)gs / (double)ctx->stats.gsip_samples : 0.0;
    // Polygon: an SDF evaluation costs several times an analytic shape's (candidate edges of the outline), a table
    // scan proportionally less of a solve, so scanning pays from a lower ratio
    const double thr = ctx->cfg.shape_id == SVSDF_SHAPE_Polygon ? 0.2 : 0.5;
    // below the threshold a large shard still gains from scanning -- but only the samples the cheap bound would have
    // had solved (lazy mode: NS, star / 16 pieces / 1 M points, 12.3 -> 11.4 ms; at 100 k points no gain)
    ctx->bound_mode = (ctx->ub_ratio > thr) ? 1 : (ctx->P >= 400000) ? 2 : 0;
    // A SMALL cloud of a cheap-bound shape (round 5): when the fused tail owns the whole GSIP loop (choose_tail_iter: at most
    // 24 interior points per CU) an evaluation is a latency chain -- a scan costs lanes that idle anyway, every solve it
    // saves is a dozen dependent steps.  Whether the lazy scans save enough depends on the workload, not on the ratio above
    // (star: 16 pieces / 1 k - 10 k points - 8 ... - 20 %, the reference's star map 398 -> 367 us; 8 pieces / 10 k points
    // + 15 %: profiles/r05_small_cloud_modes.txt), so the next evaluation TRIES the lazy mode and stays in it when its GSIP
    // solves drop to <= 76 % of this evaluation's (the cases above: 68 - 72 % against 83 - 87 %).  Same bits in every mode.
    if (ctx->bound_mode == 0 && ctx->tail_mode != -2 && (long long)ctx->stats.interior_points <= tail_interior_limit(ctx) && gs > 0) {
      ctx->lz_state = 1;
      ctx->lz_cheap_solves = gs;
    }
    if (ctx->bound_mode == 1 && ctx->lipschitz_ok) ctx->an_state = 1;   // full scans pay: does the anchor variant pay more?
    if (ctx->bound_mode != 0) forget_launch_history(ctx);   // the launch plan on record is the cheap-bound one
  }
  // the batch count follows once the bound mode is known (also when it was pinned)
  if (rc == SVSDF_OK && ctx->ub_tune == 0) {
    ctx->ub_tune = 1;
    const bool big = ctx->bound_mode != 0 && ctx->P >= 400000;
    if (ctx->want_batches == 0) {
      // Round 5 (profiles/r05_batches_by_size.txt): 3 batches pay from ~ 80 k points per device in EVERY bound mode -- 60 k: + 2 ... 9 %,
      // 100 k: + 9 ... 14 %, 150 - 250 k: + 4 ... 16 % (star / sdHorseshoe / sdHeart; 2 batches always in between, 4 lose at
      // 500 k) -- not only from 400 k in the scanning modes (round 4's rule, measured at 1 M points only): the chain's ~ 20
      // dependent launches leave the chip draining at every step, and another batch's kernels fill those tails whatever the
      // bound mode.  Matters for BASELINE config 2 (100 k points) and for the stripes of a multi-GPU run (C4 / 8 = 500 k, NS / 8 = 125 k).
      const int nb = (ctx->P >= 80000) ? 3 : 1;
      if (ctx->saved_nbatch > 0) ctx->saved_nbatch = nb;        // (serialised for profiling: takes effect when that ends)
      else if (nb != ctx->nbatch) rc = set_batches(ctx, nb);
    } else if (ctx->want_batches < 0 && big) {
      ctx->bt_state = 1;
      ctx->bt_cand[0] = 1;
      ctx->bt_cand[1] = ctx->bound_mode == 2 ? 2 : 4;
      ctx->bt_cand[2] = 3;
      ctx->bt_ncand = 3;
    }
  }
  fill_mode_stats(ctx);
  ctx->h_partial = ctx->h_out;
  return rc;
}


void accumulate(int N, const double *partial, double *cost, double *gradT, double *gradC) {
  *cost += partial[0];
  for (int e = 0; e < 18 * N; ++e) gradC[e] += partial[kPartialGradC + e];
  for (int j = 0; j < N; ++j) gradT[j] += partial[partial_gradT(N) + j];
}

// Interior-sized arrays: GSIP state per interior point and the 24 sample slots per interior point (the big ones: 24 x 52 B).
int alloc_interior_buffers(svsdf_ctx *ctx, size_t cap) {
  int rc = 0;
  cap = std::max<size_t>(cap, 1);
  if (cap * kMaxSlots > 0x7fffffffull) return fail(ctx, SVSDF_ERR_INVALID, "too many interior points per shard (max ~89M)");
  if ((rc = ctx->gs_own.pt.alloc(ctx, cap, &ctx->gs.pt))) return rc;
  if ((rc = ctx->gs_own.r.alloc(ctx, cap, &ctx->gs.r))) return rc;
  if ((rc = ctx->gs_own.theta0.alloc(ctx, cap, &ctx->gs.theta0))) return rc;
  if ((rc = ctx->gs_own.theta_res.alloc(ctx, cap, &ctx->gs.theta_res))) return rc;
  if ((rc = ctx->gs_own.iter.alloc(ctx, cap, &ctx->gs.iter))) return rc;
  if ((rc = ctx->gs_own.nsamp.alloc(ctx, cap, &ctx->gs.nsamp))) return rc;
  if ((rc = ctx->gs_own.phase.alloc(ctx, cap, &ctx->gs.phase))) return rc;
  if ((rc = ctx->gs_own.req.alloc(ctx, cap, &ctx->gs.req))) return rc;
  const size_t S = cap * kMaxSlots;
  if ((rc = ctx->gs_own.sqx.alloc(ctx, S, &ctx->gs.sqx))) return rc;
  if ((rc = ctx->gs_own.sqy.alloc(ctx, S, &ctx->gs.sqy))) return rc;
  if ((rc = ctx->gs_own.sqth.alloc(ctx, S, &ctx->gs.sqth))) return rc;
  if ((rc = ctx->gs_own.sq_ub.alloc(ctx, S, &ctx->gs.sq_ub))) return rc;
  if ((rc = ctx->gs_own.sq_k.alloc(ctx, S, &ctx->gs.sq_k))) return rc;
  if ((rc = ctx->gs_own.sq_sdf.alloc(ctx, S, &ctx->gs.sq_sdf))) return rc;
  if ((rc = ctx->gs_own.sq_t.alloc(ctx, S, &ctx->gs.sq_t))) return rc;
  ctx->icap = cap;
  return SVSDF_OK;
}

int alloc_point_buffers(svsdf_ctx *ctx, size_t P) {
  int rc = 0;
  if ((rc = ctx->d_px.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_py.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_sdf.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_t.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_res_sdf.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_res_t.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_res_gx.alloc(ctx, P))) return rc;
  if ((rc = ctx->d_res_gy.alloc(ctx, P))) return rc;
  // per batch, in the batch's range of the point arrays: the two active lists (compact interior indices) and the
  // solve list (up to kMaxSlots requests per point of the batch)
  if ((rc = ctx->gs_own.list[0].alloc(ctx, P, &ctx->gs.list[0]))) return rc;
  if ((rc = ctx->gs_own.list[1].alloc(ctx, P, &ctx->gs.list[1]))) return rc;
  if ((rc = ctx->gs_own.solve.alloc(ctx, P * kMaxSlots, &ctx->gs.solve))) return rc;
  // the interior-sized arrays start at half the cloud (a corridor cloud has 25 - 40 % interior points) and are fitted
  // to the measured count after the first evaluation; an evaluation that needs more grows them and runs again
  ctx->icap_fitted = false;
  size_t cap0 = std::min(P, std::max<size_t>(P / 2, 4096));
  if (const char *e = std::getenv("SVSDF_ICAP_INIT")) cap0 = std::max<size_t>(1, (size_t)std::atoll(e));   // tests: force the grow-and-repeat path
  return alloc_interior_buffers(ctx, cap0);
}

// Morton order of the cloud (pure host): original indices sorted by (Morton code of the quantised xy, input index).
// The 64 lanes of a wave then hold spatially adjacent points (similar t*, similar iteration counts, same
// interior/exterior class); the sum is order-independent.
void morton_order(const double *xyz, size_t P, int flags, std::vector<long long> &order) {
  order.resize(P);
  std::iota(order.begin(), order.end(), 0ll);
  if ((flags & SVSDF_FLAG_KEEP_INPUT_ORDER) || P <= 1) return;
  double xmin = std::numeric_limits<double>::infinity(), xmax = -xmin, ymin = xmin, ymax = -xmin;
  for (size_t i = 0; i < P; ++i) {
    const double x = xyz[3 * i], y = xyz[3 * i + 1];
    if (x < xmin) xmin = x;
    if (x > xmax) xmax = x;
    if (y < ymin) ymin = y;
    if (y > ymax) ymax = y;
  }
  const double ext = std::max(std::max(xmax - xmin, ymax - ymin), 1e-12);
  std::vector<uint64_t> key(P);
  for (size_t i = 0; i < P; ++i) {
    const double fx = (xyz[3 * i] - xmin) / ext, fy = (xyz[3 * i + 1] - ymin) / ext;
    const uint32_t qx = (uint32_t)std::min(65535.0, std::max(0.0, fx * 65535.0));
    const uint32_t qy = (uint32_t)std::min(65535.0, std::max(0.0, fy * 65535.0));
    key[i] = ((uint64_t)(part1by1(qx) | (part1by1(qy) << 1)) << 32) | (uint64_t)(i & 0xffffffffu);
  }
  // LSD radix sort of the 32 Morton bits, 4 stable 8-bit passes over keys that start in index order (the low 32
  // bits carry the index and are never a sort digit)
  std::vector<uint64_t> tmp(P);
  for (int pass = 0; pass < 4; ++pass) {
    const int sh = 32 + 8 * pass;
    size_t cnt[257] = {0};
    for (size_t i = 0; i < P; ++i) ++cnt[((key[i] >> sh) & 0xffu) + 1];
    for (int b = 0; b < 256; ++b) cnt[b + 1] += cnt[b];
    for (size_t i = 0; i < P; ++i) tmp[cnt[(key[i] >> sh) & 0xffu]++] = key[i];
    key.swap(tmp);
  }
  for (size_t i = 0; i < P; ++i) order[i] = (long long)(key[i] & 0xffffffffull);
}

// Stripe `rk` of `ws` of a Morton order: stripes, not blocks, so that every rank gets a spatially uniform
// subsample (interior points cost up to ~150x an exterior one and cluster in space).
void stripe_of(const std::vector<long long> &order, int rk, int ws, std::vector<long long> &out) {
  ws = std::max(1, ws);
  out.clear();
  out.reserve(order.size() / (size_t)ws + 1);
  for (size_t k = (size_t)rk; k < order.size(); k += (size_t)ws) out.push_back(order[k]);
}

// which original indices rank `rk` of `ws` owns, in device order (also exported as svsdf_shard_plan)
void shard_plan(const double *xyz, size_t P, int rk, int ws, int flags, std::vector<long long> &out) {
  if (P > 0xffffffffull) { out.clear(); return; }
  std::vector<long long> order;
  morton_order(xyz, P, flags, order);
  stripe_of(order, rk, ws, out);
}

// Split the resident shard into nb contiguous batches of the sorted cloud, each running the whole launch chain on its
// own stream.  Large shards in the full-scan GSIP mode use 4: that chain alternates k_round (table scans) and k_solve
// launches of similar weight, ~10 dependent pairs, each ending in a tail where the chip drains; another batch's
// kernels fill those tails (1 M points: sdHorseshoe / 32 pieces 9.3 -> 8.6 ms, sdHeart 11.3 -> 10.5 ms).  In the
// cheap-bound mode (star) the solves dominate and splitting buys nothing (12.0 vs 12.0-12.7 ms); small shards are
// latency-bound chains, splitting only adds launches.  Any split gives the same bits.
int set_batches(svsdf_ctx *ctx, int nb) {
  nb = std::max(1, std::min(nb, kMaxBatches));
  const size_t Ps = ctx->P;
  ctx->nbatch = nb;
  std::vector<BatchCtl> hc(kMaxBatches);
  std::memset(hc.data(), 0, sizeof(BatchCtl) * kMaxBatches);
  // (Round 6 measured batches that are STRIPES of the Morton order -- points b, b + nb, ... -- instead of contiguous parts:
  // their launch chains then weigh the same and end together, where the contiguous thirds of C3 end 300 us apart.  It is 3 - 5 %
  // SLOWER (C3 5.60 -> 5.77 ms, a 500 k-point C4 stripe 3.61 -> 3.79): identical chains run in lockstep, all in k_round or all
  // in k_solve at the same time, and the overlap of unlike phases is what the concurrent batches are for.)
  for (int b = 0; b < nb; ++b) {
    const size_t s = Ps * (size_t)b / nb, e = Ps * (size_t)(b + 1) / nb;
    ctx->bstart[b] = (int)s;
    ctx->bcount[b] = (int)(e - s);
    hc[b].start = (int)s;
    hc[b].count = (int)(e - s);
  }
  HIPCHK(hipMemcpy(ctx->d_ctl, hc.data(), sizeof(BatchCtl) * kMaxBatches, hipMemcpyHostToDevice));
  return SVSDF_OK;
}

// Plan of a cloud ON THE DEVICE: d_xyz (AoS, P x 3 doubles, on the planner's device) -> bounding box -> Morton keys ->
// radix sort (hipcub, all 64 bits of (Morton code << 32 | input index): the same order as the host planner's stable
// sort by Morton code; a partial bit range [32, 64) came back unsorted).  Same key formula as the host planner
// (svsdf_shard_plan), so both give the same order (tests/test_points_upload_gpu.py).  1 M points: ~2 ms on the device
// (+ ~4 ms PCIe when the cloud comes from host memory) against 29 ms for round 1's host radix sort.
// The plan is made ONCE per cloud; every context of a multi-device group then takes its stripe from it (take_stripe).
int plan_cloud(svsdf_ctx *ctx, const double *d_xyz, size_t P, CloudPlan &plan) {
  plan.d_xyz = d_xyz;
  plan.P = P;
  if (P > 0x7fffffffull) return fail(ctx, SVSDF_ERR_INVALID, "too many points (max 2^31 - 1 per call)");
  if (P == 0) return SVSDF_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const unsigned grid = (unsigned)std::min<size_t>((P + kBlock - 1) / kBlock, 1024);
  int rc = plan.d_part.alloc(ctx, (size_t)grid * 4);
  if (rc == SVSDF_OK) rc = plan.d_keys.alloc(ctx, P);
  if (rc == SVSDF_OK) rc = plan.d_keys2.alloc(ctx, P);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(ctx->d_nonfinite, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_points_bbox, dim3(grid), dim3(kBlock), 0, st, d_xyz, P, plan.d_part, ctx->d_nonfinite);
  std::vector<double> hp((size_t)grid * 4);
  int bad = 0;
  HIPCHK(hipMemcpyAsync(hp.data(), plan.d_part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&bad, ctx->d_nonfinite, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad) return fail(ctx, SVSDF_ERR_NONFINITE, "non-finite query point");
  double xmin = hp[0], xmax = hp[1], ymin = hp[2], ymax = hp[3];
  for (unsigned b = 1; b < grid; ++b) {
    xmin = std::min(xmin, hp[4 * b]); xmax = std::max(xmax, hp[4 * b + 1]);
    ymin = std::min(ymin, hp[4 * b + 2]); ymax = std::max(ymax, hp[4 * b + 3]);
  }
  const double ext = std::max(std::max(xmax - xmin, ymax - ymin), 1e-12);
  const int keep = ((ctx->cfg.flags & SVSDF_FLAG_KEEP_INPUT_ORDER) || P <= 1) ? 1 : 0;
  hipLaunchKernelGGL(k_points_keys, dim3(grid), dim3(kBlock), 0, st, d_xyz, P, xmin, ymin, ext, keep, plan.d_keys);
  plan.sorted = plan.d_keys;
  if (!keep) {
    size_t tmp_bytes = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, plan.d_keys.get(), plan.d_keys2.get(), (int)P, 0, 64, st));
    if ((rc = plan.d_tmp.alloc(ctx, std::max<size_t>(tmp_bytes, 16)))) return rc;
    HIPCHK(hipcub::DeviceRadixSort::SortKeys(plan.d_tmp.get(), tmp_bytes, plan.d_keys.get(), plan.d_keys2.get(), (int)P, 0, 64, st));
    plan.sorted = plan.d_keys2;
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return SVSDF_OK;
}

// Context `ctx` takes stripe (rk, ws) of a planned cloud: gather into its SoA arrays + original indices.  The planner
// may be another context (multi-device group): then the stripe is gathered on the planner's device into a staging
// buffer and handed over with hipMemcpyPeer (over xGMI between two GPUs; the same call when both are one device).
int take_stripe(svsdf_ctx *ctx, svsdf_ctx *planner, const CloudPlan &plan, int rk, int ws) {
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipDeviceSynchronize());
  ws = std::max(1, ws);
  const size_t P = plan.P;
  // until the new cloud is completely in place the context holds none (a failed upload must not leave the old point
  // count with re-allocated buffers)
  ctx->P = 0;
  ctx->points_set = false;
  ctx->saved_nbatch = 0;
  const size_t Ps = (P > (size_t)rk) ? (P - (size_t)rk + (size_t)ws - 1) / (size_t)ws : 0;
  if (Ps * kMaxSlots > 0x7fffffffull) return fail(ctx, SVSDF_ERR_INVALID, "too many points per shard (max ~89M)");
  ctx->shard_idx.assign(Ps, 0ll);
  int rc = alloc_point_buffers(ctx, Ps);
  if (rc) return rc;
  if (Ps > 0) {
    const bool local = planner == ctx;
    HIPCHK(hipSetDevice(planner->device));
    hipStream_t st = planner->stream;
    Buf<long long> d_idx;   // staging on the planner's device, freed there
    Buf<double> d_sx, d_sy;
    rc = d_idx.alloc(ctx, Ps);
    if (rc == SVSDF_OK && !local) rc = d_sx.alloc(ctx, Ps);
    if (rc == SVSDF_OK && !local) rc = d_sy.alloc(ctx, Ps);
    if (rc) return rc;
    const unsigned g2 = (unsigned)std::min<size_t>((Ps + kBlock - 1) / kBlock, 1024);
    hipLaunchKernelGGL(k_points_gather, dim3(g2), dim3(kBlock), 0, st, plan.d_xyz, plan.sorted, P, rk, ws, Ps,
                       local ? ctx->d_px.get() : d_sx.get(), local ? ctx->d_py.get() : d_sy.get(), d_idx.get());
    HIPCHK(hipMemcpyAsync(ctx->shard_idx.data(), d_idx, Ps * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (!local) {
      HIPCHK(hipMemcpyPeer(ctx->d_px, ctx->device, d_sx, planner->device, Ps * sizeof(double)));
      HIPCHK(hipMemcpyPeer(ctx->d_py, ctx->device, d_sy, planner->device, Ps * sizeof(double)));
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->P = Ps;
  ctx->points_set = true;
  // batches: contiguous ranges of the sorted shard, pipelined on separate streams (one until the GSIP bound mode is
  // known, see set_batches)
  int rcb = set_batches(ctx, ctx->want_batches > 0 ? ctx->want_batches : 1);   // (rule / measurement: after the bound mode, run_pipeline_leaf)
  if (rcb) return rcb;
  reset_plan(ctx);
  if (!ctx->G_env) {   // lanes per query by shard size (default_lanes; Polygon: 4 -- its 2-lane kernel spills 52 registers under the 3-waves cap; C5 36.5 vs 34.8 ms)
    ctx->G = default_lanes(ctx, Ps);
    if (!ctx->G_late_env) ctx->G_late = std::max(ctx->G, 8);
  }
  return SVSDF_OK;
}

// single-device context: plan + its own stripe
int upload_shard_device(svsdf_ctx *ctx, const double *d_xyz, size_t P, int rk, int ws) {
  CloudPlan plan;
  int rc = plan_cloud(ctx, d_xyz, P, plan);
  if (rc) { ctx->P = 0; ctx->points_set = false; return rc; }
  return take_stripe(ctx, ctx, plan, rk, ws);
}

// svsdf_debug_sdf_at: upload the trajectory (same path as an evaluation: k_prep, piece-time mode), evaluate on the device
int debug_sdf_at(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, size_t n, const double *pxy, const double *t,
                 double *out8) {
  if (n == 0) return SVSDF_OK;
  if (n > 0x7fffffffull) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_debug_sdf_at: too many queries");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ev_used = 0;
  const size_t e0 = next_event(ctx);
  (void)hipEventRecord(ctx->ev_pool[e0], ctx->stream);
  int rc = upload_traj(ctx, N, coeffs, T, TrajUse::evaluation);
  if (rc) return rc;
  // (an early return below frees the scratch, and the owner's free waits for the device: no queued copy still reads pxy / t or
  // writes out8 once this function has returned)
  Buf<double> d_p, d_t, d_o;
  rc = d_p.alloc(ctx, 2 * n);
  if (rc == SVSDF_OK) rc = d_t.alloc(ctx, n);
  if (rc == SVSDF_OK) rc = d_o.alloc(ctx, 8 * n);
  if (rc) return rc;
  HIPCHK_AS("svsdf_debug_sdf_at", hipMemcpyAsync(d_p, pxy, 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK_AS("svsdf_debug_sdf_at", hipMemcpyAsync(d_t, t, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const size_t lds = (size_t)traj_lds_doubles(N) * sizeof(double);
  if (!launch_k_debug_sdf_at(ctx->cfg.shape_id, (unsigned)((n + 63) / 64), lds, ctx->stream, ctx->d_traj, ctx->sp, d_p, d_t, (int)n, d_o,
                             ctx->scaled ? &ctx->scale : nullptr))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_debug_sdf_at: shape not compiled into this build");
  HIPCHK_AS("svsdf_debug_sdf_at", hipGetLastError());   // a failed launch is this function's error, not the next evaluation's
  HIPCHK_AS("svsdf_debug_sdf_at", hipMemcpyAsync(out8, d_o, 8 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK_AS("svsdf_debug_sdf_at", hipStreamSynchronize(ctx->stream));
  return SVSDF_OK;
}

// mismatch count of the kernels' inlined sincos against the device library's (svsdf_debug_sincos_mismatches)
long long sincos_mismatches(svsdf_ctx *ctx, double lo, double hi, int n) {
  if (hipSetDevice(ctx->device) != hipSuccess) return -1;
  unsigned long long *d = reinterpret_cast<unsigned long long *>(ctx->d_out.get());
  if (hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_sincos_check, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, lo, hi, n, d);
  unsigned long long h = 0;
  if (hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return -1;
  return (long long)h;
}

// mismatch count of the kernels' unscaled sqrt against sqrt on n host operands (svsdf_debug_sqrt_mismatches)
long long sqrt_mismatches(svsdf_ctx *ctx, const double *x, size_t n, int flavour) {
  if (hipSetDevice(ctx->device) != hipSuccess) return -1;
  Buf<double> dx;   // (freed on every return; that free waits for the device, so no queued copy outlives x or h)
  if (dx.alloc(ctx, n)) return -1;
  unsigned long long *d = reinterpret_cast<unsigned long long *>(ctx->d_out.get());
  unsigned long long h = 0;
  if (hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(k_sqrt_check, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, dx.get(), (long long)n, flavour, d);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return -1;
  return (long long)h;
}

}  // namespace svsdf_impl
