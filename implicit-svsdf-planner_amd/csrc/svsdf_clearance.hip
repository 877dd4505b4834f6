// svsdf_clearance.hip -- svsdf_min_clearance, svsdf_point_clearance, svsdf_motion_bounds and svsdf_scale_bounds (include/svsdf_c.h):
// the host side of the certified minimum-clearance search and of its per-point form, and the shape-independent kernels of
// svsdf_clearance.hpp (SVSDF_CLR_TU).  The shape-templated level kernels live in svsdf_shape_slice.hip behind launch_k_clr /
// launch_k_pclr.
#define SVSDF_CLR_TU
#include "svsdf_ctx.hpp"
#include "svsdf_scale_host.hpp"

using namespace svsdf;

namespace svsdf_impl {
namespace {

struct Events {   // the two events of device_ms
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

struct Frontier {   // one chunk of a level's frontier: 2 * cap pairs
  Buf<ClrPair> buf;
  size_t n = 0;
};

constexpr double kInf = std::numeric_limits<double>::infinity();

// The per-interval arrays of a search, one after the other in one buffer: V_j, W_j (svsdf_motion_bounds), then under a scale
// schedule Imax_j, Q_j, Smin_j, Smax_j (svsdf_scale_bounds), each over level-0 interval j widened by 1e-4 s (as the cull
// widens 0.075 to 0.0751) and inherited by every descendant.
std::vector<double> interval_bounds(const svsdf_ctx *ctx, int N, const double *coeffs, const std::vector<double> &S, size_t n0,
                                    double w) {
  const double td = S[N];
  std::vector<double> B((ctx->scaled ? 6 : 2) * n0);
  svsdf_scale sc{};
  sc.struct_size = (int)sizeof(svsdf_scale);
  sc.enabled = 1;
  sc.c[0] = ctx->scale.cx; sc.amp[0] = ctx->scale.ax; sc.omega[0] = ctx->scale.wx; sc.phase[0] = ctx->scale.phx;
  sc.c[1] = ctx->scale.cy; sc.amp[1] = ctx->scale.ay; sc.omega[1] = ctx->scale.wy; sc.phase[1] = ctx->scale.phy;
  for (size_t j = 0; j < n0; ++j) {
    const double m = clr_mid((unsigned)j, 0ull, 0, w, td), h = clr_half_width(w, 0);
    double b2[2];
    svsdf_traj::motion_bounds(N, coeffs, S.data(), m - h - 1e-4, m + h + 1e-4, b2);
    B[j] = b2[0];
    B[n0 + j] = b2[1];
    if (!ctx->scaled) continue;
    double b4[4];
    svsdf_traj::scale_bounds(&sc, m - h - 1e-4, m + h + 1e-4, b4);
    B[2 * n0 + j] = b4[2];   // Imax
    B[3 * n0 + j] = b4[3];   // Q
    B[4 * n0 + j] = b4[0];   // Smin
    B[5 * n0 + j] = b4[1];   // Smax
  }
  return B;
}

}  // namespace

// The search on ONE device's stripe.  Arguments are validated by svsdf_min_clearance.
int min_clearance_leaf(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, const svsdf_clearance_params &prm,
                       svsdf_clearance_result *out) {
  const char *const who = "svsdf_min_clearance";
  const bool has_target = prm.target == prm.target;
  *out = svsdf_clearance_result{};
  out->lower = out->upper = kInf;
  out->t_witness = 0.0;
  out->point_index = -1;
  if (ctx->P == 0) {   // nothing to be near to
    out->status = has_target ? SVSDF_CLEARANCE_SAFE : SVSDF_CLEARANCE_CONVERGED;
    return SVSDF_OK;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events ev;
  HIPCHK(hipEventCreate(&ev.e0));
  HIPCHK(hipEventCreate(&ev.e1));
  HIPCHK(hipEventRecord(ev.e0, st));
  if (int rc = upload_traj(ctx, N, coeffs, T, TrajUse::probe)) return rc;   // (k_prep, piece-time mode: as an evaluation's)
  const std::vector<double> S = svsdf_traj::prefix_sums(N, T);
  const double td = S[N];
  size_t n0 = (size_t)std::max(1.0, std::ceil(td / 0.15));
  if (td / (double)n0 > 0.15) ++n0;
  const double w = td / (double)n0;
  const unsigned P = (unsigned)ctx->P;
  const unsigned ntiles = (P + kClrTile - 1) / kClrTile;
  const size_t cap = prm.pair_capacity ? std::max<size_t>(prm.pair_capacity, kClrTile)
                                       : std::min<size_t>(std::max<size_t>(2 * (size_t)P, 4096), (size_t)1 << 22);
  if (cap > ((size_t)1 << 30)) return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": pair_capacity above 2^30");
  const unsigned long long budget = prm.max_evals ? prm.max_evals : 4ull * P * (unsigned long long)std::ceil(td / 0.15);

  // level-0 motion bounds (and schedule bounds): the interval widened by 1e-4 s, as the cull widens 0.075 to 0.0751
  const std::vector<double> VW = interval_bounds(ctx, N, coeffs, S, n0, w);
  const unsigned maxgrid = (unsigned)std::max(1, ctx->n_cu) * 8u;
  Buf<double> d_vw;
  Buf<Pose> d_mid;
  Buf<long long> d_orig;
  Buf<ClrTileCircle> d_tiles;
  Buf<ClrPartial> d_partials;
  Buf<ClrRecord> d_rec;
  PinBuf<ClrRecord> h_rec;
  Buf<unsigned long long> d_count;
  Buf<ClrTilePair> d_tp, d_seed;
  int rc = d_vw.alloc(ctx, VW.size());
  if (rc == SVSDF_OK) rc = d_mid.alloc(ctx, n0);
  if (rc == SVSDF_OK) rc = d_orig.alloc(ctx, P);
  if (rc == SVSDF_OK) rc = d_tiles.alloc(ctx, ntiles);
  if (rc == SVSDF_OK) rc = d_partials.alloc(ctx, maxgrid);
  if (rc == SVSDF_OK) rc = d_rec.alloc(ctx, 1);
  if (rc == SVSDF_OK) rc = h_rec.alloc(ctx, 1);
  if (rc == SVSDF_OK) rc = d_count.alloc(ctx, 1);
  if (rc == SVSDF_OK) rc = d_seed.alloc(ctx, 1);
  if (rc) return rc;
  const double *d_V = d_vw.get(), *d_W = d_vw.get() + n0;
  // under a scale schedule: the schedule with Imax_j, Q_j for the level kernels, Smin_j, Smax_j for the cheap bound
  const double *const d_sb = ctx->scaled ? d_vw.get() + 2 * n0 : nullptr;   // (the rigid buffer ends after W_j)
  const ClrScale cscale{ctx->scale, d_sb, d_sb ? d_sb + n0 : nullptr};
  const double *d_Smin = d_sb ? d_sb + 2 * n0 : nullptr, *d_Smax = d_sb ? d_sb + 3 * n0 : nullptr;
  HIPCHK_AS(who, hipMemcpyAsync(d_vw, VW.data(), VW.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK_AS(who, hipMemcpyAsync(d_orig, ctx->shard_idx.data(), (size_t)P * sizeof(long long), hipMemcpyHostToDevice, st));
  const size_t traj_lds = (size_t)traj_lds_doubles(N) * sizeof(double);
  hipLaunchKernelGGL(k_clr_tiles, dim3((ntiles + kClrBlock - 1) / kClrBlock), dim3(kClrBlock), 0, st, ctx->d_px.get(), ctx->d_py.get(), P,
                     ntiles, d_tiles.get());
  hipLaunchKernelGGL(k_clr_mid, dim3((unsigned)((n0 + 63) / 64)), dim3(64), traj_lds, st, ctx->d_traj.get(), w, (unsigned)n0, d_mid.get());
  HIPCHK_AS(who, hipGetLastError());

  // one launch's results on the host: reduce the blocks' partials, read the record
  auto read_record = [&](unsigned grid) -> int {
    hipLaunchKernelGGL(k_clr_reduce, dim3(1), dim3(kClrBlock), 0, st, d_partials.get(), grid, d_rec.get());
    HIPCHK_AS(who, hipGetLastError());
    HIPCHK_AS(who, hipMemcpyAsync(h_rec.get(), d_rec.get(), sizeof(ClrRecord), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(who, hipStreamSynchronize(st));
    if (h_rec->overflow) return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": internal error, a frontier buffer overflowed");
    return SVSDF_OK;
  };
  const unsigned long long total_tp = (unsigned long long)ntiles * n0;
  const unsigned broad_grid = (unsigned)std::min<unsigned long long>((total_tp + kClrBlock - 1) / kClrBlock, maxgrid);

  // broad phase: the pair with the smallest cheap bound is evaluated first and gives the first upper
  HIPCHK_AS(who, hipMemsetAsync(d_rec, 0, sizeof(ClrRecord), st));
  hipLaunchKernelGGL(k_clr_broad, dim3(broad_grid), dim3(kClrBlock), 0, st, d_tiles.get(), ntiles, d_mid.get(), d_V, (unsigned)n0, w,
                     ctx->r_bound, 0.0, (ClrTilePair *)nullptr, 0ull, (unsigned long long *)nullptr, d_partials.get(), d_Smin, d_Smax);
  if ((rc = read_record(broad_grid))) return rc;
  ClrLaunch a{};
  a.traj = ctx->d_traj; a.sp = ctx->sp; a.px = ctx->d_px; a.py = ctx->d_py; a.orig = d_orig; a.P = P; a.mid = d_mid;
  a.V = d_V; a.W = d_W; a.w = w; a.dur = td; a.rec = d_rec; a.partials = d_partials;
  a.scl = ctx->scaled ? &cscale : nullptr;
  auto launch = [&](unsigned grid) -> int {
    if (!launch_k_clr(ctx->cfg.shape_id, grid, traj_lds, st, a))
      return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": shape not compiled into this build");
    HIPCHK_AS(who, hipGetLastError());
    return read_record(grid);
  };
  ClrBest best = clr_no_best();
  unsigned long long evals = 0, pairs = 0;
  {
    const ClrTilePair seed{(unsigned)((unsigned long long)h_rec->best.idx / n0), (unsigned)((unsigned long long)h_rec->best.idx % n0)};
    HIPCHK_AS(who, hipMemcpyAsync(d_seed, &seed, sizeof(seed), hipMemcpyHostToDevice, st));
    HIPCHK_AS(who, hipMemsetAsync(d_rec, 0, sizeof(ClrRecord), st));
    a.L = 0; a.tp = d_seed; a.n = 1; a.thr = 0.0; a.emit = 0; a.out = nullptr; a.out_cap = 0;
    if ((rc = launch(1))) return rc;
    best = h_rec->best;
    evals += h_rec->evals;
  }
  // tiles whose cheap bound exceeds that upper cannot hold the minimum: the others are listed (count, then fill)
  unsigned long long kept = 0;
  for (int pass = 0; pass < 2; ++pass) {
    HIPCHK_AS(who, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_clr_broad, dim3(broad_grid), dim3(kClrBlock), 0, st, d_tiles.get(), ntiles, d_mid.get(), d_V, (unsigned)n0, w,
                       ctx->r_bound, best.f, pass ? d_tp.get() : (ClrTilePair *)nullptr, kept, d_count.get(), d_partials.get(), d_Smin, d_Smax);
    HIPCHK_AS(who, hipGetLastError());
    unsigned long long c = 0;
    HIPCHK_AS(who, hipMemcpyAsync(&c, d_count.get(), sizeof(c), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(who, hipStreamSynchronize(st));
    if (pass == 0) {
      kept = c;
      if (kept > 0xffffffffull) return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": too many (tile, interval) pairs");
      if ((rc = d_tp.alloc(ctx, (size_t)kept))) return rc;
    } else if (c != kept) {
      return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": internal error, the broad phase counted twice differently");
    }
  }

  // the levels.  A frontier is a list of chunks of 2 * cap pairs; a launch takes <= cap pairs of one chunk and appends
  // what they split into to the next frontier's last chunk, or to a fresh one when that has no room for all of them
  std::vector<Frontier> cur, nxt, pool;
  auto room = [&](size_t need) -> int {
    if (!nxt.empty() && nxt.back().n + need <= 2 * cap) return SVSDF_OK;
    Frontier f;
    if (!pool.empty()) { f = std::move(pool.back()); pool.pop_back(); f.n = 0; }
    else if (int r = f.buf.alloc(ctx, 2 * cap)) return r;
    nxt.push_back(std::move(f));
    return SVSDF_OK;
  };
  double settled = kInf, open = kInf;
  int levels = 0, status = -1;
  for (int L = 0;; ++L) {
    unsigned long long todo = 0;   // evaluations of this level
    if (L == 0) todo = kept * kClrTile;
    else for (const Frontier &f : cur) todo += f.n;
    if (L > 0 && (evals + todo > budget || L > kClrMaxLevel)) { status = SVSDF_CLEARANCE_BUDGET; break; }
    const double thr = best.f - prm.eps;   // fixed before the level starts
    ClrBest lbest = clr_no_best();
    double lopen = kInf;
    auto fold = [&](Frontier &dst) {
      if (clr_better(h_rec->best, lbest)) lbest = h_rec->best;
      settled = std::min(settled, h_rec->settled_min);
      lopen = std::min(lopen, h_rec->open_min);
      evals += h_rec->evals;
      dst.n += (size_t)h_rec->out_count;
    };
    a.L = L; a.thr = thr; a.emit = 1;
    if (L == 0) {
      const size_t per = cap / kClrTile;   // >= 1
      for (size_t off = 0; off < (size_t)kept; off += per) {
        const size_t n = std::min(per, (size_t)kept - off);
        if ((rc = room(2 * kClrTile * n))) return rc;
        Frontier &dst = nxt.back();
        HIPCHK_AS(who, hipMemsetAsync(d_rec, 0, sizeof(ClrRecord), st));
        a.tp = d_tp.get() + off; a.n = (unsigned)n; a.out = dst.buf.get() + dst.n; a.out_cap = (unsigned)(2 * kClrTile * n);
        if ((rc = launch((unsigned)std::min<size_t>((n + 3) / 4, maxgrid)))) return rc;
        fold(dst);
      }
    } else {
      pairs += todo;
      for (Frontier &src : cur)
        for (size_t off = 0; off < src.n; off += cap) {
          const size_t n = std::min(cap, src.n - off);
          if ((rc = room(2 * n))) return rc;
          Frontier &dst = nxt.back();
          HIPCHK_AS(who, hipMemsetAsync(d_rec, 0, sizeof(ClrRecord), st));
          a.in = src.buf.get() + off; a.n = (unsigned)n; a.out = dst.buf.get() + dst.n; a.out_cap = (unsigned)(2 * n);
          if ((rc = launch((unsigned)std::min<size_t>((n + kClrBlock - 1) / kClrBlock, maxgrid)))) return rc;
          fold(dst);
        }
    }
    ++levels;
    if (clr_better(lbest, best)) best = lbest;
    open = lopen;
    for (Frontier &f : cur) pool.push_back(std::move(f));
    cur.clear();
    for (Frontier &f : nxt) { if (f.n) cur.push_back(std::move(f)); else pool.push_back(std::move(f)); }
    nxt.clear();
    if (has_target && std::min(settled, open) >= prm.target) { status = SVSDF_CLEARANCE_SAFE; break; }
    if (has_target && best.f < prm.target) { status = SVSDF_CLEARANCE_UNSAFE; break; }
    if (cur.empty()) { status = SVSDF_CLEARANCE_CONVERGED; break; }
  }
  double xy[2] = {0.0, 0.0};
  HIPCHK_AS(who, hipMemcpyAsync(&xy[0], ctx->d_px.get() + best.pt, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK_AS(who, hipMemcpyAsync(&xy[1], ctx->d_py.get() + best.pt, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK_AS(who, hipEventRecord(ev.e1, st));
  HIPCHK_AS(who, hipStreamSynchronize(st));
  float ms = 0.0f;
  HIPCHK_AS(who, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  out->status = status;
  out->levels = levels;
  out->upper = best.f;
  out->lower = std::min(best.f, std::min(settled, open));   // every settled and every still-open bound
  out->t_witness = best.t;
  out->point_index = best.idx;
  out->point_xy[0] = xy[0];
  out->point_xy[1] = xy[1];
  out->evals = evals;
  out->pairs = pairs;
  out->tile_pairs = total_tp;
  out->tile_pairs_kept = kept;
  out->device_ms = (double)ms;
  return SVSDF_OK;
}

static_assert(kPclrConverged == SVSDF_POINT_CONVERGED && kPclrFar == SVSDF_POINT_FAR && kPclrSafe == SVSDF_POINT_SAFE &&
              kPclrUnsafe == SVSDF_POINT_UNSAFE && kPclrOpen == SVSDF_POINT_OPEN, "k_pclr_final writes the C ABI's states");

// svsdf_point_clearance on ONE device's stripe.  Arguments are validated by svsdf_point_clearance; the four arrays (any may
// be null) are indexed by ORIGINAL point index, so the stripes of a group write disjoint entries of the caller's arrays.
int point_clearance_leaf(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, const svsdf_point_clearance_params &prm,
                         double *lower, double *upper, double *t_witness, unsigned char *state, svsdf_point_clearance_result *out) {
  const char *const who = "svsdf_point_clearance";
  *out = svsdf_point_clearance_result{};
  out->status = SVSDF_CLEARANCE_CONVERGED;
  out->lower = out->upper = kInf;
  out->t_witness = 0.0;
  out->point_index = -1;
  if (ctx->P == 0) return SVSDF_OK;   // nothing to be near to
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events ev;
  HIPCHK(hipEventCreate(&ev.e0));
  HIPCHK(hipEventCreate(&ev.e1));
  HIPCHK(hipEventRecord(ev.e0, st));
  if (int rc = upload_traj(ctx, N, coeffs, T, TrajUse::probe)) return rc;   // (k_prep, piece-time mode: as an evaluation's)
  const std::vector<double> S = svsdf_traj::prefix_sums(N, T);
  const double td = S[N];
  size_t n0 = (size_t)std::max(1.0, std::ceil(td / 0.15));   // the sibling's intervals
  if (td / (double)n0 > 0.15) ++n0;
  const double w = td / (double)n0;
  const unsigned P = (unsigned)ctx->P;
  const unsigned ntiles = (P + kClrTile - 1) / kClrTile;
  const size_t cap = prm.pair_capacity ? std::max<size_t>(prm.pair_capacity, kClrTile)
                                       : std::min<size_t>(std::max<size_t>(2 * (size_t)P, 4096), (size_t)1 << 22);
  if (cap > ((size_t)1 << 30)) return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": pair_capacity above 2^30");
  const unsigned long long budget = prm.max_evals ? prm.max_evals : 4ull * P * (unsigned long long)std::ceil(td / 0.15);

  const std::vector<double> VW = interval_bounds(ctx, N, coeffs, S, n0, w);   // the sibling's V_j, W_j (Imax_j, Q_j, Smin_j, Smax_j)
  const unsigned maxgrid = (unsigned)std::max(1, ctx->n_cu) * 8u;
  const size_t tiles64 = (size_t)ntiles * kClrTile, n_ev = std::max(cap, tiles64);
  Buf<double> d_vw, d_tmax, d_res;
  Buf<Pose> d_mid;
  Buf<ClrTileCircle> d_tiles;
  Buf<unsigned long long> d_keys, d_tdrop, d_count;   // d_keys: U, S, open, tw, snap -- P keys each
  Buf<unsigned char> d_state;
  Buf<PclrCounters> d_cnt;
  PinBuf<PclrCounters> h_cnt;
  Buf<PclrEval> d_ev;
  Buf<ClrTilePair> d_tp, d_seed;
  PinBuf<double> h_res;
  PinBuf<unsigned char> h_state;
  int rc = d_vw.alloc(ctx, VW.size());
  if (rc == SVSDF_OK) rc = d_mid.alloc(ctx, n0);
  if (rc == SVSDF_OK) rc = d_tiles.alloc(ctx, ntiles);
  if (rc == SVSDF_OK) rc = d_tmax.alloc(ctx, ntiles);
  if (rc == SVSDF_OK) rc = d_tdrop.alloc(ctx, ntiles);
  if (rc == SVSDF_OK) rc = d_keys.alloc(ctx, 5 * (size_t)P);
  if (rc == SVSDF_OK) rc = d_res.alloc(ctx, 3 * (size_t)P);
  if (rc == SVSDF_OK) rc = d_state.alloc(ctx, P);
  if (rc == SVSDF_OK) rc = h_res.alloc(ctx, 3 * (size_t)P);
  if (rc == SVSDF_OK) rc = h_state.alloc(ctx, P);
  if (rc == SVSDF_OK) rc = d_cnt.alloc(ctx, 1);
  if (rc == SVSDF_OK) rc = h_cnt.alloc(ctx, 1);
  if (rc == SVSDF_OK) rc = d_count.alloc(ctx, 1);
  if (rc == SVSDF_OK) rc = d_seed.alloc(ctx, ntiles);
  if (rc == SVSDF_OK) rc = d_ev.alloc(ctx, n_ev);
  if (rc) return rc;
  const double *d_V = d_vw.get(), *d_W = d_vw.get() + n0;
  // under a scale schedule: the schedule with Imax_j, Q_j for the level kernels, Smin_j, Smax_j for the cheap bound
  const double *const d_sb = ctx->scaled ? d_vw.get() + 2 * n0 : nullptr;   // (the rigid buffer ends after W_j)
  const ClrScale cscale{ctx->scale, d_sb, d_sb ? d_sb + n0 : nullptr};
  const double *d_Smin = d_sb ? d_sb + 2 * n0 : nullptr, *d_Smax = d_sb ? d_sb + 3 * n0 : nullptr;
  PclrState ps{};
  ps.U = d_keys.get(); ps.S = ps.U + P; ps.open = ps.S + P; ps.tw = ps.open + P;
  unsigned long long *const d_snap = ps.tw + P;
  ps.snap = d_snap;
  const unsigned pgrid = std::min((P + kClrBlock - 1) / kClrBlock, maxgrid);
  HIPCHK_AS(who, hipMemcpyAsync(d_vw, VW.data(), VW.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const size_t traj_lds = (size_t)traj_lds_doubles(N) * sizeof(double);
  hipLaunchKernelGGL(k_pclr_fill, dim3((unsigned)std::min<size_t>((5 * (size_t)P + kClrBlock - 1) / kClrBlock, maxgrid)), dim3(kClrBlock), 0, st, d_keys.get(),
                     5 * (size_t)P, kOrdKeyPosInf);
  hipLaunchKernelGGL(k_clr_tiles, dim3((ntiles + kClrBlock - 1) / kClrBlock), dim3(kClrBlock), 0, st, ctx->d_px.get(), ctx->d_py.get(), P,
                     ntiles, d_tiles.get());
  hipLaunchKernelGGL(k_clr_mid, dim3((unsigned)((n0 + 63) / 64)), dim3(64), traj_lds, st, ctx->d_traj.get(), w, (unsigned)n0, d_mid.get());
  hipLaunchKernelGGL(k_pclr_seed, dim3((ntiles + 3) / 4), dim3(kClrBlock), 0, st, d_tiles.get(), ntiles, d_mid.get(), d_V, (unsigned)n0, w,
                     ctx->r_bound, d_seed.get(), d_Smin, d_Smax);
  HIPCHK_AS(who, hipGetLastError());

  PclrLaunch a{};
  a.traj = ctx->d_traj; a.sp = ctx->sp; a.px = ctx->d_px; a.py = ctx->d_py; a.P = P; a.mid = d_mid; a.V = d_V; a.W = d_W; a.w = w;
  a.dur = td; a.rule = PclrRule{prm.eps, prm.cap, prm.target}; a.s = ps; a.ev = d_ev; a.cnt = d_cnt;
  a.scl = ctx->scaled ? &cscale : nullptr;
  // one launch: the level kernel, the witness pass over its evaluations (n_evals entries of d_ev), one record read
  auto launch = [&](unsigned grid, unsigned n_evals) -> int {
    HIPCHK_AS(who, hipMemsetAsync(d_cnt, 0, sizeof(PclrCounters), st));
    if (!launch_k_pclr(ctx->cfg.shape_id, grid, traj_lds, st, a))
      return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": shape not compiled into this build");
    hipLaunchKernelGGL(k_pclr_witness, dim3(std::min((n_evals + kClrBlock - 1) / kClrBlock, maxgrid)), dim3(kClrBlock), 0, st,
                       a.L == 0 ? a.tp : (const ClrTilePair *)nullptr, a.in, n_evals, P, d_ev.get(), ps.U, ps.tw);
    HIPCHK_AS(who, hipGetLastError());
    HIPCHK_AS(who, hipMemcpyAsync(h_cnt.get(), d_cnt.get(), sizeof(PclrCounters), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(who, hipStreamSynchronize(st));
    if (h_cnt->overflow) return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": internal error, a frontier buffer overflowed");
    return SVSDF_OK;
  };
  unsigned long long evals = 0, pairs = 0;
  // the seed: every tile against the interval of its smallest cheap bound gives every point a finite U
  a.L = 0; a.tp = d_seed; a.n = ntiles; a.emit = 0; a.out = nullptr; a.out_cap = 0;
  if ((rc = launch(std::min((ntiles + 3) / 4, maxgrid), (unsigned)tiles64))) return rc;
  evals += h_cnt->evals;
  hipLaunchKernelGGL(k_pclr_tile_max, dim3((ntiles + kClrBlock - 1) / kClrBlock), dim3(kClrBlock), 0, st, ps.U, P, ntiles, d_tmax.get(),
                     d_tdrop.get());
  // the broad phase per tile (count, then fill)
  const unsigned long long total_tp = (unsigned long long)ntiles * n0;
  const unsigned broad_grid = (unsigned)std::min<unsigned long long>((total_tp + kClrBlock - 1) / kClrBlock, maxgrid);
  unsigned long long kept = 0;
  for (int pass = 0; pass < 2; ++pass) {
    HIPCHK_AS(who, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_pclr_broad, dim3(broad_grid), dim3(kClrBlock), 0, st, d_tiles.get(), ntiles, d_mid.get(), d_V, (unsigned)n0, w,
                       ctx->r_bound, prm.cap, d_tmax.get(), pass ? d_tp.get() : (ClrTilePair *)nullptr, kept, d_count.get(), d_tdrop.get(),
                       d_Smin, d_Smax);
    HIPCHK_AS(who, hipGetLastError());
    unsigned long long c = 0;
    HIPCHK_AS(who, hipMemcpyAsync(&c, d_count.get(), sizeof(c), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(who, hipStreamSynchronize(st));
    if (pass == 0) {
      kept = c;
      if (kept > 0xffffffffull) return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": too many (tile, interval) pairs");
      if ((rc = d_tp.alloc(ctx, (size_t)kept))) return rc;
    } else if (c != kept) {
      return fail(ctx, SVSDF_ERR_INVALID, std::string(who) + ": internal error, the broad phase counted twice differently");
    }
  }

  // the levels: the sibling's frontier chunks, slicing and one record read per launch
  std::vector<Frontier> cur, nxt, pool;
  auto room = [&](size_t need) -> int {
    if (!nxt.empty() && nxt.back().n + need <= 2 * cap) return SVSDF_OK;
    Frontier f;
    if (!pool.empty()) { f = std::move(pool.back()); pool.pop_back(); f.n = 0; }
    else if (int r = f.buf.alloc(ctx, 2 * cap)) return r;
    nxt.push_back(std::move(f));
    return SVSDF_OK;
  };
  int levels = 0;
  for (int L = 0;; ++L) {
    unsigned long long todo = 0;   // evaluations of this level
    if (L == 0) todo = kept * kClrTile;
    else for (const Frontier &f : cur) todo += f.n;
    if (L > 0 && (todo == 0 || evals + todo > budget || L > kClrMaxLevel)) break;   // (open[] keeps the bounds of what is left)
    hipLaunchKernelGGL(k_pclr_snapshot, dim3(pgrid), dim3(kClrBlock), 0, st, ps.U, d_snap, ps.open, P);   // fixed before the level starts
    a.L = L; a.emit = 1;
    if (L == 0) {
      const size_t per = cap / kClrTile;   // >= 1
      for (size_t off = 0; off < (size_t)kept; off += per) {
        const size_t n = std::min(per, (size_t)kept - off);
        if ((rc = room(2 * kClrTile * n))) return rc;
        Frontier &dst = nxt.back();
        a.tp = d_tp.get() + off; a.n = (unsigned)n; a.out = dst.buf.get() + dst.n; a.out_cap = (unsigned)(2 * kClrTile * n);
        if ((rc = launch((unsigned)std::min<size_t>((n + 3) / 4, maxgrid), (unsigned)(n * kClrTile)))) return rc;
        evals += h_cnt->evals;
        dst.n += (size_t)h_cnt->out_count;
      }
    } else {
      pairs += todo;
      for (Frontier &src : cur)
        for (size_t off = 0; off < src.n; off += cap) {
          const size_t n = std::min(cap, src.n - off);
          if ((rc = room(2 * n))) return rc;
          Frontier &dst = nxt.back();
          a.in = src.buf.get() + off; a.n = (unsigned)n; a.out = dst.buf.get() + dst.n; a.out_cap = (unsigned)(2 * n);
          if ((rc = launch((unsigned)std::min<size_t>((n + kClrBlock - 1) / kClrBlock, maxgrid), (unsigned)n))) return rc;
          evals += h_cnt->evals;
          dst.n += (size_t)h_cnt->out_count;
        }
    }
    ++levels;
    for (Frontier &f : cur) pool.push_back(std::move(f));
    cur.clear();
    for (Frontier &f : nxt) { if (f.n) cur.push_back(std::move(f)); else pool.push_back(std::move(f)); }
    nxt.clear();
  }
  double *const d_lo = d_res.get(), *const d_up = d_lo + P, *const d_tw = d_up + P;
  hipLaunchKernelGGL(k_pclr_final, dim3(pgrid), dim3(kClrBlock), 0, st, P, ps, d_tdrop.get(), a.rule, d_lo, d_up, d_tw, d_state.get());
  HIPCHK_AS(who, hipGetLastError());
  HIPCHK_AS(who, hipEventRecord(ev.e1, st));
  HIPCHK_AS(who, hipMemcpyAsync(h_res.get(), d_res.get(), 3 * (size_t)P * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK_AS(who, hipMemcpyAsync(h_state.get(), d_state.get(), (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK_AS(who, hipStreamSynchronize(st));
  float ms = 0.0f;
  HIPCHK_AS(who, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  // shard order -> the caller's order; the minimum over the points (ties: the smaller original index)
  const double *h_lo = h_res.get(), *h_up = h_lo + P, *h_tw = h_up + P;
  for (unsigned p = 0; p < P; ++p) {
    const long long o = ctx->shard_idx[p];
    if (lower) lower[o] = h_lo[p];
    if (upper) upper[o] = h_up[p];
    if (t_witness) t_witness[o] = h_tw[p];
    if (state) state[o] = h_state[p];
    out->counts[h_state[p] < SVSDF_POINT_STATES ? h_state[p] : SVSDF_POINT_OPEN] += 1ull;
    out->lower = std::min(out->lower, h_lo[p]);
    if (out->point_index < 0 || h_up[p] < out->upper || (h_up[p] == out->upper && o < out->point_index)) {
      out->upper = h_up[p]; out->t_witness = h_tw[p]; out->point_index = o;
    }
  }
  out->status = out->counts[SVSDF_POINT_OPEN] ? SVSDF_CLEARANCE_BUDGET : SVSDF_CLEARANCE_CONVERGED;
  out->levels = levels;
  out->evals = evals;
  out->pairs = pairs;
  out->tile_pairs = total_tp;
  out->tile_pairs_kept = kept;
  out->device_ms = (double)ms;
  return SVSDF_OK;
}

}  // namespace svsdf_impl

using namespace svsdf_impl;

extern "C" {

void svsdf_clearance_params_default(svsdf_clearance_params *p) {
  if (!p) return;
  *p = svsdf_clearance_params{};
  p->struct_size = sizeof(svsdf_clearance_params);
  p->eps = 1e-3;
  p->target = std::numeric_limits<double>::quiet_NaN();
  p->max_evals = 0;
  p->pair_capacity = 0;
}

int svsdf_motion_bounds(int N, const double *coeffs, const double *T, double ta, double tb, double out2[2]) {
  if (!coeffs || !T || !out2) return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_motion_bounds: null argument");
  if (ta != ta || tb != tb || tb < ta) return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_motion_bounds: needs ta <= tb");
  const svsdf_traj::TrajCheck chk = svsdf_traj::check_traj(N, coeffs, T);
  if (chk.code) return fail(nullptr, chk.code, std::string("svsdf_motion_bounds: ") + chk.reason);
  svsdf_traj::motion_bounds(N, coeffs, svsdf_traj::prefix_sums(N, T).data(), ta, tb, out2);
  return SVSDF_OK;
}

int svsdf_scale_bounds(const svsdf_scale *scale, double ta, double tb, double out4[4]) {
  if (!out4) return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_scale_bounds: null argument");
  if (!std::isfinite(ta) || !std::isfinite(tb) || tb < ta) return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_scale_bounds: needs finite ta <= tb");
  const svsdf_traj::ScaleCheck chk = svsdf_traj::check_scale(scale);
  if (chk.code) return fail(nullptr, chk.code, std::string("svsdf_scale_bounds: ") + chk.reason);
  svsdf_traj::scale_bounds(scale, ta, tb, out4);
  return SVSDF_OK;
}

int svsdf_min_clearance(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, const svsdf_clearance_params *params,
                        svsdf_clearance_result *out) {
  if (!ctx || !coeffs || !T || !out) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_min_clearance: null argument");
  svsdf_clearance_params prm;
  svsdf_clearance_params_default(&prm);
  if (params) {
    if (params->struct_size != sizeof(svsdf_clearance_params))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_min_clearance: struct_size is not sizeof(svsdf_clearance_params)");
    prm = *params;
  }
  if (!(prm.eps > 0.0) || !std::isfinite(prm.eps)) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_min_clearance: eps must be positive and finite");
  if (int rc = require_resident(ctx)) return rc;
  const svsdf_traj::TrajCheck chk = svsdf_traj::check_traj(N, coeffs, T);
  if (chk.code) return fail(ctx, chk.code, std::string("svsdf_min_clearance: ") + chk.reason);
  if (!(chk.td < 3 * 1e2))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_min_clearance: total duration >= 300 s (the reference's stale-duration regime)");
  svsdf_ctx *leaf = leaf_of(ctx);
  if ((ctx->scaled || leaf->scaled) && !(ctx->cfg.flags & SVSDF_FLAG_SCALED_CLEARANCE))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_min_clearance: a scale schedule is set and the context was created without "
                                        "SVSDF_FLAG_SCALED_CLEARANCE (the bound is the rigid one)");
  if (!leaf->lipschitz_ok)
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_min_clearance: the shape SDF failed the context's Lipschitz self-check");
  if (ctx->subs.empty()) return min_clearance_leaf(ctx, N, coeffs, T, prm, out);

  // every stripe on its own device; the host combines
  const size_t G = ctx->subs.size();
  std::vector<svsdf_clearance_result> res(G);
  size_t Ptot = 0;
  for (svsdf_ctx *s : ctx->subs) Ptot += s->P;
  const int rcg = group_run(ctx, [&](int k) -> int {
    svsdf_clearance_params pk = prm;
    if (prm.max_evals && Ptot)
      pk.max_evals = std::max<unsigned long long>(1ull, (unsigned long long)std::ceil((double)prm.max_evals * (double)ctx->subs[k]->P / (double)Ptot));
    return min_clearance_leaf(ctx->subs[k], N, coeffs, T, pk, &res[k]);
  });
  if (rcg) return rcg;
  svsdf_clearance_result r = res[0];
  bool any_budget = res[0].status == SVSDF_CLEARANCE_BUDGET;
  for (size_t k = 1; k < G; ++k) {
    const svsdf_clearance_result &q = res[k];
    any_budget = any_budget || q.status == SVSDF_CLEARANCE_BUDGET;
    const double lower = std::min(r.lower, q.lower);
    const int levels = std::max(r.levels, q.levels);
    const double ms = std::max(r.device_ms, q.device_ms);
    const unsigned long long evals = r.evals + q.evals, pairs = r.pairs + q.pairs, tp = r.tile_pairs + q.tile_pairs,
                             tk = r.tile_pairs_kept + q.tile_pairs_kept;
    const bool take = q.point_index >= 0 && (r.point_index < 0 || q.upper < r.upper || (q.upper == r.upper && q.point_index < r.point_index));
    if (take) r = q;
    r.lower = lower; r.levels = levels; r.device_ms = ms; r.evals = evals; r.pairs = pairs; r.tile_pairs = tp; r.tile_pairs_kept = tk;
  }
  const bool has_target = prm.target == prm.target;
  if (has_target && r.lower >= prm.target) r.status = SVSDF_CLEARANCE_SAFE;
  else if (has_target && r.upper < prm.target) r.status = SVSDF_CLEARANCE_UNSAFE;
  else r.status = any_budget ? SVSDF_CLEARANCE_BUDGET : SVSDF_CLEARANCE_CONVERGED;
  *out = r;
  return SVSDF_OK;
}

void svsdf_point_clearance_params_default(svsdf_point_clearance_params *p) {
  if (!p) return;
  *p = svsdf_point_clearance_params{};
  p->struct_size = sizeof(svsdf_point_clearance_params);
  p->eps = 1e-3;
  p->cap = std::numeric_limits<double>::infinity();
  p->target = std::numeric_limits<double>::quiet_NaN();
  p->max_evals = 0;
  p->pair_capacity = 0;
}

int svsdf_point_clearance(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, const svsdf_point_clearance_params *params,
                          double *lower, double *upper, double *t_witness, unsigned char *state, svsdf_point_clearance_result *out) {
  if (!ctx || !coeffs || !T || !out) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: null argument");
  svsdf_point_clearance_params prm;
  svsdf_point_clearance_params_default(&prm);
  if (params) {
    if (params->struct_size != sizeof(svsdf_point_clearance_params))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: struct_size is not sizeof(svsdf_point_clearance_params)");
    prm = *params;
  }
  if (!(prm.eps > 0.0) || !std::isfinite(prm.eps)) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: eps must be positive and finite");
  if (prm.cap != prm.cap) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: cap must not be NaN");
  if (int rc = require_resident(ctx)) return rc;
  const svsdf_traj::TrajCheck chk = svsdf_traj::check_traj(N, coeffs, T);
  if (chk.code) return fail(ctx, chk.code, std::string("svsdf_point_clearance: ") + chk.reason);
  if (!(chk.td < 3 * 1e2))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: total duration >= 300 s (the reference's stale-duration regime)");
  svsdf_ctx *leaf = leaf_of(ctx);
  if ((ctx->scaled || leaf->scaled) && !(ctx->cfg.flags & SVSDF_FLAG_SCALED_CLEARANCE))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: a scale schedule is set and the context was created without "
                                        "SVSDF_FLAG_SCALED_CLEARANCE (the bound is the rigid one)");
  if (!leaf->lipschitz_ok)
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_point_clearance: the shape SDF failed the context's Lipschitz self-check");
  if (ctx->subs.empty()) return point_clearance_leaf(ctx, N, coeffs, T, prm, lower, upper, t_witness, state, out);

  // every stripe on its own device, writing its own points of the caller's arrays; the host combines the structs
  const size_t G = ctx->subs.size();
  std::vector<svsdf_point_clearance_result> res(G);
  size_t Ptot = 0;
  for (svsdf_ctx *s : ctx->subs) Ptot += s->P;
  const int rcg = group_run(ctx, [&](int k) -> int {
    svsdf_point_clearance_params pk = prm;
    if (prm.max_evals && Ptot)
      pk.max_evals = std::max<unsigned long long>(1ull, (unsigned long long)std::ceil((double)prm.max_evals * (double)ctx->subs[k]->P / (double)Ptot));
    return point_clearance_leaf(ctx->subs[k], N, coeffs, T, pk, lower, upper, t_witness, state, &res[k]);
  });
  if (rcg) return rcg;
  svsdf_point_clearance_result r = res[0];
  for (size_t k = 1; k < G; ++k) {
    const svsdf_point_clearance_result &q = res[k];
    if (q.point_index >= 0 && (r.point_index < 0 || q.upper < r.upper || (q.upper == r.upper && q.point_index < r.point_index))) {
      r.upper = q.upper; r.t_witness = q.t_witness; r.point_index = q.point_index;
    }
    r.lower = std::min(r.lower, q.lower);
    r.levels = std::max(r.levels, q.levels);
    r.device_ms = std::max(r.device_ms, q.device_ms);
    for (int i = 0; i < SVSDF_POINT_STATES; ++i) r.counts[i] += q.counts[i];
    r.evals += q.evals; r.pairs += q.pairs; r.tile_pairs += q.tile_pairs; r.tile_pairs_kept += q.tile_pairs_kept;
  }
  r.status = r.counts[SVSDF_POINT_OPEN] ? SVSDF_CLEARANCE_BUDGET : SVSDF_CLEARANCE_CONVERGED;
  *out = r;
  return SVSDF_OK;
}

}  // extern "C"
