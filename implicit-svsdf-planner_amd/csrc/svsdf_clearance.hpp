// svsdf_clearance.hpp -- device side of svsdf_min_clearance: a level-synchronous branch and bound over (point, time interval)
// pairs that brackets
//   c* = min over p in the resident cloud, t in [0, sum T] of getSDFAtTimeStamp<false>(p, t)      (SWM:741-750)
// (DESIGN.md §4e).  The bound is the one the exact cull rests on (svsdf_pipeline.hip upload_traj, scan_layer1): for a
// 1-Lipschitz shape SDF, a pose x(t) that moves at most V per second and turns at most W per second on an interval of half
// width h around m,
//   sdf(p, t) >= sdf(p, m) - h (V + W |p - x(m)|)            for every t of the interval.
// Intervals: [0, sum T] is cut into n0 equal intervals of width w <= 0.15 s (level 0); interval (j, k) of level L is the
// k-th of the 2^L equal parts of level-0 interval j, its midpoint (j + (2k + 1) / 2^(L+1)) w.  V and W are the level-0
// interval's (the host's Bernstein bounds), inherited by every descendant.
// Kernels:
//   k_clr_tiles    bounding circle of every run of 64 consecutive points of the resident SoA cloud
//   k_clr_mid      pose at every level-0 midpoint (pose_at: what every SDF-at-time evaluation inlines)
//   k_clr_broad    the cheap bound |c_tile - x(m)| - r_tile - h V - r_bound of every (tile, interval): its minimum, or the
//                  list of the pairs a threshold keeps
//   k_clr_level0<SHAPE>  one wave per kept (tile, interval): transform + shape SDF against the midpoint's pose
//   k_clr_level<SHAPE>   one lane per (point, interval) pair of a deeper level: pose_at + sdf_from_pose
//                        (each with a scaled instantiation, Scl = ClrScale: scale_inv + rel_scaled + shape_sdf, clr_lower_sc)
//   k_clr_reduce   fixed-order reduction of the blocks' partial results into one record the host reads
// A level's pruning threshold is a kernel argument, fixed by the host before the level starts; the only atomics are the
// integer slot counters of the compaction, so the SET of pairs a level emits, and with it every reported number, does not
// depend on the order the lanes ran in.
#pragma once
#include <hip/hip_runtime.h>

#include "svsdf_kernels.hpp"
#include "svsdf_ordkey.hpp"

namespace svsdf {

constexpr int kClrBlock = 256;
constexpr int kClrTile = 64;        // points per tile = lanes of a wave
constexpr int kClrMaxLevel = 44;    // h = w / 2^45 ~ 2e-15 s: below that an interval is a single double

struct ClrPair { unsigned pt, j; unsigned long long k; };   // shard-local point, level-0 interval, index within it
struct ClrTileCircle { double cx, cy, r; };
struct ClrTilePair { unsigned tile, j; };
// The best evaluation so far: smallest value, then smallest original point index, then smallest time.
struct ClrBest { double f; long long idx; double t; unsigned pt; unsigned pad_; };
struct ClrPartial { ClrBest best; double settled_min, open_min; unsigned long long evals; };
// What the host reads per launch.  out_count / overflow are written by the level kernels (integer atomics), the rest by k_clr_reduce.
struct ClrRecord { ClrBest best; double settled_min, open_min; unsigned long long evals, out_count; unsigned overflow, pad_; };

__host__ __device__ __forceinline__ bool clr_better(const ClrBest &a, const ClrBest &b) {
  return a.f < b.f || (a.f == b.f && (a.idx < b.idx || (a.idx == b.idx && a.t < b.t)));
}
__host__ __device__ __forceinline__ ClrBest clr_no_best() {
  ClrBest b;
  b.f = __builtin_huge_val(); b.idx = 0x7fffffffffffffffll; b.t = __builtin_huge_val(); b.pt = 0u; b.pad_ = 0u;
  return b;
}
// midpoint and half width of interval (j, k) of level L; every kernel and the host use this one expression
__host__ __device__ __forceinline__ double clr_half_width(double w, int L) { return __builtin_ldexp(w, -(L + 1)); }
__host__ __device__ __forceinline__ double clr_mid(unsigned j, unsigned long long k, int L, double w, double dur) {
  const double frac = __builtin_ldexp((double)(2ull * k + 1ull), -(L + 1));   // exact: 2k + 1 < 2^(L+1) <= 2^45
  const double m = ((double)j + frac) * w;
  return m < dur ? m : dur;
}
// the lane's lower bound over its interval: the allowance convention of the exact cull (upload_traj)
__device__ __forceinline__ double clr_lower(double f, double h, double V, double W, double D) {
  return f - (h * (V + W * D) * (1.0 + 1e-9) + 1e-9);
}

// ---- under a scale schedule (SVSDF_FLAG_SCALED_CLEARANCE; DESIGN.md §4e "Under a scale schedule"): the value is
// getSDFAtTimeStamp<true>, sdf(u(t)) with u(t) = R(t)^T S(t)^-1 (p - x(t)) (rel_scaled), and on the interval
//   sdf_sc(p, t) >= sdf_sc(p, m) - h (V Imax + W |u(m)| + Q |p - x(m)|)
// with Imax >= 1 / s_a(t) and Q >= |s_a'(t)| / s_a(t)^2 over the level-0 interval (svsdf_scale_bounds, inherited like V, W).
// The level kernels take the schedule as the parameter pack `Scl... scl_arg` of svsdf_kernels.hpp's ScaleArg idiom: empty
// for the rigid kernel, whose arguments and bits are then exactly those of a kernel without it, and exactly ClrScale -- the
// ScaleDev with the two per-interval arrays of the bound -- for the scaled one.
struct ClrScale { ScaleDev scl; const double *Imax, *Q; };
template <typename... Scl>
struct ClrScaleArg {
  static_assert(sizeof...(Scl) == 0, "the scale pack is empty (rigid kernel) or exactly ClrScale (scaled kernel)");
  static constexpr bool SC = false;
  static __device__ __forceinline__ ClrScale get() { return ClrScale{}; }
};
template <>
struct ClrScaleArg<ClrScale> {
  static constexpr bool SC = true;
  static __device__ __forceinline__ const ClrScale &get(const ClrScale &s) { return s; }
};
// U = |u(m)|, the norm of the rel_scaled output; Imax = 1, Q = 0, U = D is clr_lower
__device__ __forceinline__ double clr_lower_sc(double f, double h, double V, double W, double Imax, double Q, double D, double U) {
  return f - (h * (V * Imax + W * U + Q * D) * (1.0 + 1e-9) + 1e-9);
}
// One evaluation against pose p at time t and its bound over the half width h: the rigid pair (sdf_from_pose, clr_lower)
// or the scaled one (scale_inv, rel_scaled, shape_sdf: sdf_at_sc's value bit for bit; clr_lower_sc).
template <int SHAPE, bool SC>
__device__ __forceinline__ double clr_eval(const ShapeParams &sp, const ClrScale &cs, const Pose &p, double px, double py, double t,
                                           double h, const double *__restrict__ V_, const double *__restrict__ W_, unsigned j,
                                           double &lb) {
  const double dx = px - p.x, dy = py - p.y;
  if constexpr (SC) {
    double i00, i11, rx, ry;
    scale_inv(cs.scl, t, i00, i11);
    rel_scaled(p, px, py, i00, i11, rx, ry);
    const double f = shape_sdf<SHAPE>(sp, rx, ry);
    lb = clr_lower_sc(f, h, V_[j], W_[j], cs.Imax[j], cs.Q[j], sqrt(dx * dx + dy * dy), sqrt(rx * rx + ry * ry));
    return f;
  } else {
    const double f = sdf_from_pose<SHAPE>(sp, p, px, py);
    lb = clr_lower(f, h, V_[j], W_[j], sqrt(dx * dx + dy * dy));
    return f;
  }
}

// block-wide fixed-order reduction of the lanes' partials; thread 0 writes the block's
__device__ __forceinline__ void clr_block_reduce(ClrPartial mine, ClrPartial *__restrict__ out) {
  __shared__ ClrPartial s_part[kClrBlock];
  s_part[threadIdx.x] = mine;
  __syncthreads();
  for (int s = kClrBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s && (int)threadIdx.x + s < (int)blockDim.x) {
      ClrPartial a = s_part[threadIdx.x];
      const ClrPartial b = s_part[threadIdx.x + s];
      if (clr_better(b.best, a.best)) a.best = b.best;
      a.settled_min = b.settled_min < a.settled_min ? b.settled_min : a.settled_min;
      a.open_min = b.open_min < a.open_min ? b.open_min : a.open_min;
      a.evals += b.evals;
      s_part[threadIdx.x] = a;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = s_part[0];
}
__device__ __forceinline__ ClrPartial clr_no_partial() {
  ClrPartial p;
  p.best = clr_no_best(); p.settled_min = __builtin_huge_val(); p.open_min = __builtin_huge_val(); p.evals = 0ull;
  return p;
}

// A pair's verdict against the level's threshold: settled (its bound joins the settled minimum) or split into its halves.
// `emit == 0` (the seed evaluation): values only.
__device__ __forceinline__ void clr_settle_or_split(ClrPartial &mine, double lb, double thr, int emit, unsigned pt, unsigned j,
                                                    unsigned long long k, ClrPair *__restrict__ out, unsigned out_cap,
                                                    ClrRecord *__restrict__ rec) {
  if (!emit) return;
  if (lb >= thr) {
    mine.settled_min = lb < mine.settled_min ? lb : mine.settled_min;
    return;
  }
  mine.open_min = lb < mine.open_min ? lb : mine.open_min;
  const unsigned long long slot = atomicAdd(&rec->out_count, 2ull);
  if (slot + 2ull > (unsigned long long)out_cap) { rec->overflow = 1u; return; }   // (the host sizes the buffer for every pair splitting)
  ClrPair c;
  c.pt = pt; c.j = j; c.k = 2ull * k;
  out[slot] = c;
  c.k = 2ull * k + 1ull;
  out[slot + 1] = c;
}

// Level 0: wave v of the launch takes (tile, interval) pair tp[v], lane l the tile's point l.  The value is
// sdf_from_pose against the midpoint's pose from k_clr_mid, i.e. pose_at's pose: bit for bit sdf_at(p, m).
template <int SHAPE, typename... Scl>
__global__ void __launch_bounds__(kClrBlock)
k_clr_level0(ShapeParams sp, const double *__restrict__ px_, const double *__restrict__ py_, const long long *__restrict__ orig,
             unsigned P, const Pose *__restrict__ mid, const double *__restrict__ V_, const double *__restrict__ W_, double w,
             double dur, const ClrTilePair *__restrict__ tp, unsigned ntp, double thr, int emit, ClrPair *__restrict__ out,
             unsigned out_cap, ClrRecord *__restrict__ rec, ClrPartial *__restrict__ partials, Scl... scl_arg) {
  constexpr bool SC = ClrScaleArg<Scl...>::SC;
  const ClrScale cs = ClrScaleArg<Scl...>::get(scl_arg...);
  ClrPartial mine = clr_no_partial();
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = kClrBlock / 64;
  const double h = clr_half_width(w, 0);
  for (unsigned v = blockIdx.x * waves + wave; v < ntp; v += gridDim.x * waves) {
    const ClrTilePair q = tp[v];
    const unsigned pt = q.tile * (unsigned)kClrTile + lane;
    if (pt >= P) continue;
    const Pose p = mid[q.j];
    const double px = px_[pt], py = py_[pt];
    const double t = clr_mid(q.j, 0ull, 0, w, dur);
    double lb;
    const double f = clr_eval<SHAPE, SC>(sp, cs, p, px, py, t, h, V_, W_, q.j, lb);
    ClrBest b;
    b.f = f; b.idx = orig[pt]; b.t = t; b.pt = pt; b.pad_ = 0u;
    if (clr_better(b, mine.best)) mine.best = b;
    mine.evals += 1ull;
    clr_settle_or_split(mine, lb, thr, emit, pt, q.j, 0ull, out, out_cap, rec);
  }
  clr_block_reduce(mine, partials);
}

// Level L >= 1: lane per pair, the evaluation of k_debug_sdf_at (pose_at, sdf_from_pose, the context's piece-time mode).
template <int SHAPE, typename... Scl>
__global__ void __launch_bounds__(kClrBlock)
k_clr_level(const TrajDev *__restrict__ trg, ShapeParams sp, const double *__restrict__ px_, const double *__restrict__ py_,
            const long long *__restrict__ orig, const double *__restrict__ V_, const double *__restrict__ W_, double w, int L,
            const ClrPair *__restrict__ in, unsigned n, double thr, ClrPair *__restrict__ out, unsigned out_cap,
            ClrRecord *__restrict__ rec, ClrPartial *__restrict__ partials, Scl... scl_arg) {
  constexpr bool SC = ClrScaleArg<Scl...>::SC;
  const ClrScale cs = ClrScaleArg<Scl...>::get(scl_arg...);
  extern __shared__ double clr_lds[];
  const TrajL tr = stage_traj(trg, clr_lds);
  ClrPartial mine = clr_no_partial();
  const double h = clr_half_width(w, L);
  PieceCache pc = piece_cache_init();
  for (unsigned i = blockIdx.x * kClrBlock + threadIdx.x; i < n; i += gridDim.x * kClrBlock) {
    const ClrPair q = in[i];
    const double t = clr_mid(q.j, q.k, L, w, tr.dur);
    const Pose p = pose_at(tr, t, pc);
    const double px = px_[q.pt], py = py_[q.pt];
    double lb;
    const double f = clr_eval<SHAPE, SC>(sp, cs, p, px, py, t, h, V_, W_, q.j, lb);
    ClrBest b;
    b.f = f; b.idx = orig[q.pt]; b.t = t; b.pt = q.pt; b.pad_ = 0u;
    if (clr_better(b, mine.best)) mine.best = b;
    mine.evals += 1ull;
    clr_settle_or_split(mine, lb, thr, 1, q.pt, q.j, q.k, out, out_cap, rec);
  }
  clr_block_reduce(mine, partials);
}

// ---- svsdf_point_clearance: the same search with one minimum PER POINT ("per point").  Same intervals, same
// bound, same evaluations; what differs is where the running minima live and what a pair is settled against.
//   U[p]     smallest value evaluated so far for point p          S[p]    smallest bound of p's settled pairs
//   open[p]  smallest bound of p's pairs that split in the level that ran last      tw[p]   witness time of U[p]
// all as ord_key() keys lowered with the integer atomicMin: the minimum of a set does not depend on the order its members
// arrive in, so every array is the same from run to run.  A level settles pair (p, j, k) against snap[p], the copy of U[p]
// taken before the level's first launch (k_pclr_snapshot): the set of pairs a level emits depends neither on lane order nor
// on how the level was sliced.
// The witness: a lane that lowers U[p] stores the "none" key to tw[p] (every such store writes the same value); after the
// launch k_pclr_witness goes over the launch's evaluations and lowers tw[p] to the time of each one whose value equals
// U[p].  An evaluation of an earlier launch that still equals U[p] was recorded by that launch's pass and is not cleared,
// since U[p] did not go down after it: tw[p] ends as the smallest time among all evaluations that attain U[p].
// Kernels: k_pclr_seed, k_pclr_tile_max, k_pclr_broad (seed and broad phase per tile), k_pclr_snapshot,
// k_pclr_level0<SHAPE>, k_pclr_level<SHAPE>, k_pclr_witness (a level), k_pclr_final (brackets and states).
enum : unsigned char { kPclrConverged = 0, kPclrFar = 1, kPclrSafe = 2, kPclrUnsafe = 3, kPclrOpen = 4 };   // SVSDF_POINT_*
struct PclrState { unsigned long long *U, *S, *open, *tw; const unsigned long long *snap; };   // P keys each
struct PclrEval { double f, t; };                        // one per evaluation of a launch, beside its pair
struct PclrRule { double eps, cap, target; };            // target NaN: none
// What the host reads per launch; integer atomics only.
struct PclrCounters { unsigned long long out_count, evals; unsigned overflow, pad_; };

// Lower a key; true when this call did.  The plain load is a filter only: a stale value is never below the current one.
__device__ __forceinline__ bool pclr_key_min(unsigned long long *addr, unsigned long long key) {
  if (key >= __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
  return atomicMin(addr, key) > key;
}
__device__ __forceinline__ void pclr_value(const PclrState &s, unsigned pt, double f) {
  if (f == f && pclr_key_min(&s.U[pt], ord_key(f))) s.tw[pt] = kOrdKeyPosInf;   // (a NaN never becomes a minimum)
}

// A pair's verdict against its point's snapshot: settled iff lb >= min(snap - eps, cap), under a target also iff
// lb >= target or snap < target (the point is decided); any other pair splits into its halves.
__device__ __forceinline__ void pclr_settle_or_split(double lb, const PclrRule &r, const PclrState &s, unsigned pt, unsigned j,
                                                     unsigned long long k, ClrPair *__restrict__ out, unsigned out_cap,
                                                     PclrCounters *__restrict__ cnt) {
  const double u = ord_unkey(s.snap[pt]);
  const double a = u - r.eps, thr = a < r.cap ? a : r.cap;
  const bool settled = lb >= thr || (r.target == r.target && (lb >= r.target || u < r.target));
  const unsigned long long key = ord_key(lb == lb ? lb : -__builtin_huge_val());
  if (settled) { pclr_key_min(&s.S[pt], key); return; }
  pclr_key_min(&s.open[pt], key);
  const unsigned long long slot = atomicAdd(&cnt->out_count, 2ull);
  if (slot + 2ull > (unsigned long long)out_cap) { cnt->overflow = 1u; return; }   // (the host sizes the buffer for every pair splitting)
  ClrPair c;
  c.pt = pt; c.j = j; c.k = 2ull * k;
  out[slot] = c;
  c.k = 2ull * k + 1ull;
  out[slot + 1] = c;
}
// the lanes' evaluation counts: summed over the wave, one integer atomic per wave
__device__ __forceinline__ void pclr_count_evals(unsigned long long evals, PclrCounters *__restrict__ cnt) {
  for (int o = 32; o > 0; o >>= 1) evals += __shfl_down(evals, o);
  if ((threadIdx.x & 63u) == 0u && evals) atomicAdd(&cnt->evals, evals);
}

// Level 0 and the seed (`emit == 0`: values only): k_clr_level0's wave per (tile, interval), evaluation v * 64 + lane.
template <int SHAPE, typename... Scl>
__global__ void __launch_bounds__(kClrBlock)
k_pclr_level0(ShapeParams sp, const double *__restrict__ px_, const double *__restrict__ py_, unsigned P,
              const Pose *__restrict__ mid, const double *__restrict__ V_, const double *__restrict__ W_, double w, double dur,
              const ClrTilePair *__restrict__ tp, unsigned ntp, PclrRule rule, int emit, PclrState s, PclrEval *__restrict__ ev,
              ClrPair *__restrict__ out, unsigned out_cap, PclrCounters *__restrict__ cnt, Scl... scl_arg) {
  constexpr bool SC = ClrScaleArg<Scl...>::SC;
  const ClrScale cs = ClrScaleArg<Scl...>::get(scl_arg...);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = kClrBlock / 64;
  const double h = clr_half_width(w, 0);
  unsigned long long evals = 0ull;
  for (unsigned v = blockIdx.x * waves + wave; v < ntp; v += gridDim.x * waves) {
    const ClrTilePair q = tp[v];
    const unsigned pt = q.tile * (unsigned)kClrTile + lane;
    if (pt >= P) continue;
    const Pose p = mid[q.j];
    const double px = px_[pt], py = py_[pt];
    PclrEval e;
    e.t = clr_mid(q.j, 0ull, 0, w, dur);
    double lb;
    const double f = clr_eval<SHAPE, SC>(sp, cs, p, px, py, e.t, h, V_, W_, q.j, lb);
    e.f = f;
    ev[(size_t)v * kClrTile + lane] = e;
    evals += 1ull;
    pclr_value(s, pt, f);
    if (!emit) continue;
    pclr_settle_or_split(lb, rule, s, pt, q.j, 0ull, out, out_cap, cnt);
  }
  pclr_count_evals(evals, cnt);
}

// Level L >= 1: k_clr_level's lane per pair, evaluation i beside pair i.
template <int SHAPE, typename... Scl>
__global__ void __launch_bounds__(kClrBlock)
k_pclr_level(const TrajDev *__restrict__ trg, ShapeParams sp, const double *__restrict__ px_, const double *__restrict__ py_,
             const double *__restrict__ V_, const double *__restrict__ W_, double w, int L, const ClrPair *__restrict__ in,
             unsigned n, PclrRule rule, PclrState s, PclrEval *__restrict__ ev, ClrPair *__restrict__ out, unsigned out_cap,
             PclrCounters *__restrict__ cnt, Scl... scl_arg) {
  constexpr bool SC = ClrScaleArg<Scl...>::SC;
  const ClrScale cs = ClrScaleArg<Scl...>::get(scl_arg...);
  extern __shared__ double clr_lds[];
  const TrajL tr = stage_traj(trg, clr_lds);
  const double h = clr_half_width(w, L);
  PieceCache pc = piece_cache_init();
  unsigned long long evals = 0ull;
  for (unsigned i = blockIdx.x * kClrBlock + threadIdx.x; i < n; i += gridDim.x * kClrBlock) {
    const ClrPair q = in[i];
    const double t = clr_mid(q.j, q.k, L, w, tr.dur);
    const Pose p = pose_at(tr, t, pc);
    const double px = px_[q.pt], py = py_[q.pt];
    double lb;
    const double f = clr_eval<SHAPE, SC>(sp, cs, p, px, py, t, h, V_, W_, q.j, lb);
    PclrEval e;
    e.f = f; e.t = t;
    ev[i] = e;
    evals += 1ull;
    pclr_value(s, q.pt, f);
    pclr_settle_or_split(lb, rule, s, q.pt, q.j, q.k, out, out_cap, cnt);
  }
  pclr_count_evals(evals, cnt);
}

#ifdef SVSDF_CLR_TU   // shape-independent kernels: compiled once, by svsdf_clearance.hip

// Bounding circle of points [64 i, 64 i + 64) of the cloud: centre of their box, radius the largest distance to it, rounded up.
__global__ void __launch_bounds__(kClrBlock)
k_clr_tiles(const double *__restrict__ px, const double *__restrict__ py, unsigned P, unsigned ntiles, ClrTileCircle *__restrict__ tiles) {
  const unsigned i = blockIdx.x * kClrBlock + threadIdx.x;
  if (i >= ntiles) return;
  const unsigned p0 = i * (unsigned)kClrTile, p1 = (p0 + (unsigned)kClrTile < P) ? p0 + (unsigned)kClrTile : P;
  double x0 = px[p0], x1 = x0, y0 = py[p0], y1 = y0;
  for (unsigned p = p0 + 1; p < p1; ++p) {
    const double x = px[p], y = py[p];
    x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
    y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
  }
  ClrTileCircle c;
  c.cx = 0.5 * (x0 + x1); c.cy = 0.5 * (y0 + y1);
  double r2 = 0.0;
  for (unsigned p = p0; p < p1; ++p) {
    const double dx = px[p] - c.cx, dy = py[p] - c.cy;
    const double d2 = dx * dx + dy * dy;
    r2 = d2 > r2 ? d2 : r2;
  }
  c.r = sqrt(r2) * (1.0 + 1e-12);
  tiles[i] = c;
}

// Pose at the midpoint of every level-0 interval.  One wave per block, like k_debug_sdf_at.
__global__ void __launch_bounds__(64)
k_clr_mid(const TrajDev *__restrict__ trg, double w, unsigned n0, Pose *__restrict__ mid) {
  extern __shared__ double clr_mid_lds[];
  const TrajL tr = stage_traj(trg, clr_mid_lds);
  const unsigned j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n0) return;
  PieceCache pc = piece_cache_init();
  mid[j] = pose_at(tr, clr_mid(j, 0ull, 0, w, tr.dur), pc);
}

// cheap bound of (tile, interval): every point of the tile is at least this far outside the shape during the interval
__device__ __forceinline__ double clr_cheap(const ClrTileCircle c, const Pose p, double h, double V, double r_bound) {
  const double dx = c.cx - p.x, dy = c.cy - p.y;
  return sqrt(dx * dx + dy * dy) * (1.0 - 1e-12) - c.r - r_bound - (h * V * (1.0 + 1e-9) + 1e-9);
}

// Under a scale schedule (Smin_ / Smax_ not null: the per-interval bounds of s_a): with num = |c_tile - x(m)| - r_tile - h V,
// every point of the tile has |p - x(t)| >= num, |u| = |S^-1 (p - x)| >= |p - x| / Smax and sdf(u) >= |u| - r_bound, so
// num / Smax - r_bound bounds the tile from below when num >= 0.  When num < 0 the tile may reach the pose and -r_bound is
// all that holds; ANY value at or below it is a valid bound, and which one only orders the overlapping pairs -- that is, it
// picks the seed.  num Smin - r_bound ranks them by how deep the overlap is in the world times the smallest scale of the
// interval: a tile deep inside a LARGE robot first, where one of its points is likeliest to be interior and to give a first
// upper near the minimum (dividing by Smin instead would put the intervals where the robot is smallest first).
__device__ __forceinline__ double clr_cheap_sc(const ClrTileCircle c, const Pose p, double h, double V, double r_bound, double Smin,
                                               double Smax) {
  const double dx = c.cx - p.x, dy = c.cy - p.y;
  const double num = sqrt(dx * dx + dy * dy) * (1.0 - 1e-12) - c.r - (h * V * (1.0 + 1e-9) + 1e-9);
  return (num >= 0.0 ? num / Smax * (1.0 - 1e-12) : num * Smin) - r_bound;
}
__device__ __forceinline__ double clr_cheap_any(const ClrTileCircle c, const Pose p, double h, double V, double r_bound,
                                                const double *__restrict__ Smin_, const double *__restrict__ Smax_, unsigned j) {
  return Smax_ ? clr_cheap_sc(c, p, h, V, r_bound, Smin_[j], Smax_[j]) : clr_cheap(c, p, h, V, r_bound);
}

// list == null, count == null: the minimum of the cheap bound (ties: the smallest pair index) as block partials.
// count != null: the pairs with cheap <= thr are counted, and written to `list` when there is one (cap entries).
__global__ void __launch_bounds__(kClrBlock)
k_clr_broad(const ClrTileCircle *__restrict__ tiles, unsigned ntiles, const Pose *__restrict__ mid, const double *__restrict__ V_,
            unsigned n0, double w, double r_bound, double thr, ClrTilePair *__restrict__ list, unsigned long long cap,
            unsigned long long *__restrict__ count, ClrPartial *__restrict__ partials, const double *__restrict__ Smin_,
            const double *__restrict__ Smax_) {
  ClrPartial mine = clr_no_partial();
  const double h = clr_half_width(w, 0);
  const unsigned long long total = (unsigned long long)ntiles * n0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * kClrBlock + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * kClrBlock) {
    const unsigned tile = (unsigned)(i / n0), j = (unsigned)(i % n0);
    const double cheap = clr_cheap_any(tiles[tile], mid[j], h, V_[j], r_bound, Smin_, Smax_, j);
    if (count) {
      if (cheap <= thr) {
        const unsigned long long slot = atomicAdd(count, 1ull);
        if (list && slot < cap) { ClrTilePair q; q.tile = tile; q.j = j; list[slot] = q; }
      }
    } else {
      ClrBest b;
      b.f = cheap; b.idx = (long long)i; b.t = 0.0; b.pt = 0u; b.pad_ = 0u;
      if (clr_better(b, mine.best)) mine.best = b;
    }
  }
  if (!count) clr_block_reduce(mine, partials);
}

// one block: the blocks' partials in index order -> the record (out_count / overflow are the level kernels')
__global__ void __launch_bounds__(kClrBlock)
k_clr_reduce(const ClrPartial *__restrict__ partials, unsigned n, ClrRecord *__restrict__ rec) {
  __shared__ ClrPartial s_one[1];
  ClrPartial mine = clr_no_partial();
  for (unsigned i = threadIdx.x; i < n; i += kClrBlock) {
    const ClrPartial b = partials[i];
    if (clr_better(b.best, mine.best)) mine.best = b.best;
    mine.settled_min = b.settled_min < mine.settled_min ? b.settled_min : mine.settled_min;
    mine.open_min = b.open_min < mine.open_min ? b.open_min : mine.open_min;
    mine.evals += b.evals;
  }
  clr_block_reduce(mine, s_one);   // (blockIdx.x == 0: lands in s_one[0])
  __syncthreads();
  if (threadIdx.x == 0) { rec->best = s_one[0].best; rec->settled_min = s_one[0].settled_min; rec->open_min = s_one[0].open_min; rec->evals = s_one[0].evals; }
}

// ---- svsdf_point_clearance, shape-independent kernels

__global__ void __launch_bounds__(kClrBlock)
k_pclr_fill(unsigned long long *__restrict__ a, size_t n, unsigned long long value) {
  for (size_t i = (size_t)blockIdx.x * kClrBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kClrBlock) a[i] = value;
}

// Before a level's first launch: the thresholds' snapshot of U, and no open bound yet.
__global__ void __launch_bounds__(kClrBlock)
k_pclr_snapshot(const unsigned long long *__restrict__ U, unsigned long long *__restrict__ snap, unsigned long long *__restrict__ open,
                unsigned P) {
  for (unsigned p = blockIdx.x * kClrBlock + threadIdx.x; p < P; p += gridDim.x * kClrBlock) { snap[p] = U[p]; open[p] = kOrdKeyPosInf; }
}

// The seed: per tile the interval with the smallest cheap bound (ties: the smallest j) -- k_clr_broad's minimum, taken per
// tile.  One wave per tile.
__global__ void __launch_bounds__(kClrBlock)
k_pclr_seed(const ClrTileCircle *__restrict__ tiles, unsigned ntiles, const Pose *__restrict__ mid, const double *__restrict__ V_,
            unsigned n0, double w, double r_bound, ClrTilePair *__restrict__ seed, const double *__restrict__ Smin_,
            const double *__restrict__ Smax_) {
  const unsigned lane = threadIdx.x & 63u, tile = blockIdx.x * (kClrBlock / 64) + (threadIdx.x >> 6);
  if (tile >= ntiles) return;   // (the whole wave)
  const double h = clr_half_width(w, 0);
  const ClrTileCircle c = tiles[tile];
  double best = __builtin_huge_val();
  unsigned bj = 0xffffffffu;
  for (unsigned j = lane; j < n0; j += 64u) {
    const double cheap = clr_cheap_any(c, mid[j], h, V_[j], r_bound, Smin_, Smax_, j);
    if (cheap < best || bj == 0xffffffffu) { best = cheap == cheap ? cheap : __builtin_huge_val(); bj = j; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const unsigned oj = __shfl_xor(bj, o);
    if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
  }
  if (lane == 0u) { ClrTilePair q; q.tile = tile; q.j = bj; seed[tile] = q; }   // (n0 >= 1: lane 0 always holds an interval)
}

// After the seed: the largest U of every tile, and no dropped bound yet.
__global__ void __launch_bounds__(kClrBlock)
k_pclr_tile_max(const unsigned long long *__restrict__ U, unsigned P, unsigned ntiles, double *__restrict__ tmax,
                unsigned long long *__restrict__ tdrop) {
  const unsigned i = blockIdx.x * kClrBlock + threadIdx.x;
  if (i >= ntiles) return;
  const unsigned p0 = i * (unsigned)kClrTile, p1 = (p0 + (unsigned)kClrTile < P) ? p0 + (unsigned)kClrTile : P;
  unsigned long long m = U[p0];
  for (unsigned p = p0 + 1; p < p1; ++p) m = U[p] > m ? U[p] : m;
  tmax[i] = ord_unkey(m);
  tdrop[i] = kOrdKeyPosInf;
}

// The broad phase per tile: (tile, interval) is kept iff its cheap bound is <= min(cap, the tile's largest U).  A dropped
// pair's bound lies above every U[p] of its tile, or above cap: it cannot lower a U[p] (every value of the pair is above
// the bound), and it lowers lower[p] only below a cap -- through tdrop, the smallest dropped bound of the tile, which
// k_pclr_final takes into every lower[p] of the tile (without a cap it is above U[p] and changes nothing).
// list == null: count, and record the dropped bounds; list != null: fill (cap_entries entries).
__global__ void __launch_bounds__(kClrBlock)
k_pclr_broad(const ClrTileCircle *__restrict__ tiles, unsigned ntiles, const Pose *__restrict__ mid, const double *__restrict__ V_,
             unsigned n0, double w, double r_bound, double cap, const double *__restrict__ tmax, ClrTilePair *__restrict__ list,
             unsigned long long cap_entries, unsigned long long *__restrict__ count, unsigned long long *__restrict__ tdrop,
             const double *__restrict__ Smin_, const double *__restrict__ Smax_) {
  const double h = clr_half_width(w, 0);
  const unsigned long long total = (unsigned long long)ntiles * n0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * kClrBlock + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * kClrBlock) {
    const unsigned tile = (unsigned)(i / n0), j = (unsigned)(i % n0);
    const double cheap = clr_cheap_any(tiles[tile], mid[j], h, V_[j], r_bound, Smin_, Smax_, j);
    const double tm = tmax[tile], thr = cap < tm ? cap : tm;
    if (!(cheap > thr)) {
      const unsigned long long slot = atomicAdd(count, 1ull);
      if (list && slot < cap_entries) { ClrTilePair q; q.tile = tile; q.j = j; list[slot] = q; }
    } else if (!list) {
      pclr_key_min(&tdrop[tile], ord_key(cheap));
    }
  }
}

// After a launch: the witness time of every evaluation that attains its point's U.  tp != null: level 0 (evaluation
// v * 64 + lane of tile pair v), else pair i of `in`.
__global__ void __launch_bounds__(kClrBlock)
k_pclr_witness(const ClrTilePair *__restrict__ tp, const ClrPair *__restrict__ in, unsigned n, unsigned P,
               const PclrEval *__restrict__ ev, const unsigned long long *__restrict__ U, unsigned long long *__restrict__ tw) {
  for (unsigned i = blockIdx.x * kClrBlock + threadIdx.x; i < n; i += gridDim.x * kClrBlock) {
    const unsigned pt = tp ? tp[i >> 6].tile * (unsigned)kClrTile + (i & 63u) : in[i].pt;
    if (pt >= P) continue;
    const PclrEval e = ev[i];
    if (e.f == e.f && ord_key(e.f) == U[pt]) pclr_key_min(&tw[pt], ord_key(e.t));
  }
}

// The end of the search, in shard order: lower[p] = min(U, S, open, the tile's dropped bound), and the state.
__global__ void __launch_bounds__(kClrBlock)
k_pclr_final(unsigned P, PclrState s, const unsigned long long *__restrict__ tdrop, PclrRule r, double *__restrict__ lower,
             double *__restrict__ upper, double *__restrict__ tw, unsigned char *__restrict__ state) {
  for (unsigned p = blockIdx.x * kClrBlock + threadIdx.x; p < P; p += gridDim.x * kClrBlock) {
    const double u = ord_unkey(s.U[p]);
    unsigned long long k = s.U[p];
    k = s.S[p] < k ? s.S[p] : k;
    k = s.open[p] < k ? s.open[p] : k;
    k = tdrop[p / (unsigned)kClrTile] < k ? tdrop[p / (unsigned)kClrTile] : k;
    const double lo = ord_unkey(k);
    const bool has_target = r.target == r.target;
    unsigned char st = kPclrOpen;
    if (has_target && u < r.target) st = kPclrUnsafe;
    else if (has_target && lo >= r.target) st = kPclrSafe;
    else if (lo >= r.cap) st = kPclrFar;
    else if (u - lo <= r.eps) st = kPclrConverged;
    lower[p] = lo; upper[p] = u; tw[p] = ord_unkey(s.tw[p]); state[p] = st;
  }
}

#endif  // SVSDF_CLR_TU

}  // namespace svsdf
