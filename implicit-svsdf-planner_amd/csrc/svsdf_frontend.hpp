// svsdf_frontend.hpp -- SURVEY.md §8 row f3: the front end's consumers of the same shape SDFs.
//
//   k_subsw<SHAPE>         SweptVolumeManager::checkSubSWCollision (SWM:1171-1211), batched over A* edges
//   k_shape_kernels<SHAPE> BasicShape::initShape (SHP:386-430): occupancy of the kernel cells per yaw
//   k_yaw_free             kernelConv<true> (SWM:1033-1099) for every (cell, yaw kernel) of a map: the yaw-free table
//   kernel_bfs             checkKernelValue + visit_kernels_by_distance (SWM:1103-1169) on one cell's table word
//   k_succ<SHAPE>          the successor test of AstarPathSearcher::AstarGetSucc (front_end_Astar.hpp:192-241), batched
//   k_astar<SHAPE>         AstarPathSearch + getPath (front_end_Astar.hpp:243-390): the whole search, one workgroup
//
// Both are maps over independent (edge, obstacle point, interpolation step) / (yaw, cell) items with a
// boolean reduction; the reference's early exits only shorten its loops, they never change the result, so
// the order of evaluation is free.  FP64, strict arithmetic (no contraction), same operation order as the
// reference's Eigen expressions.
#pragma once
#include "svsdf_kernels.hpp"

namespace svsdf {

constexpr int kSubswPoints = 64;   // obstacle points per block (one per lane)
constexpr int kSubswBlock = 256;   // 4 waves share the interpolation steps of those points
constexpr int kMaxKt = 64;         // interpolation steps per edge (the reference loop yields 50: kt = 0 ... 0.98)

// One block = one (edge, 64-point chunk).  LDS holds the edge's interpolated poses
// linear_state(kt) = kt*child + (1-kt)*father (SWM:1191) with sin/cos of its yaw; lane = point, wave w takes
// the steps w, w+4, ...  hit_flag[e] starts at 0 and is set by any (point, step) with sdf < 0
// (SWM:1201-1204: `min_sdf < 0` can only become true through the current temp_sdf).
template <int SHAPE>
__global__ void __launch_bounds__(kSubswBlock)
k_subsw(ShapeParams sp, const double *__restrict__ father, const double *__restrict__ child,
        const unsigned long long *__restrict__ offs, const double *__restrict__ pts_xy,
        const double *__restrict__ kt_tab, int nkt, int *__restrict__ hit_flag) {
  __shared__ double s_x[kMaxKt], s_y[kMaxKt], s_c[kMaxKt], s_s[kMaxKt];
  const unsigned e = blockIdx.x;
  const unsigned long long p0 = offs[e], p1 = offs[e + 1];
  const unsigned long long first = p0 + (unsigned long long)blockIdx.y * kSubswPoints;
  if (first >= p1) return;
  if (threadIdx.x < (unsigned)nkt) {
    const double kt = kt_tab[threadIdx.x];
    const double omk = 1 - kt;
    const double lx = kt * child[3 * e + 0] + omk * father[3 * e + 0];
    const double ly = kt * child[3 * e + 1] + omk * father[3 * e + 1];
    const double yaw = kt * child[3 * e + 2] + omk * father[3 * e + 2];
    double sn, cs;
    sincos_exact(yaw, &sn, &cs);
    s_x[threadIdx.x] = lx; s_y[threadIdx.x] = ly; s_c[threadIdx.x] = cs; s_s[threadIdx.x] = sn;
  }
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long pi = first + lane;
  bool hit = false;
  if (pi < p1) {
    const double px = pts_xy[2 * pi], py = pts_xy[2 * pi + 1];
    for (int k = (int)wave; k < nkt; k += kSubswBlock / 64) {
      const double dx = px - s_x[k], dy = py - s_y[k];
      const double c = s_c[k], s = s_s[k];
      const double rx = c * dx + s * dy;       // posEva2Rel: Rt^T (p - x)  SWM:521-526
      const double ry = (-s) * dx + c * dy;
      if (shape_sdf<SHAPE>(sp, rx, ry) < 0) { hit = true; break; }
    }
  }
  if (__any(hit)) {
    if (lane == 0) hit_flag[e] = 1;
  }
}

// One thread per (yaw index, a, b) cell: x = resu*a - size_side*resu, y likewise (SHP:413-414),
// occupied iff getonlySDF(pos, R(yaw)) <= safemargin (SHP:418-423).
template <int SHAPE>
__global__ void __launch_bounds__(kBlock)
k_shape_kernels(ShapeParams sp, int ks, int count, double resu, int size_side, double safemargin,
                const double *__restrict__ yaw_tab, unsigned char *__restrict__ map) {
  const int cells = ks * ks;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)cells * count) return;
  const int ind = (int)(gid / cells);
  const int ab = (int)(gid - (long long)ind * cells);
  const int a = ab / ks, b = ab - a * ks;
  const double x = resu * a - size_side * resu;
  const double y = resu * b - size_side * resu;
  double sn, cs;
  sincos_exact(yaw_tab[ind], &sn, &cs);
  // (Polygon: consecutive lanes are consecutive cells b of one row a, so the wave's walk of svsdf_polygon.hpp sees
  // neighbouring list cells)
  map[gid] = (shape_sdf_rot<SHAPE>(sp, x, y, cs, sn) <= safemargin) ? 1 : 0;
}

// ---- yaw-kernel free-space table and batched A* successor test -------------------------------------------------------
//
// Bit layout shared by the packed map and the packed kernels: bit (y & 63) of word (y >> 6) of a row.  A map row is one
// row (fixed x) of the reference's INFLATED map (generateMapKernel2D, PCSmap_manager.h:81-108): (X + 2 side) rows of
// (Y + 2 side) bits, cell (x, y) at (x + side, y + side), zero outside the map, padded to `row_words` words so that the
// word after any cell's word exists.  A kernel row is row a of byte kernel k: bit b = kernels[k][a][b], zero from
// kernel_size on.  kernelConv<true>(k, (ix, iy, 0)) ANDs kernel row a with the bits [iy, iy + 8 bpl) of inflated row
// ix + a; the bits it reads past a row (or past the array) only meet kernel columns >= kernel_size, which are zero, so
// the test is `window(ix + a, iy) & kernel_row(k, a)` over kernel_size columns.
constexpr int kMaxKernelSize = 63;    // a kernel row is one word
constexpr int kMaxKernelCount = 64;   // a cell's mask is one word
constexpr int kYawFreeBlock = 256;    // 4 waves: 256 consecutive iy of one ix
constexpr int kYawFreeRowWords = kYawFreeBlock / 64 + 1;
constexpr int kSuccBlock = 256;
constexpr int kSuccPoints = 1024;     // obstacle cells a block of k_succ holds in LDS before it evaluates them

// Resident front-end map as the kernels see it (svsdf_frontend_set_map).
struct FrontMapDev {
  const unsigned long long *occ;    // inflated bitmap, (X + 2 side) x row_words
  const unsigned long long *free_;  // yaw-free table [ix * Y + iy]
  const double *kt;                 // the 50 accumulated interpolation steps of SWM:1189
  int nkt;
  int X, Y, side, row_words, kernel_count;
  double res, half;                 // cell size; half extent of getPointsInAABB2D: kernel_size / 2 + 1, in metres
  double bmin[3], bmax[3];
};

// checkKernelValue (SWM:1158-1169) + visit_kernels_by_distance (:1103-1156) on one cell's word of the yaw-free table.
// Returns 1 and writes both outputs when a kernel is found, 0 when none (outputs untouched), -1 when the father's index
// falls outside [0, kernel_count) (the reference indexes past its arrays there), -2 for a bad kernel_count.
// `pi` is sw_manager.hpp:20's literal, not the PI of the yaw table (Shape.hpp:31).
__host__ __device__ inline int kernel_bfs(unsigned long long free_mask, int kernel_count, double father_yaw,
                                          double *child_yaw, int *kernel_index) {
  if (kernel_count < 1 || kernel_count > kMaxKernelCount) return -2;
  const double pi = 3.1415926536;
  const double v = kernel_count * ((father_yaw + pi) / (2 * pi));
  if (!(v > -1.0 && v < (double)kernel_count)) return -1;   // (NaN too)
  const int father_i = (int)v;                               // truncation: (-1, 0) -> 0
  // the queue of the breadth-first search: at most 11 pops, two pushes each; one byte per entry in three words
  unsigned long long q0 = (unsigned long long)father_i, q1 = 0ull, q2 = 0ull;
  unsigned long long visited = 1ull << father_i;
  int head = 0, tail = 1, deep = 0;
  while (head < tail) {
    ++deep;
    const unsigned long long qw = head < 8 ? q0 : (head < 16 ? q1 : q2);
    const int x = (int)((qw >> ((head & 7) * 8)) & 0xffull);
    ++head;
    if ((free_mask >> x) & 1ull) {
      *kernel_index = x;
      *child_yaw = 2 * pi * x / kernel_count - pi;
      return 1;
    }
    for (int dir = -1; dir <= 1; dir += 2) {
      int nx = x + dir;
      if (nx < 0) nx = kernel_count - 1;
      if (nx >= kernel_count) nx = 0;
      if ((visited >> nx) & 1ull) continue;
      visited |= 1ull << nx;
      const unsigned long long e = (unsigned long long)nx << ((tail & 7) * 8);
      if (tail < 8) q0 |= e; else if (tail < 16) q1 |= e; else q2 |= e;
      ++tail;
    }
    if (deep > 10) break;
  }
  return 0;
}

#ifdef SVSDF_API_TU   // shape-independent kernels: compiled once, by svsdf_pipeline.hip
// Byte kernels of k_shape_kernels ([k][a][b], one byte per cell) -> one word per (k, a).
__global__ void __launch_bounds__(kBlock)
k_pack_kernel_rows(const unsigned char *__restrict__ map, int ks, int count, unsigned long long *__restrict__ rows) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ks * count) return;
  const unsigned char *m = map + (size_t)r * ks;
  unsigned long long w = 0ull;
  for (int b = 0; b < ks; ++b) w |= (unsigned long long)(m[b] != 0) << b;
  rows[r] = w;
}

// One block = 256 consecutive iy (blockIdx.y) of one ix (blockIdx.x), a wave = 64 of them.  LDS: the ks map rows
// ix .. ix + ks - 1 of the inflated bitmap (the 5 words the block's windows touch) and all kernel rows.  A lane forms
// its window of row a with a two-word funnel shift and tests it against the wave-uniform kernel words; every lane
// runs the same ks x count trip, the mask is stored once.
__global__ void __launch_bounds__(kYawFreeBlock)
k_yaw_free(const unsigned long long *__restrict__ occ, int row_words, const unsigned long long *__restrict__ krows,
           int ks, int count, int X, int Y, unsigned long long *__restrict__ free_out) {
  extern __shared__ unsigned long long yf_lds[];
  unsigned long long *s_map = yf_lds;                           // [ks][kYawFreeRowWords]
  unsigned long long *s_k = yf_lds + ks * kYawFreeRowWords;     // [count][ks]
  const int ix = blockIdx.x;
  const int w0 = blockIdx.y * (kYawFreeBlock / 64);
  for (int t = threadIdx.x; t < ks * kYawFreeRowWords; t += kYawFreeBlock) {
    const int a = t / kYawFreeRowWords, w = t - a * kYawFreeRowWords;
    s_map[t] = (w0 + w < row_words) ? occ[(size_t)(ix + a) * row_words + (w0 + w)] : 0ull;
  }
  for (int t = threadIdx.x; t < ks * count; t += kYawFreeBlock) s_k[t] = krows[t];
  __syncthreads();
  const int iy = blockIdx.y * kYawFreeBlock + threadIdx.x;
  if (iy >= Y) return;
  const int wq = threadIdx.x >> 6, sh = iy & 63;
  unsigned long long hit = 0ull;
  for (int a = 0; a < ks; ++a) {
    const unsigned long long lo = s_map[a * kYawFreeRowWords + wq], hi = s_map[a * kYawFreeRowWords + wq + 1];
    const unsigned long long win = sh ? ((lo >> sh) | (hi << (64 - sh))) : lo;
    for (int k = 0; k < count; ++k)
      hit |= (unsigned long long)((win & s_k[k * ks + a]) != 0ull) << k;
  }
  const unsigned long long all = count >= 64 ? ~0ull : ((1ull << count) - 1ull);
  free_out[(size_t)ix * Y + iy] = ~hit & all;
}
#endif  // SVSDF_API_TU

// getGridIndex (Gridmap3D.cpp:137-177) of a coordinate that projInMap (PCSmap_manager.h:128-135) has clamped into the map
__device__ __forceinline__ int succ_box_index(double c, double half, double bmin, double bmax, double res, int size) {
  double a = c + half;
  if (a < bmin) a = bmin;
  if (a > bmax) a = bmax;
  int i = (int)floor((a - bmin) / res);
  if (i < 0) i = 0;
  if (i >= size) i = size - 1;
  return i;
}

// ---- the four stages of AstarGetSucc as device helpers: k_succ (one block per (parent, neighbour)) and k_astar (one block
// per search) run the same code, so a neighbour's stage and yaw do not depend on which kernel asked.
// stage: 0 accepted, 1 index invalid, 2 cell occupied, 3 no yaw kernel, 4 sub-swept-volume collision.

// Stages 1 - 3, one thread: isIndexValid, the cell's own bit (isIndexOccupiedFlate(vi, 0)), kernel_bfs on the cell's table
// word.  *cy: the chosen yaw, NaN when the child has none.
__device__ __forceinline__ int succ_cheap_stages(const FrontMapDev &fm, int vi, int vj, double fy, double *cy) {
  int ki = 0;
  *cy = __longlong_as_double(0x7ff8000000000000ll);
  if (vi < 0 || vi >= fm.X || vj < 0 || vj >= fm.Y) return 1;
  if ((fm.occ[(size_t)(vi + fm.side) * fm.row_words + ((vj + fm.side) >> 6)] >> ((vj + fm.side) & 63)) & 1ull) return 2;
  if (kernel_bfs(fm.free_[(size_t)vi * fm.Y + vj], fm.kernel_count, fy, cy, &ki) != 1) return 3;
  return 0;
}

// Interpolated pose k of the edge (parent cell, fy) -> (child cell, cy): linear_state(kt) of SWM:1191 with sin / cos of its
// yaw, cell centres by getGridCubeCenter (Gridmap3D.cpp:184-195).  One thread per k < fm.nkt.
__device__ __forceinline__ void succ_pose(const FrontMapDev &fm, int pi_, int pj_, int vi, int vj, double fy, double cy, int k,
                                          double *s_x, double *s_y, double *s_c, double *s_s) {
  const double fx = (pi_ + 0.5) * fm.res + fm.bmin[0], fyy = (pj_ + 0.5) * fm.res + fm.bmin[1];
  const double cx = (vi + 0.5) * fm.res + fm.bmin[0], cyy = (vj + 0.5) * fm.res + fm.bmin[1];
  const double kt = fm.kt[k];
  const double omk = 1 - kt;
  const double lx = kt * cx + omk * fx;
  const double ly = kt * cyy + omk * fyy;
  const double yaw = kt * cy + omk * fy;
  double sn, cs;
  sincos_exact(yaw, &sn, &cs);
  s_x[k] = lx; s_y[k] = ly; s_c[k] = cs; s_s[k] = sn;
}

// Stage 4, the whole block of BLOCK threads (every thread must call it; it synchronises).  Walks the index box of
// getPointsInAABB2D (PCSmap_manager.h:137-158) around the child BLOCK cells at a time, compacts the occupied ones into the
// LDS list s_pi / s_pj (kSuccPoints entries; __ballot + popcount prefix over s_wcnt[BLOCK / 64]) and deals the (point, step)
// pairs of checkSubSWCollision over the threads, exactly as k_subsw evaluates them against the poses s_x .. s_s.  Returns
// the same value in every thread: true when some pair has sdf < 0.  The first barrier inside also orders the caller's
// writes of the poses before their use.
template <int SHAPE, int BLOCK>
__device__ __forceinline__ bool succ_collides(const ShapeParams &sp, const FrontMapDev &fm, int vi, int vj, const double *s_x,
                                              const double *s_y, const double *s_c, const double *s_s, int *s_pi, int *s_pj,
                                              int *s_wcnt) {
  static_assert(kSuccPoints >= 2 * BLOCK, "one more chunk must fit behind the flush threshold");
  const double cx = (vi + 0.5) * fm.res + fm.bmin[0], cyy = (vj + 0.5) * fm.res + fm.bmin[1];
  const int i1 = succ_box_index(cx, -fm.half, fm.bmin[0], fm.bmax[0], fm.res, fm.X);
  const int i2 = succ_box_index(cx, fm.half, fm.bmin[0], fm.bmax[0], fm.res, fm.X);
  const int j1 = succ_box_index(cyy, -fm.half, fm.bmin[1], fm.bmax[1], fm.res, fm.Y);
  const int j2 = succ_box_index(cyy, fm.half, fm.bmin[1], fm.bmax[1], fm.res, fm.Y);
  const unsigned bh = (unsigned)(j2 - j1 + 1);
  const unsigned long long total = (i2 >= i1 && j2 >= j1) ? (unsigned long long)(i2 - i1 + 1) * bh : 0ull;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  int n = 0;          // points in the list: every thread keeps the same count
  bool hit = false;
  for (unsigned long long base = 0; base < total; base += BLOCK) {
    const unsigned long long c = base + threadIdx.x;
    bool occ = false;
    int ci = 0, cj = 0;
    if (c < total) {
      ci = i1 + (int)(c / bh);
      cj = j1 + (int)(c % bh);
      occ = (fm.occ[(size_t)(ci + fm.side) * fm.row_words + ((cj + fm.side) >> 6)] >> ((cj + fm.side) & 63)) & 1ull;
    }
    const unsigned long long bal = __ballot(occ);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();   // (also: the poses are written, the previous flush has read the list)
    int off = n, add = 0;
    for (unsigned w = 0; w < BLOCK / 64; ++w) {
      if (w < wave) off += s_wcnt[w];
      add += s_wcnt[w];
    }
    if (occ) {
      const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
      s_pi[at] = ci; s_pj[at] = cj;
    }
    n += add;
    __syncthreads();
    if (n > kSuccPoints - BLOCK || base + BLOCK >= total) {
      const unsigned pairs = (unsigned)n * (unsigned)fm.nkt;
      for (unsigned q = threadIdx.x; q < pairs && !hit; q += BLOCK) {
        const unsigned ip = q / (unsigned)fm.nkt, k = q - ip * (unsigned)fm.nkt;
        const double px = (s_pi[ip] + 0.5) * fm.res + fm.bmin[0], py = (s_pj[ip] + 0.5) * fm.res + fm.bmin[1];
        const double dx = px - s_x[k], dy = py - s_y[k];
        const double c_ = s_c[k], s_ = s_s[k];
        const double rx = c_ * dx + s_ * dy;       // posEva2Rel: Rt^T (p - x)  SWM:521-526
        const double ry = (-s_) * dx + c_ * dy;
        if (shape_sdf<SHAPE>(sp, rx, ry) < 0) hit = true;
      }
      n = 0;
      if (__syncthreads_or(hit)) { hit = true; break; }   // a pure AND: a found collision ends the edge
    }
  }
  return hit;
}

// One block = one (parent, neighbour): e = 9 p + 3 (i + 1) + (j + 1), the loop order of AstarGetSucc.  Thread 0 runs the
// cheap stages and the block goes on only for a child that has a yaw.
template <int SHAPE>
__global__ void __launch_bounds__(kSuccBlock)
k_succ(ShapeParams sp, FrontMapDev fm, const int *__restrict__ parent_ij, const double *__restrict__ parent_yaw,
       double *__restrict__ yaw_out, unsigned char *__restrict__ stage_out) {
  __shared__ double s_x[kMaxKt], s_y[kMaxKt], s_c[kMaxKt], s_s[kMaxKt];
  __shared__ int s_pi[kSuccPoints], s_pj[kSuccPoints];
  __shared__ int s_wcnt[kSuccBlock / 64];
  __shared__ int s_stage;
  __shared__ double s_cy;
  const unsigned e = blockIdx.x;
  const unsigned p = e / 9u, slot = e - 9u * p;
  const int pi_ = parent_ij[2 * p], pj_ = parent_ij[2 * p + 1];
  const int vi = pi_ + (int)(slot / 3u) - 1, vj = pj_ + (int)(slot % 3u) - 1;
  const double fy = parent_yaw[p];
  if (threadIdx.x == 0) {
    double cy;
    const int stage = succ_cheap_stages(fm, vi, vj, fy, &cy);
    s_stage = stage;
    s_cy = cy;
    if (stage) { yaw_out[e] = cy; stage_out[e] = (unsigned char)stage; }
  }
  __syncthreads();
  if (s_stage) return;
  const double cy = s_cy;
  if (threadIdx.x < (unsigned)fm.nkt) succ_pose(fm, pi_, pj_, vi, vj, fy, cy, (int)threadIdx.x, s_x, s_y, s_c, s_s);
  const bool hit = succ_collides<SHAPE, kSuccBlock>(sp, fm, vi, vj, s_x, s_y, s_c, s_s, s_pi, s_pj, s_wcnt);
  if (threadIdx.x == 0) { yaw_out[e] = cy; stage_out[e] = hit ? 4 : 0; }
}

// ---- A* search on the resident map: AstarPathSearcher::AstarPathSearch + getPath (front_end_Astar.hpp:243-390) -------------
//
// One workgroup runs one search; a launch advances it by at most `slice` pops and leaves everything it knows -- node
// records, open set, counters -- in device memory, so the next launch goes on where this one stopped.  No waiting on other
// workgroups, flags or the host: every loop is bounded by the data or by `slice`.
//
// Open set: the reference's std::multimap<double, GridNode*> pops begin(), the smallest key and among equal keys the one
// inserted first.  Here: an unordered array of (key, insertion sequence number, cell); pop = block-wide lexicographic
// argmin over (key, seq), removal = swap with the last entry, push = append.  A node is in the set at most once (pushed on
// id 0 -> 1 and -1 -> 1 only, removed on pop; the id == 1 branch rewrites the node's fScore, not the key), so X * Y + 1
// entries are exact.
constexpr int kAstarBlock = 512;          // 8 waves: up to 256 VGPRs each, no instantiation spills
constexpr int kAstarStartNode = -2;       // `father` / open-set cell of the reference's separate startPtr
constexpr int kAstarRunning = -1;         // status between launches; final values: enum svsdf_astar_status
constexpr int kAstarOverflow = 4;         // internal: the open set or the path outgrew its exact capacity (cannot happen)
constexpr int kAstarDefaultSlice = 256;

struct AstarState {
  int status, started, n_open, path_len;
  int si, sj, gi, gj;
  unsigned long long seq, max_expansions;
  unsigned long long expansions, pushes, relaxed_open, reopened;
  unsigned long long stage_counts[5];
  double start_yaw, g_goal;
};
struct AstarDev {
  AstarState *st;
  signed char *id;                  // node records [ix * Y + iy]: 0 new, 1 open, -1 closed
  double *g, *f, *yaw;
  int *father;                      // cell of the father, -1 none, kAstarStartNode
  double *okey;                     // open set, open_cap entries
  unsigned long long *oseq;
  int *ocell;
  int *path_cell;                   // found path, start first; open_cap entries
  double *path_yaw;
  int open_cap;                     // X * Y + 1
};

// getHeu (front_end_Astar.hpp:165-182) with dz = 0, evaluated left to right
__host__ __device__ inline double astar_heu(int i, int j, int gi, int gj) {
  const double p = 1.0 / 1000;
  const int dx = i > gi ? i - gi : gi - i, dy = j > gj ? j - gj : gj - j, dz = 0;
  const int m2 = dy < dz ? dy : dz, dmin = dx < m2 ? dx : m2;
  const int M2 = dy > dz ? dy : dz, dmax = dx > M2 ? dx : M2;
  const int dmid = dx + dy + dz - dmin - dmax;
  const double h = 1.7320508075688772 /* sqrt(3) */ * dmin + 1.4142135623730951 /* sqrt(2) */ * (dmid - dmin) + (dmax - dmid);
  return h * (1 + p);
}

template <int SHAPE>
__global__ void __launch_bounds__(kAstarBlock)
k_astar(ShapeParams sp, FrontMapDev fm, AstarDev a, int slice) {
  __shared__ double s_x[9 * kMaxKt], s_y[9 * kMaxKt], s_c[9 * kMaxKt], s_s[9 * kMaxKt];   // poses of the nine edges
  __shared__ int s_pi[kSuccPoints], s_pj[kSuccPoints];
  __shared__ int s_wcnt[kAstarBlock / 64];
  __shared__ double s_rf[kAstarBlock / 64];
  __shared__ unsigned long long s_rs[kAstarBlock / 64];
  __shared__ int s_ri[kAstarBlock / 64];
  __shared__ int s_stage[9], s_nid[9];
  __shared__ double s_cy[9], s_ng[9];
  __shared__ AstarState S;
  __shared__ int s_cur, s_ci, s_cj;     // the popped node: its cell (kAstarStartNode: the start node) and index
  __shared__ double s_fy, s_gcur;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) {
    S = *a.st;
    if (!S.started) {   // AstarPathSearch :266-287: the start node enters the open set, the map's start cell is marked
      S.started = 1;
      const double h = astar_heu(S.si, S.sj, S.gi, S.gj);
      a.okey[0] = h; a.oseq[0] = 0ull; a.ocell[0] = kAstarStartNode;
      S.n_open = 1; S.seq = 1ull;
      const int sc = S.si * fm.Y + S.sj;
      a.id[sc] = 1; a.g[sc] = 0.0; a.f[sc] = h;
    }
  }
  __syncthreads();
  for (int it = 0; it < slice; ++it) {
    if (S.status != kAstarRunning) break;
    // ---- pop: argmin over (key, seq)
    const int n = S.n_open;
    double bf = __longlong_as_double(0x7ff0000000000000ll);
    unsigned long long bs = ~0ull;
    int bi = -1;
    for (int q = (int)tid; q < n; q += kAstarBlock) {
      const double kf = a.okey[q];
      const unsigned long long ks = a.oseq[q];
      if (kf < bf || (kf == bf && ks < bs)) { bf = kf; bs = ks; bi = q; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double of = __shfl_xor(bf, o);
      const unsigned long long os = __shfl_xor(bs, o);
      const int oi = __shfl_xor(bi, o);
      if (of < bf || (of == bf && os < bs)) { bf = of; bs = os; bi = oi; }
    }
    if (lane == 0) { s_rf[wave] = bf; s_rs[wave] = bs; s_ri[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kAstarBlock / 64; ++w)
        if (s_rf[w] < bf || (s_rf[w] == bf && s_rs[w] < bs)) { bf = s_rf[w]; bs = s_rs[w]; bi = s_ri[w]; }
      const int cur = a.ocell[bi];
      const int last = n - 1;          // openSet.erase(iter)
      if (bi != last) { a.okey[bi] = a.okey[last]; a.oseq[bi] = a.oseq[last]; a.ocell[bi] = a.ocell[last]; }
      S.n_open = last;
      s_cur = cur;
      if (cur == kAstarStartNode) {
        s_ci = S.si; s_cj = S.sj; s_fy = S.start_yaw; s_gcur = 0.0;
      } else {
        s_ci = cur / fm.Y; s_cj = cur - s_ci * fm.Y; s_fy = a.yaw[cur]; s_gcur = a.g[cur];
        a.id[cur] = -1;
      }
      if (s_ci == S.gi && s_cj == S.gj) {   // the goal test, before expansion; then getPath (:367-390)
        S.status = 0;
        S.g_goal = s_gcur;
        int len = 1, c = cur;
        while (c != kAstarStartNode && len <= a.open_cap) { c = a.father[c]; if (c == -1) break; ++len; }
        if (c != kAstarStartNode || len > a.open_cap) {
          S.status = kAstarOverflow;
        } else {
          S.path_len = len;
          c = cur;
          for (int k = len - 1; k >= 0; --k) {
            if (c == kAstarStartNode) { a.path_cell[k] = S.si * fm.Y + S.sj; a.path_yaw[k] = S.start_yaw; }
            else { a.path_cell[k] = c; a.path_yaw[k] = a.yaw[c]; c = a.father[c]; }
          }
        }
      }
    }
    __syncthreads();
    if (S.status != kAstarRunning) break;
    // ---- AstarGetSucc: stages 1 - 3 of the nine neighbours, one thread each; the neighbour's record rides along
    const int ci = s_ci, cj = s_cj;
    const double fy = s_fy;
    if (tid < 9u) {
      const int vi = ci + (int)(tid / 3u) - 1, vj = cj + (int)(tid % 3u) - 1;
      double cy;
      const int stage = succ_cheap_stages(fm, vi, vj, fy, &cy);
      s_stage[tid] = stage;
      s_cy[tid] = cy;
      if (stage == 0) { s_nid[tid] = a.id[vi * fm.Y + vj]; s_ng[tid] = a.g[vi * fm.Y + vj]; }
    }
    __syncthreads();
    if (tid < 9u * (unsigned)fm.nkt) {
      const unsigned c = tid / (unsigned)fm.nkt, k = tid - c * (unsigned)fm.nkt;
      if (s_stage[c] == 0)
        succ_pose(fm, ci, cj, ci + (int)(c / 3u) - 1, cj + (int)(c % 3u) - 1, fy, s_cy[c], (int)k, s_x + c * kMaxKt,
                  s_y + c * kMaxKt, s_c + c * kMaxKt, s_s + c * kMaxKt);
    }
    __syncthreads();
    // ---- stage 4, child after child: each tests exactly the cells of its own clamped index box
    for (unsigned c = 0; c < 9u; ++c) {
      if (s_stage[c] != 0) continue;
      const bool hit = succ_collides<SHAPE, kAstarBlock>(sp, fm, ci + (int)(c / 3u) - 1, cj + (int)(c % 3u) - 1, s_x + c * kMaxKt,
                                                         s_y + c * kMaxKt, s_c + c * kMaxKt, s_s + c * kMaxKt, s_pi, s_pj, s_wcnt);
      if (tid == 0 && hit) s_stage[c] = 4;
    }
    // ---- the three-way update of AstarPathSearch :315-358 for the accepted neighbours, in loop order
    if (tid == 0) {
      const double gcur = s_gcur;
      for (int c = 0; c < 9; ++c) {
        const int stage = s_stage[c];
        S.stage_counts[stage] += 1ull;
        if (stage != 0) continue;
        const int di = c / 3 - 1, dj = c % 3 - 1;
        const int vi = ci + di, vj = cj + dj, cell = vi * fm.Y + vj;
        const int e2 = di * di + dj * dj;
        const double ec = e2 == 0 ? 0.0 : (e2 == 1 ? 1.0 : 1.4142135623730951);   // sqrt(i*i + j*j)
        const double tg = ec + gcur;
        const int nid = s_nid[c];
        const bool fresh = nid == 0;
        if (!fresh && !(tg < s_ng[c])) continue;
        if (fresh) a.yaw[cell] = s_cy[c];     // :231-234: the yaw of a node's first discovery stays
        const double fs = tg + astar_heu(vi, vj, S.gi, S.gj);
        a.father[cell] = s_cur;
        a.g[cell] = tg;
        a.f[cell] = fs;
        if (nid == 1) { S.relaxed_open += 1ull; continue; }   // the multimap key stays
        if (S.n_open >= a.open_cap) { S.status = kAstarOverflow; break; }
        a.id[cell] = 1;
        a.okey[S.n_open] = fs; a.oseq[S.n_open] = S.seq; a.ocell[S.n_open] = cell;
        S.n_open += 1; S.seq += 1ull; S.pushes += 1ull;
        if (!fresh) S.reopened += 1ull;
      }
      S.expansions += 1ull;
      if (S.status == kAstarRunning) {
        if (S.n_open == 0) S.status = 1;
        else if (S.max_expansions != 0ull && S.expansions >= S.max_expansions) S.status = 2;
      }
    }
    __syncthreads();
  }
  if (tid == 0) *a.st = S;
}

// Diagnostic / test kernel (svsdf_debug_sdf_at): getSDFAtTimeStamp<false> (SWM:741-750) for arbitrary (point, time) pairs
// through the very pose_at / sdf_from_pose the solve kernels inline, with the intermediates: out[8 i ..] = sdf, x, y, cos,
// sin, body-frame x, body-frame y, piece-local-time path taken (0 cumulative, 1 / 2 chain).  One wave per block: the
// faithful piece-time chain works on whole waves.
// Scl = ScaleDev: the same under a time-varying scale (§4c), getSDFAtTimeStamp<true>, out8[5..6] = the scaled body-frame point u.
template <int SHAPE, typename... Scl>
__global__ void __launch_bounds__(64)
k_debug_sdf_at(const TrajDev *__restrict__ trg, ShapeParams sp, const double *__restrict__ pxy, const double *__restrict__ t_,
               int n, double *__restrict__ out, Scl... scl_arg) {
  constexpr bool SC = ScaleArg<Scl...>::SC;
  const ScaleDev scl = ScaleArg<Scl...>::get(scl_arg...);
  extern __shared__ double dbg_lds[];
  const TrajL tr = stage_traj(trg, dbg_lds);
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  PieceCache pc = piece_cache_init();
  const Pose p = pose_at(tr, t_[i], pc);
  const double px = pxy[2 * i], py = pxy[2 * i + 1];
  double *o = out + 8 * (size_t)i;
  double rx, ry;
  if constexpr (SC) {
    double i00, i11;
    scale_inv(scl, t_[i], i00, i11);
    rel_scaled(p, px, py, i00, i11, rx, ry);
    o[0] = shape_sdf<SHAPE>(sp, rx, ry);
  } else {
    const double dx = px - p.x, dy = py - p.y;
    rx = p.cs * dx + p.sn * dy;
    ry = (-p.sn) * dx + p.cs * dy;
    o[0] = sdf_from_pose<SHAPE>(sp, p, px, py);
  }
  o[1] = p.x; o[2] = p.y; o[3] = p.cs; o[4] = p.sn; o[5] = rx; o[6] = ry; o[7] = (double)tr.exact;
}

}  // namespace svsdf
