// svsdf_mapdev.hpp -- the query-point producer on the device: float32 cloud -> occupancy grid -> front-end bitmap ->
// waypoint-box gather -> AoS voxel centres in unified-id order, ready for the device planner (plan_cloud).  Included by
// svsdf_extras.hip alone; the kernels are shape-independent and are compiled there, under the build's -ffp-contract=off and
// without fast-math: (x - bmin) / res is the correctly rounded division, (i + 0.5) * res + bmin a multiply then an add.
//
// Behavioural spec: svsdf_host::OccupancyMap (svsdf_points.hpp), operation for operation, and through it the reference
//   PCS = src/map_manager/src/PCSmap_manager.cpp        rcvGlobalMapHandler :88-210
//   PCH = src/map_manager/include/map_manager/PCSmap_manager.h   unifiedID :118-125, projInMap :128-135,
//         getPointsInAABBOutOfLastOne :184-219
//   GRD = src/map_manager/src/Gridmap3D.cpp              createGridMap :25-41, isInMap :43-71, getGridIndex :137-177,
//         getGridCubeCenter :184-195, isIndexOccupied :239-283
// Deliberate differences, both refusals or omissions where the host code would misbehave: a non-finite cloud coordinate
// fails the build (the host casts floor(NaN) to int); a box index outside the grid -- only a map of zero cells has one --
// marks nothing (the host counts it as occupied and emits (0, 0, 0) points for it).
//
// Order guarantees.  Bounds and the occupied count: per-block partials, finished on the host in block order -- min, max and an
// integer sum, none of which depends on the order anyway.  Counts: integer atomics.  The gather: a set bit per unified id in a
// cleared bitmap (atomicOr: idempotent, so a voxel that several boxes reach is marked once), then popcount -> scan -> scatter
// in three launches, which writes ascending ids whatever order the marks arrived in.  No kernel waits for another workgroup:
// every dependency between workgroups is a kernel boundary on one stream, and every loop is bounded by its data.
#pragma once
#include "svsdf_ctx.hpp"
#include "svsdf_points.hpp"

namespace svsdf {

constexpr int kMapBlock = 256;
constexpr unsigned kMapMaxGrid = 1024;      // grid-stride kernels: blocks at most
constexpr double kMapSentinel = 999999999.0;   // PCS:11-12

struct MapGeom {   // svsdf_host::GridGeometry as the kernels take it
  double bmin[3], bmax[3], res;
  int X, Y, Z;
};

// GRD:43-71
__device__ __forceinline__ bool map_in_map(const MapGeom &g, double x, double y, double z) {
  return !(x < g.bmin[0] || y < g.bmin[1] || z < g.bmin[2] || x > g.bmax[0] || y > g.bmax[1] || z > g.bmax[2]);
}
// GRD:137-177, including its clamping quirk (a negative iy / iz resets ix)
__device__ __forceinline__ void map_grid_index(const MapGeom &g, double x, double y, double z, int id[3]) {
  if (!map_in_map(g, x, y, z)) { id[0] = id[1] = id[2] = 0; return; }
  int ix = (int)floor((x - g.bmin[0]) / g.res);
  int iy = (int)floor((y - g.bmin[1]) / g.res);
  int iz = (int)floor((z - g.bmin[2]) / g.res);
  if (ix < 0) ix = 0;
  if (ix >= g.X) ix = g.X - 1;
  if (iy < 0) ix = 0;
  if (iy >= g.Y) iy = g.Y - 1;
  if (iz < 0) ix = 0;
  if (iz >= g.Z) iz = g.Z - 1;
  id[0] = ix; id[1] = iy; id[2] = iz;
}

// sum over the block, valid in thread 0 (kMapBlock threads)
__device__ __forceinline__ unsigned map_block_sum(unsigned v) {
  __shared__ unsigned s_sum[kMapBlock / 64];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();   // (a second call in one kernel must not overwrite what the first one's thread 0 still reads)
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kMapBlock / 64; ++w) t += s_sum[w];
  return t;
}

// ---- 1. bounds (PCS:116-135): per-block [xmin, xmax, ymin, ymax, zmin, zmax] from the sentinels, and the block's count of
// non-finite coordinates.  The finish is the host's, in block order.
__global__ void __launch_bounds__(kMapBlock)
k_map_bounds(const float *__restrict__ xyz, size_t n, double *__restrict__ part, unsigned *__restrict__ part_bad) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double lo[3] = {kMapSentinel, kMapSentinel, kMapSentinel}, hi[3] = {-kMapSentinel, -kMapSentinel, -kMapSentinel};
  unsigned bad = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double v = (double)xyz[3 * i + d];
      if (!(fabs(v) < inf)) ++bad;   // NaN or inf
      if (v > hi[d]) hi[d] = v;
      if (v < lo[d]) lo[d] = v;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], m, 64));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], m, 64));
    }
  __shared__ double s[kMapBlock / 64][6];
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; ++d) { s[threadIdx.x >> 6][2 * d] = lo[d]; s[threadIdx.x >> 6][2 * d + 1] = hi[d]; }
  const unsigned nbad = map_block_sum(bad);   // (its barriers order the stores above too)
  if (threadIdx.x == 0) {
    for (int w = 1; w < kMapBlock / 64; ++w)
      for (int d = 0; d < 3; ++d) {
        s[0][2 * d] = fmin(s[0][2 * d], s[w][2 * d]);
        s[0][2 * d + 1] = fmax(s[0][2 * d + 1], s[w][2 * d + 1]);
      }
    for (int q = 0; q < 6; ++q) part[6 * (size_t)blockIdx.x + q] = s[0][q];
    part_bad[blockIdx.x] = nbad;
  }
}

// ---- 2. counting (PCS:137-160): one point per thread and pass, an integer atomic per point whose result nobody reads
__global__ void __launch_bounds__(kMapBlock)
k_map_count(const float *__restrict__ xyz, size_t n, MapGeom g, unsigned *__restrict__ cnt, size_t cells) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int id[3];
    map_grid_index(g, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], id);
    if (id[0] < 0 || id[1] < 0 || id[2] < 0) continue;
    const size_t a = ((size_t)id[0] * g.Y + id[1]) * g.Z + id[2];   // GridMap3D.h:129-130
    if (a < cells) atomicAdd(&cnt[a], 1u);
  }
}

// ---- 3. threshold (PCS:162-178): occ[a] = count[a] >= sta_threshold, and the block's occupied count
__global__ void __launch_bounds__(kMapBlock)
k_map_threshold(const unsigned *__restrict__ cnt, size_t cells, long long thr, unsigned char *__restrict__ occ,
                unsigned *__restrict__ part_occupied) {
  unsigned mine = 0;
  for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < cells; a += (size_t)gridDim.x * blockDim.x) {
    const unsigned char o = (long long)cnt[a] >= thr ? 1 : 0;
    occ[a] = o;
    mine += o;
  }
  const unsigned t = map_block_sum(mine);
  if (threadIdx.x == 0) part_occupied[blockIdx.x] = t;
}

// ---- 4. front-end bitmap (generateMapKernel2D, PCH:81-108, in 64-bit row words as svsdf_frontend_set_map packs it): layer
// k = 0, cell (x, y) at bit (y + side) of row x + side.  One thread builds one whole word.
__global__ void __launch_bounds__(kMapBlock)
k_map_front_bitmap(const unsigned char *__restrict__ occ, int X, int Y, int Z, int side, int row_words, size_t words,
                   unsigned long long *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= words) return;
  const long long x = (long long)(t / (size_t)row_words) - side;
  const long long y0 = (long long)(t % (size_t)row_words) * 64 - side;
  unsigned long long w = 0ull;
  if (x >= 0 && x < X)
    for (int b = 0; b < 64; ++b) {
      const long long y = y0 + b;
      if (y >= 0 && y < Y && occ[((size_t)x * Y + (size_t)y) * Z]) w |= 1ull << b;
    }
  out[t] = w;
}

// ---- 5. gather (PCH:184-219 for every centre, plan_manager.cpp:156-167).  boxes: 12 ints per centre, c1 c2 l1 l2
// (GridGeometry::centre_boxes).  A cell of the centre's box that lies outside the previous centre's and is occupied sets bit
// uid = k X Y + j X + i (PCH:118-125) of the bitmap, whose word 0 holds the ids from 32 * word0.
__global__ void __launch_bounds__(kMapBlock)
k_map_mark(const int *__restrict__ boxes, size_t ncentres, const unsigned char *__restrict__ occ, int X, int Y, int Z,
           size_t word0, size_t nwords, unsigned *__restrict__ bits) {
  for (size_t c = blockIdx.y; c < ncentres; c += gridDim.y) {
    const int *b = boxes + 12 * c;
    const int c1[3] = {b[0], b[1], b[2]}, c2[3] = {b[3], b[4], b[5]}, l1[3] = {b[6], b[7], b[8]}, l2[3] = {b[9], b[10], b[11]};
    if (c2[0] < c1[0] || c2[1] < c1[1] || c2[2] < c1[2]) continue;
    const size_t ny = (size_t)(c2[1] - c1[1]) + 1, nz = (size_t)(c2[2] - c1[2]) + 1;
    const size_t ncell = ((size_t)(c2[0] - c1[0]) + 1) * ny * nz;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < ncell; t += (size_t)gridDim.x * blockDim.x) {
      const int k = c1[2] + (int)(t % nz), j = c1[1] + (int)((t / nz) % ny), i = c1[0] + (int)(t / (nz * ny));
      if (i < 0 || i >= X || j < 0 || j >= Y || k < 0 || k >= Z) continue;
      if (!(i > l2[0] || i < l1[0] || j > l2[1] || j < l1[1] || k > l2[2] || k < l1[2])) continue;
      if (!occ[((size_t)i * Y + j) * Z + k]) continue;
      const size_t uid = ((size_t)k * Y + j) * X + i;
      const size_t w = (uid >> 5) - word0;   // (below word0: wraps, and fails the test)
      if (w < nwords) atomicOr(&bits[w], 1u << (uid & 31));
    }
  }
}

// set bits per block of kMapBlock words
__global__ void __launch_bounds__(kMapBlock)
k_map_block_counts(const unsigned *__restrict__ bits, size_t nwords, unsigned *__restrict__ bcount) {
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned t = map_block_sum(w < nwords ? (unsigned)__popc(bits[w]) : 0u);
  if (threadIdx.x == 0) bcount[blockIdx.x] = t;
}

// exclusive scan over the block: returns the sum of v over the threads below this one
__device__ __forceinline__ unsigned map_block_exclusive(unsigned v, unsigned *total) {
  __shared__ unsigned s_wave[kMapBlock / 64];
  unsigned inc = v;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned up = __shfl_up(inc, m, 64);
    if ((int)(threadIdx.x & 63) >= m) inc += up;
  }
  __syncthreads();   // (the previous round of a loop has read s_wave)
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int w = 0; w < kMapBlock / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) before += s_wave[w];
    all += s_wave[w];
  }
  *total = all;
  return before + inc - v;
}

// one block: exclusive scan of the block counts, a tile of kMapBlock at a time with a running carry; the grand total last
__global__ void __launch_bounds__(kMapBlock)
k_map_scan_blocks(const unsigned *__restrict__ bcount, size_t nblocks, unsigned *__restrict__ boff, unsigned *__restrict__ total) {
  unsigned carry = 0;
  for (size_t base = 0; base < nblocks; base += kMapBlock) {
    const size_t e = base + threadIdx.x;
    unsigned tile = 0;
    const unsigned ex = map_block_exclusive(e < nblocks ? bcount[e] : 0u, &tile);
    if (e < nblocks) boff[e] = carry + ex;
    carry += tile;
  }
  if (threadIdx.x == 0) *total = carry;
}

// the centres of the marked voxels (GRD:184-195), ascending unified id
__global__ void __launch_bounds__(kMapBlock)
k_map_scatter(const unsigned *__restrict__ bits, size_t nwords, size_t word0, const unsigned *__restrict__ boff, MapGeom g,
              double *__restrict__ out_xyz, size_t count) {
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned m = w < nwords ? bits[w] : 0u;
  unsigned tile = 0;
  size_t pos = (size_t)boff[blockIdx.x] + map_block_exclusive((unsigned)__popc(m), &tile);
  while (m) {   // at most 32 rounds
    const int b = __ffs((int)m) - 1;
    m &= m - 1u;
    const size_t uid = (word0 + w) * 32 + (size_t)b;
    const size_t i = uid % (size_t)g.X, j = (uid / (size_t)g.X) % (size_t)g.Y, k = uid / ((size_t)g.X * (size_t)g.Y);
    if (pos < count && k < (size_t)g.Z) {
      out_xyz[3 * pos] = ((double)(int)i + 0.5) * g.res + g.bmin[0];
      out_xyz[3 * pos + 1] = ((double)(int)j + 0.5) * g.res + g.bmin[1];
      out_xyz[3 * pos + 2] = ((double)(int)k + 0.5) * g.res + g.bmin[2];
    }
    ++pos;
  }
}

}  // namespace svsdf

namespace svsdf_impl {

inline unsigned map_grid(size_t n) { return (unsigned)std::min<size_t>((n + svsdf::kMapBlock - 1) / svsdf::kMapBlock, svsdf::kMapMaxGrid); }

inline svsdf_host::GridGeometry map_geometry(const ResidentMap &rm) {
  svsdf_host::GridGeometry g;
  g.res_ = rm.res;
  for (int d = 0; d < 3; ++d) { g.bmin_[d] = rm.bmin[d]; g.bmax_[d] = rm.bmax[d]; g.size_[d] = rm.dims[d]; }
  return g;
}
inline svsdf::MapGeom map_geom_dev(const ResidentMap &rm) {
  svsdf::MapGeom g;
  for (int d = 0; d < 3; ++d) { g.bmin[d] = rm.bmin[d]; g.bmax[d] = rm.bmax[d]; }
  g.res = rm.res; g.X = rm.dims[0]; g.Y = rm.dims[1]; g.Z = rm.dims[2];
  return g;
}

// svsdf_map_build_device on the context that owns a device.  d_cloud: n x 3 floats on ctx's device (null with n == 0).
inline int map_build(svsdf_ctx *ctx, const float *d_cloud, size_t n, double resolution, int sta_threshold) {
  using namespace svsdf;
  const char *what = "svsdf_map_build_device";
  hipStream_t st = ctx->stream;
  ResidentMap rm;
  rm.res = resolution; rm.sta_threshold = sta_threshold; rm.n_cloud = n;
  svsdf_host::GridGeometry geo;
  for (int d = 0; d < 3; ++d) { geo.bmin_[d] = kMapSentinel; geo.bmax_[d] = -kMapSentinel; }   // PCS:11-12
  if (n) {
    const unsigned grid = map_grid(n);
    Buf<double> d_part;
    Buf<unsigned> d_bad;
    int rc = d_part.alloc(ctx, (size_t)grid * 6);
    if (rc == SVSDF_OK) rc = d_bad.alloc(ctx, grid);
    if (rc) return rc;
    hipLaunchKernelGGL(k_map_bounds, dim3(grid), dim3(kMapBlock), 0, st, d_cloud, n, d_part.get(), d_bad.get());
    HIPCHK_AS(what, hipGetLastError());
    std::vector<double> hp((size_t)grid * 6);
    std::vector<unsigned> hb(grid);
    HIPCHK_AS(what, hipMemcpyAsync(hp.data(), d_part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(what, hipMemcpyAsync(hb.data(), d_bad, hb.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(what, hipStreamSynchronize(st));
    unsigned long long bad = 0;
    for (unsigned b = 0; b < grid; ++b) {
      bad += hb[b];
      for (int d = 0; d < 3; ++d) {
        if (hp[6 * (size_t)b + 2 * d + 1] > geo.bmax_[d]) geo.bmax_[d] = hp[6 * (size_t)b + 2 * d + 1];
        if (hp[6 * (size_t)b + 2 * d] < geo.bmin_[d]) geo.bmin_[d] = hp[6 * (size_t)b + 2 * d];
      }
    }
    if (bad)
      return fail(ctx, SVSDF_ERR_INVALID, std::string(what) + ": " + std::to_string(bad) + " non-finite coordinate(s) in the cloud");
  }
  // the host's cast of the ceil is defined only inside int
  for (int d = 0; d < 3; ++d)
    if (!(std::fabs(std::ceil((geo.bmax_[d] - geo.bmin_[d]) / resolution)) < 2147483647.0))
      return fail(ctx, SVSDF_ERR_INVALID, std::string(what) + ": the grid has more than 2^31 - 1 cells along an axis");
  geo.set_resolution(resolution);
  for (int d = 0; d < 3; ++d) { rm.dims[d] = geo.size_[d]; rm.bmin[d] = geo.bmin_[d]; rm.bmax[d] = geo.bmax_[d]; }
  {
    const double cx = std::max(0, rm.dims[0]), cy = std::max(0, rm.dims[1]), cz = std::max(0, rm.dims[2]);
    if (cx * cy * cz > 2147483647.0)
      return fail(ctx, SVSDF_ERR_INVALID, std::string(what) + ": X * Y * Z exceeds 2^31 - 1 (the unified voxel id is an int)");
  }
  rm.cells = geo.cells();
  if (rm.cells && n) {
    Buf<unsigned> d_cnt, d_partocc;
    const unsigned g_cells = map_grid(rm.cells);
    int rc = d_cnt.alloc(ctx, rm.cells);
    if (rc == SVSDF_OK) rc = rm.d_occ.alloc(ctx, rm.cells);
    if (rc == SVSDF_OK) rc = d_partocc.alloc(ctx, g_cells);
    if (rc) return rc;
    HIPCHK_AS(what, hipMemsetAsync(d_cnt, 0, rm.cells * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_map_count, dim3(map_grid(n)), dim3(kMapBlock), 0, st, d_cloud, n, map_geom_dev(rm), d_cnt.get(), rm.cells);
    HIPCHK_AS(what, hipGetLastError());
    hipLaunchKernelGGL(k_map_threshold, dim3(g_cells), dim3(kMapBlock), 0, st, d_cnt.get(), rm.cells, (long long)sta_threshold,
                       rm.d_occ.get(), d_partocc.get());
    HIPCHK_AS(what, hipGetLastError());
    std::vector<unsigned> ho(g_cells);
    HIPCHK_AS(what, hipMemcpyAsync(ho.data(), d_partocc, ho.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK_AS(what, hipStreamSynchronize(st));
    for (unsigned b = 0; b < g_cells; ++b) rm.occupied += ho[b];
  }
  rm.set = true;
  ctx->rmap = std::move(rm);
  return SVSDF_OK;
}

// The resident map's layer 0 into the front-end bitmap `d_out` (rows x row_words words), queued on the context's stream
inline int map_front_bitmap(svsdf_ctx *ctx, const char *what, int side, int row_words, size_t rows, unsigned long long *d_out) {
  using namespace svsdf;
  const ResidentMap &rm = ctx->rmap;
  const size_t words = rows * (size_t)row_words;
  if ((words + kMapBlock - 1) / kMapBlock > 0x7fffffffull) return fail(ctx, SVSDF_ERR_INVALID, std::string(what) + ": map too large");
  hipLaunchKernelGGL(k_map_front_bitmap, dim3((unsigned)((words + kMapBlock - 1) / kMapBlock)), dim3(kMapBlock), 0, ctx->stream,
                     rm.d_occ.get(), rm.dims[0], rm.dims[1], rm.dims[2], side, row_words, words, d_out);
  HIPCHK_AS(what, hipGetLastError());
  return SVSDF_OK;
}

// The gather of svsdf_set_points_from_map on the map's context: the marked voxels' centres into rmap.d_pts, count in rmap.gathered
inline int map_gather(svsdf_ctx *ctx, const double *centres, size_t ncentres, const double halfbd[3]) {
  using namespace svsdf;
  const char *what = "svsdf_set_points_from_map";
  ResidentMap &rm = ctx->rmap;
  hipStream_t st = ctx->stream;
  rm.gathered = 0;
  rm.d_pts.reset();
  if (ncentres == 0 || rm.cells == 0 || rm.occupied == 0) return SVSDF_OK;
  std::vector<int> boxes;
  map_geometry(rm).centre_boxes(centres, ncentres, halfbd, boxes);
  const size_t X = (size_t)rm.dims[0], Y = (size_t)rm.dims[1];
  // the ids the boxes span: the id grows with each index, so a box's smallest is its c1 corner's and its largest its c2 corner's
  size_t lo = ~(size_t)0, hi = 0, max_cells = 0;
  for (size_t c = 0; c < ncentres; ++c) {
    const int *b = boxes.data() + 12 * c;
    bool inside = true;
    for (int d = 0; d < 3; ++d) inside = inside && b[d] >= 0 && b[3 + d] >= b[d] && b[3 + d] < rm.dims[d];
    if (!inside) continue;
    lo = std::min(lo, ((size_t)b[2] * Y + (size_t)b[1]) * X + (size_t)b[0]);
    hi = std::max(hi, ((size_t)b[5] * Y + (size_t)b[4]) * X + (size_t)b[3]);
    max_cells = std::max(max_cells, (size_t)(b[3] - b[0] + 1) * (size_t)(b[4] - b[1] + 1) * (size_t)(b[5] - b[2] + 1));
  }
  if (max_cells == 0) return SVSDF_OK;
  const size_t word0 = lo >> 5, nwords = (hi >> 5) - word0 + 1;
  const size_t nblocks = (nwords + kMapBlock - 1) / kMapBlock;   // <= 2^31 / 32 / 256
  Buf<int> d_boxes;
  Buf<unsigned> d_bits, d_bcount, d_boff, d_total;
  int rc = d_boxes.alloc(ctx, boxes.size());
  if (rc == SVSDF_OK) rc = d_bits.alloc(ctx, nwords);
  if (rc == SVSDF_OK) rc = d_bcount.alloc(ctx, nblocks);
  if (rc == SVSDF_OK) rc = d_boff.alloc(ctx, nblocks);
  if (rc == SVSDF_OK) rc = d_total.alloc(ctx, 1);
  if (rc) return rc;
  // (`boxes` is pageable: it outlives the copy because every path below ends in a stream synchronisation or in the owners'
  // frees, which wait for the device)
  HIPCHK_AS(what, hipMemcpyAsync(d_boxes, boxes.data(), boxes.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK_AS(what, hipMemsetAsync(d_bits, 0, nwords * sizeof(unsigned), st));
  const dim3 gmark(map_grid(max_cells), (unsigned)std::min<size_t>(ncentres, 65535));
  hipLaunchKernelGGL(k_map_mark, gmark, dim3(kMapBlock), 0, st, d_boxes.get(), ncentres, rm.d_occ.get(), rm.dims[0], rm.dims[1],
                     rm.dims[2], word0, nwords, d_bits.get());
  HIPCHK_AS(what, hipGetLastError());
  hipLaunchKernelGGL(k_map_block_counts, dim3((unsigned)nblocks), dim3(kMapBlock), 0, st, d_bits.get(), nwords, d_bcount.get());
  HIPCHK_AS(what, hipGetLastError());
  hipLaunchKernelGGL(k_map_scan_blocks, dim3(1), dim3(kMapBlock), 0, st, d_bcount.get(), nblocks, d_boff.get(), d_total.get());
  HIPCHK_AS(what, hipGetLastError());
  unsigned total = 0;
  HIPCHK_AS(what, hipMemcpyAsync(&total, d_total, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK_AS(what, hipStreamSynchronize(st));
  if (total == 0) return SVSDF_OK;
  if ((rc = rm.d_pts.alloc(ctx, 3 * (size_t)total))) return rc;
  hipLaunchKernelGGL(k_map_scatter, dim3((unsigned)nblocks), dim3(kMapBlock), 0, st, d_bits.get(), nwords, word0, d_boff.get(),
                     map_geom_dev(rm), rm.d_pts.get(), (size_t)total);
  HIPCHK_AS(what, hipGetLastError());
  HIPCHK_AS(what, hipStreamSynchronize(st));
  rm.gathered = total;
  return SVSDF_OK;
}

}  // namespace svsdf_impl
