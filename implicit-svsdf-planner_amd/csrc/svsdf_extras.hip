// svsdf_extras.hip -- C ABI of the rows around the hot path: batched front-end collision check and
// shape byte kernels (SWM:1171-1211, SHP:386-430), query-point producer (PCSmap_manager.cpp:88-210) on the host and on the
// device (svsdf_mapdev.hpp), mesh outline, the
// swept volume's outline and its extrusion (SWM:321-336), the in-repo L-BFGS driver (lbfgs.hpp:290-438).
// The device entries open with on_device (svsdf_ctx.hpp); their packed buffers are laid out in svsdf_layout.hpp.
#include "svsdf_ctx.hpp"
#include "svsdf_lbfgs.hpp"
#include "svsdf_mesh.hpp"
#include "svsdf_contour.hpp"
#include "svsdf_points.hpp"
#include "svsdf_mapdev.hpp"

using namespace svsdf;
using namespace svsdf_impl;
namespace lay = svsdf_layout;

// yaw table of the byte kernels: for (yaw = -PI; yaw < PI; yaw += yaw_res) (SHP:400-401); PI macro of SHP:31
static std::vector<double> shape_kernel_yaws(int kernel_count, int *loop_count) {
  const double PI_ = 3.14159265358979323846;
  const double yaw_res = 2 * PI_ / kernel_count;
  std::vector<double> yaws;
  int ind = 0;
  for (double yaw = -PI_; yaw < PI_; yaw += yaw_res, ind++)
    if (ind < kernel_count) yaws.push_back(yaw);
  if (loop_count) *loop_count = ind;
  return yaws;
}

// A Polygon context has yaw kernels -- and with them the resident map, successors and search -- only when it was created
// with SVSDF_FLAG_POLYGON_YAW_KERNELS (svsdf_c.h: the reference's stated intent, shape_sdf_rot<kPolygon>)
static bool polygon_refused(const svsdf_ctx *ctx) {
  return ctx->cfg.shape_id == SVSDF_SHAPE_Polygon && !(ctx->cfg.flags & SVSDF_FLAG_POLYGON_YAW_KERNELS);
}

// The byte kernels of `yaws` (BasicShape::initShape's loop, SHP:400-428) into the caller's d_map, kernel_size^2 bytes per yaw:
// the yaw table's upload, then k_shape_kernels.  `what` names the caller in a HIP error.  `uncompiled`: the caller's error for a
// shape that is not compiled into the library, null to go on without one.  `then_upload` (optional) queues the caller's own
// uploads between the table's and the launch.
static int build_yaw_kernels(svsdf_ctx *ctx, const char *what, const char *uncompiled, const std::vector<double> &yaws,
                             int kernel_size, double resolution, int side, double safemargin, double *d_yaw,
                             unsigned char *d_map, const std::function<int()> &then_upload = nullptr) {
  const int count = (int)yaws.size();
  hipStream_t st = ctx->stream;
  HIPCHK_AS(what, hipMemcpyAsync(d_yaw, yaws.data(), count * sizeof(double), hipMemcpyHostToDevice, st));
  if (then_upload) {
    int rc = then_upload();
    if (rc) return rc;
  }
  const unsigned grid = (unsigned)(((size_t)kernel_size * kernel_size * count + kBlock - 1) / kBlock);
  if (!launch_k_shape_kernels(ctx->cfg.shape_id, grid, st, ctx->sp, kernel_size, count, resolution, side, safemargin, d_yaw, d_map) &&
      uncompiled)
    return fail(ctx, SVSDF_ERR_INVALID, uncompiled);
  HIPCHK_AS(what, hipGetLastError());
  return SVSDF_OK;
}

// kt = 0, 0.02, ... by accumulated adds while kt <= 1.0 (SWM:1189)
static int subsw_kt_table(double kt_tab[kMaxKt]) {
  int nkt = 0;
  for (double kt = 0.0; kt <= 1.0 && nkt < kMaxKt; kt += 0.02) kt_tab[nkt++] = kt;
  return nkt;
}

// One output of a "size query, then fill" entry: `v`, reported in units of `per` elements, copied to `out` if `capacity` units hold it
template <typename T> struct Out { const std::vector<T> &v; size_t per; T *out; size_t capacity; size_t *count; };
// Reports every count.  With every output pointer given, copies them all -- or none, and returns false, when one capacity is too small.
template <typename... T> static bool deliver(const Out<T> &...o) {
  ((*o.count = o.v.size() / o.per), ...);
  if (!(... && (o.out != nullptr))) return true;   // the size query
  if (!(... && (o.capacity >= *o.count))) return false;
  (std::copy(o.v.begin(), o.v.end(), o.out), ...);
  return true;
}

// The grid a front-end map is made from: the host map's (svsdf_frontend_set_map) or the resident one's (svsdf_frontend_set_map_device)
struct FrontGrid { int X, Y, Z; double res; const double *bmin, *bmax; };

// What the two set-map entries share: the argument checks (`what` names the entry in every message), then the yaw kernels,
// their row words, the yaw-free table and the FrontMapDev fill.  `fill_occ(d_occ, side, row_words, rows)` queues the inflated
// layer-0 bitmap into d_occ on the context's stream, between the yaw table's upload and the kernels' launch.
static int frontend_install(svsdf_ctx *ctx, const std::string &what, const FrontGrid &g, int kernel_size, int kernel_count,
                            double safemargin, const std::function<int(unsigned long long *, int, int, size_t)> &fill_occ) {
  if (polygon_refused(ctx))
    return fail(ctx, SVSDF_ERR_INVALID,
                what + ": Polygon has no getonlySDF(pos_rel, Matrix3d) in the reference (Shape.hpp:1477), so no yaw kernels");
  if (kernel_size <= 0 || kernel_size % 2 == 0)
    return fail(ctx, SVSDF_ERR_INVALID, what + ": kernel_size must be odd and positive");
  if (kernel_size > kMaxKernelSize || kernel_count > kMaxKernelCount || kernel_count < 1)
    return fail(ctx, SVSDF_ERR_INVALID,
                what + ": kernel_size <= 63 and 1 <= kernel_count <= 64 (a kernel row and a cell's mask are one word each)");
  if (!std::isfinite(safemargin)) return fail(ctx, SVSDF_ERR_INVALID, what + ": safemargin not finite");
  const int X = g.X, Y = g.Y, Z = g.Z;
  const int side = (kernel_size - 1) / 2;
  if (X < 1 || Y < 1 || Z < 1) return fail(ctx, SVSDF_ERR_INVALID, what + ": empty map");
  if ((Y + kYawFreeBlock - 1) / kYawFreeBlock > 65535 || (long long)X * Y > 0x7fffffffll)
    return fail(ctx, SVSDF_ERR_INVALID, what + ": map too large");
  int loops = 0;
  const std::vector<double> yaws = shape_kernel_yaws(kernel_count, &loops);
  if ((int)yaws.size() != kernel_count)
    return fail(ctx, SVSDF_ERR_INVALID, what + ": the reference's yaw loop yields fewer kernels than kernel_count");
  const int row_words = (Y + 2 * side + 63) / 64 + 1;
  const size_t rows = (size_t)X + 2 * (size_t)side;
  double kt_tab[kMaxKt];
  const int nkt = subsw_kt_table(kt_tab);

  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  FrontMap &fm = ctx->fmap;
  fm = FrontMap{};   // the old map goes, and its search state with it
  Buf<double> d_yaw;
  Buf<unsigned char> d_bytes;
  Buf<unsigned long long> d_krows;
  hipStream_t st = ctx->stream;
  const std::string uncompiled = what + ": shape not compiled into this library";
  const auto build = [&]() -> int {
    int rc = d_yaw.alloc(ctx, kernel_count);
    if (rc == SVSDF_OK) rc = d_bytes.alloc(ctx, (size_t)kernel_size * kernel_size * kernel_count);
    if (rc == SVSDF_OK) rc = d_krows.alloc(ctx, (size_t)kernel_size * kernel_count);
    if (rc == SVSDF_OK) rc = fm.d_occ.alloc(ctx, rows * row_words);
    if (rc == SVSDF_OK) rc = fm.d_free.alloc(ctx, (size_t)X * Y);
    if (rc == SVSDF_OK) rc = fm.d_kt.alloc(ctx, kMaxKt);
    if (rc) return rc;
    // the kernel resolution is the map's: kernelConv overlays kernel cells on map cells one to one
    rc = build_yaw_kernels(ctx, what.c_str(), uncompiled.c_str(), yaws, kernel_size, g.res, side, safemargin, d_yaw, d_bytes, [&]() -> int {
      const int rf = fill_occ(fm.d_occ, side, row_words, rows);
      if (rf) return rf;
      HIPCHK_AS(what, hipMemcpyAsync(fm.d_kt, kt_tab, kMaxKt * sizeof(double), hipMemcpyHostToDevice, st));
      return SVSDF_OK;
    });
    if (rc) return rc;
    launch_k_pack_kernel_rows(st, d_bytes, kernel_size, kernel_count, d_krows);
    HIPCHK_AS(what, hipGetLastError());
    launch_k_yaw_free(st, fm.d_occ, row_words, d_krows, kernel_size, kernel_count, X, Y, fm.d_free);
    HIPCHK_AS(what, hipGetLastError());
    return SVSDF_OK;
  };
  int rc = build();
  // on every path: the pageable sources above and the scratch must outlive what the stream still does with them
  const hipError_t es = hipStreamSynchronize(st);
  if (rc == SVSDF_OK && es != hipSuccess)
    rc = fail(ctx, SVSDF_ERR_HIP_BASE + (int)es, what + ": " + hipGetErrorString(es));
  if (rc) { fm = FrontMap{}; return rc; }
  FrontMapDev &dev = fm.dev;
  dev.occ = fm.d_occ; dev.free_ = fm.d_free; dev.kt = fm.d_kt; dev.nkt = nkt;
  dev.X = X; dev.Y = Y; dev.side = side; dev.row_words = row_words; dev.kernel_count = kernel_count;
  dev.res = g.res;
  dev.half = (double)(kernel_size / 2 + 1);   // front_end_Astar.hpp:224: integer division, metres
  for (int d = 0; d < 3; ++d) { dev.bmin[d] = g.bmin[d]; dev.bmax[d] = g.bmax[d]; }
  fm.Z = Z;
  fm.set = true;
  return SVSDF_OK;
}

extern "C" {

// ---- front end -----------------------------------------------------------------
int svsdf_check_sub_sw_collision(svsdf_ctx *group, size_t n_edges, const double *father_states,
                                 const double *child_states, const size_t *pts_offset, const double *pts_xy,
                                 unsigned char *free_out) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    if (n_edges == 0) return SVSDF_OK;
    if (!father_states || !child_states || !pts_offset || !free_out)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_check_sub_sw_collision: null argument");
    const size_t total = pts_offset[n_edges];
    if (pts_offset[0] != 0 || (total && !pts_xy))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_check_sub_sw_collision: bad offsets");
    size_t max_pts = 0;
    for (size_t e = 0; e < n_edges; ++e) {
      if (pts_offset[e + 1] < pts_offset[e]) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_check_sub_sw_collision: offsets not monotone");
      max_pts = std::max(max_pts, pts_offset[e + 1] - pts_offset[e]);
    }
    if (n_edges > 0x7fffffffu || (max_pts + kSubswPoints - 1) / kSubswPoints > 65535u)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_check_sub_sw_collision: batch too large");
    double kt_tab[kMaxKt];
    const int nkt = subsw_kt_table(kt_tab);
    if (total == 0) { std::memset(free_out, 1, n_edges); return SVSDF_OK; }
    HIPCHK(hipSetDevice(ctx->device));
    // one packed upload through a pinned staging buffer
    const lay::SubswLayout L = lay::subsw_layout(n_edges, total, kMaxKt);
    const size_t need = L.bytes / sizeof(double);
    FrontStaging &fs = ctx->fstage;
    if (need > fs.edges.cap) {
      int rc = fs.edges.reserve(ctx, need + need / 2);
      if (rc) return rc;
    }
    if (n_edges > fs.flag_cap) {
      int rc = fs.d_flag.alloc(ctx, 2 * n_edges);
      if (rc) return rc;
      fs.flag_cap = 2 * n_edges;
      fs.h_flag.resize(2 * n_edges);
    }
    double *h = fs.edges.h, *d = fs.edges.d;
    std::memcpy(lay::at<double>(h, L.father), father_states, 3 * n_edges * sizeof(double));
    std::memcpy(lay::at<double>(h, L.child), child_states, 3 * n_edges * sizeof(double));
    std::memcpy(lay::at<double>(h, L.kt), kt_tab, kMaxKt * sizeof(double));
    unsigned long long *h_offs = lay::at<unsigned long long>(h, L.offs);
    for (size_t e = 0; e <= n_edges; ++e) h_offs[e] = pts_offset[e];
    std::memcpy(lay::at<double>(h, L.pts), pts_xy, 2 * total * sizeof(double));
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(d, h, L.bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(fs.d_flag, 0, n_edges * sizeof(int), st));   // hit flags: 1 = some sdf < 0
    const dim3 grid((unsigned)n_edges, (unsigned)((max_pts + kSubswPoints - 1) / kSubswPoints));
    (void)launch_k_subsw(ctx->cfg.shape_id, grid, st, ctx->sp, lay::at<double>(d, L.father), lay::at<double>(d, L.child),
                         lay::at<unsigned long long>(d, L.offs), lay::at<double>(d, L.pts), lay::at<double>(d, L.kt), nkt, fs.d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fs.h_flag.data(), fs.d_flag, n_edges * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int *hit = fs.h_flag.data();
    unsigned char *out = free_out;   // (locals: byte stores through the captured pointer would reload it every time)
    for (size_t e = 0; e < n_edges; ++e) out[e] = hit[e] ? 0 : 1;
    return SVSDF_OK;
  });
}

int svsdf_shape_kernels(svsdf_ctx *group, int kernel_size, int kernel_count, double kernel_resolution,
                        double safemargin, unsigned char *map_out, unsigned char *bytes_out, double *yaw_out,
                        int *loop_count) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    if (kernel_size <= 0 || kernel_count <= 0 || kernel_size > 4096 || kernel_count > 65536 || !map_out)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_shape_kernels: bad argument");
    if (polygon_refused(ctx))
      return fail(ctx, SVSDF_ERR_INVALID,
                  "svsdf_shape_kernels: Polygon has no getonlySDF(pos_rel, Matrix3d) in the reference (Shape.hpp:1477)");
    int ind = 0;
    const std::vector<double> yaws = shape_kernel_yaws(kernel_count, &ind);
    if (loop_count) *loop_count = ind;
    const int count = (int)yaws.size();
    const int size_side = (int)(0.5 * (kernel_size - 1));
    const size_t cells = (size_t)kernel_size * kernel_size;
    HIPCHK(hipSetDevice(ctx->device));
    // (an early return below frees the scratch, and the owner's free waits for the device: nothing queued on the stream still reads
    // yaws -- declared before d_yaw, so destroyed after it -- or writes map_out once this function has returned)
    Buf<double> d_yaw;
    Buf<unsigned char> d_map;
    int rc = d_yaw.alloc(ctx, count);
    if (rc == SVSDF_OK) rc = d_map.alloc(ctx, cells * count);
    if (rc == SVSDF_OK)
      rc = build_yaw_kernels(ctx, "svsdf_shape_kernels", nullptr, yaws, kernel_size, kernel_resolution, size_side, safemargin, d_yaw, d_map);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK_AS("svsdf_shape_kernels", hipMemcpyAsync(map_out, d_map, cells * count, hipMemcpyDeviceToHost, st));
    HIPCHK_AS("svsdf_shape_kernels", hipStreamSynchronize(st));
    if (yaw_out) std::memcpy(yaw_out, yaws.data(), count * sizeof(double));
    if (bytes_out) {  // byteShapeKernel::generateByteKernel SHP:194-216, or_mask SHP:95
      const int bpl = (kernel_size + 7) / 8;
      std::memset(bytes_out, 0, (size_t)count * kernel_size * bpl);
      for (int k = 0; k < count; ++k)
        for (int a = 0; a < kernel_size; ++a)
          for (int b = 0; b < kernel_size; ++b)
            if (map_out[(size_t)k * cells + (size_t)a * kernel_size + b])
              bytes_out[((size_t)k * kernel_size + a) * bpl + b / 8] |= (unsigned char)(0x80u >> (b % 8));
    }
    return SVSDF_OK;
  });
}

// ---- query-point producer (host) -----------------------------------------------------------------
struct svsdf_map {
  svsdf_host::OccupancyMap m;
};

svsdf_map *svsdf_map_create(const float *xyz, size_t n, double resolution, int sta_threshold) {
  if ((!xyz && n) || !(resolution > 0.0)) return nullptr;
  svsdf_map *mp = new svsdf_map();
  mp->m.build(xyz, n, resolution, sta_threshold);
  return mp;
}
void svsdf_map_destroy(svsdf_map *map) { delete map; }
int svsdf_map_info(const svsdf_map *map, int dims[3], double bmin[3], double bmax[3], size_t *occupied) {
  if (!map) return SVSDF_ERR_INVALID;
  for (int d = 0; d < 3; ++d) {
    if (dims) dims[d] = map->m.dims()[d];
    if (bmin) bmin[d] = map->m.bmin()[d];
    if (bmax) bmax[d] = map->m.bmax()[d];
  }
  if (occupied) *occupied = map->m.occupied_count();
  return SVSDF_OK;
}
int svsdf_map_gather(const svsdf_map *map, const double *centres_xyz, size_t ncentres, const double halfbd[3],
                     double *out_xyz, size_t capacity, size_t *count) {
  if (!map || (!centres_xyz && ncentres) || !halfbd || !count) return SVSDF_ERR_INVALID;
  std::vector<double> pts;
  map->m.gather(centres_xyz, ncentres, halfbd, pts);
  return deliver(Out<double>{pts, 3, out_xyz, capacity, count}) ? SVSDF_OK : SVSDF_ERR_INVALID;
}
int svsdf_pcd_read_ascii(const char *path, float *xyz, size_t capacity, size_t *n) {
  if (!path || !n) return SVSDF_ERR_INVALID;
  std::vector<float> v;
  if (!svsdf_host::read_pcd_ascii(path, v)) return SVSDF_ERR_INVALID;
  return deliver(Out<float>{v, 3, xyz, capacity, n}) ? SVSDF_OK : SVSDF_ERR_INVALID;
}

// ---- front end: resident map, yaw-free table, batched successor test ---------------------------------------------
int svsdf_frontend_set_map(svsdf_ctx *group, const svsdf_map *map, int kernel_size, int kernel_count, double safemargin) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    if (!map) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_frontend_set_map: null map");
    const svsdf_host::OccupancyMap &m = map->m;
    const FrontGrid g{m.dims()[0], m.dims()[1], m.dims()[2], m.resolution(), m.bmin(), m.bmax()};
    // generateMapKernel2D (PCSmap_manager.h:81-108) in 64-bit row words: layer iz = 0, cell (x, y) at (x + side, y + side)
    std::vector<unsigned long long> occ;   // pageable: frontend_install synchronises the stream on every path after the upload
    return frontend_install(ctx, "svsdf_frontend_set_map", g, kernel_size, kernel_count, safemargin,
                            [&](unsigned long long *d_occ, int side, int row_words, size_t rows) -> int {
      occ.assign(rows * row_words, 0ull);
      for (int x = 0; x < g.X; ++x)
        for (int y = 0; y < g.Y; ++y)
          if (m.cell(x, y, 0)) occ[(size_t)(x + side) * row_words + ((y + side) >> 6)] |= 1ull << ((y + side) & 63);
      HIPCHK_AS("svsdf_frontend_set_map", hipMemcpyAsync(d_occ, occ.data(), occ.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
      return SVSDF_OK;
    });
  });
}

// ---- the producer on the device (svsdf_mapdev.hpp): cloud -> resident map -> front-end bitmap / gathered query points ------
int svsdf_map_build_device(svsdf_ctx *group, const float *xyz, size_t n, int xyz_on_device, double resolution, int sta_threshold) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    if (!xyz && n) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_build_device: null cloud");
    if (!(resolution > 0.0) || !std::isfinite(resolution))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_build_device: resolution must be positive and finite");
    if (n > 0xffffffffull) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_build_device: too many points (n >= 2^32)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const auto t0 = std::chrono::steady_clock::now();
    ctx->rmap = ResidentMap{};   // the earlier map goes whatever becomes of this call
    Buf<float> d_stage;
    const float *d_cloud = xyz;
    if (n && !xyz_on_device) {
      int rc = d_stage.alloc(ctx, 3 * n);
      if (rc) return rc;
      HIPCHK_AS("svsdf_map_build_device", hipMemcpyAsync(d_stage, xyz, 3 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
      d_cloud = d_stage;
    }
    int rc = map_build(ctx, d_cloud, n, resolution, sta_threshold);
    // on every path: the caller's (pageable) cloud and the staging must outlive what the stream still does with them
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc == SVSDF_OK && es != hipSuccess)
      rc = fail(ctx, SVSDF_ERR_HIP_BASE + (int)es, std::string("svsdf_map_build_device: ") + hipGetErrorString(es));
    if (rc) { ctx->rmap = ResidentMap{}; return rc; }
    ctx->rmap.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SVSDF_OK;
  });
}

int svsdf_map_device_get_info(const svsdf_ctx *group, svsdf_map_device_info *out) {
  return on_device(const_cast<svsdf_ctx *>(group), __func__, [&](svsdf_ctx *ctx) -> int {
    if (!out) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_get_info: null argument");
    if (out->struct_size != (int)sizeof(svsdf_map_device_info))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_get_info: out->struct_size is not sizeof(svsdf_map_device_info)");
    const ResidentMap &rm = ctx->rmap;
    if (!rm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_get_info: no resident map (svsdf_map_build_device)");
    for (int d = 0; d < 3; ++d) { out->dims[d] = rm.dims[d]; out->bmin[d] = rm.bmin[d]; out->bmax[d] = rm.bmax[d]; }
    out->resolution = rm.res; out->sta_threshold = rm.sta_threshold;
    out->n_cloud = rm.n_cloud; out->occupied = rm.occupied; out->gathered = rm.gathered;
    out->build_ms = rm.build_ms; out->gather_ms = rm.gather_ms;
    return SVSDF_OK;
  });
}

int svsdf_map_device_cells(const svsdf_ctx *group, unsigned char *occ_out, size_t capacity) {
  return on_device(const_cast<svsdf_ctx *>(group), __func__, [&](svsdf_ctx *ctx) -> int {
    const ResidentMap &rm = ctx->rmap;
    if (!rm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_cells: no resident map (svsdf_map_build_device)");
    if (rm.cells == 0) return SVSDF_OK;
    if (!occ_out || capacity < rm.cells)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_cells: capacity too small (X * Y * Z bytes, svsdf_map_device_get_info)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(occ_out, rm.d_occ, rm.cells, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SVSDF_OK;
  });
}

int svsdf_frontend_set_map_device(svsdf_ctx *group, int kernel_size, int kernel_count, double safemargin) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    const ResidentMap &rm = ctx->rmap;
    if (!rm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_frontend_set_map_device: no resident map (svsdf_map_build_device)");
    const FrontGrid g{rm.dims[0], rm.dims[1], rm.dims[2], rm.res, rm.bmin, rm.bmax};
    return frontend_install(ctx, "svsdf_frontend_set_map_device", g, kernel_size, kernel_count, safemargin,
                            [&](unsigned long long *d_occ, int side, int row_words, size_t rows) -> int {
      return map_front_bitmap(ctx, "svsdf_frontend_set_map_device", side, row_words, rows, d_occ);
    });
  });
}

int svsdf_set_points_from_map(svsdf_ctx *ctx, const double *centres_xyz, size_t ncentres, const double halfbd[3], size_t *count) {
  if (!ctx || ctx->host_only) return fail(ctx, SVSDF_ERR_NO_DEVICE, "svsdf_set_points_from_map: no device context");
  if ((!centres_xyz && ncentres) || !halfbd) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_set_points_from_map: null argument");
  for (size_t e = 0; e < 3 * ncentres; ++e)
    if (!std::isfinite(centres_xyz[e])) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_set_points_from_map: non-finite centre");
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(halfbd[d])) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_set_points_from_map: non-finite half extent");
  svsdf_ctx *leaf = leaf_of(ctx);   // the map lives on the first device
  ResidentMap &rm = leaf->rmap;
  if (!rm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_set_points_from_map: no resident map (svsdf_map_build_device)");
  const auto t0 = std::chrono::steady_clock::now();
  int rc = SVSDF_OK;
  if (hipSetDevice(leaf->device) != hipSuccess || hipStreamSynchronize(leaf->stream) != hipSuccess)
    rc = fail(leaf, SVSDF_ERR_HIP_BASE, "svsdf_set_points_from_map: the map's device is not usable");
  if (rc == SVSDF_OK) rc = map_gather(leaf, centres_xyz, ncentres, halfbd);
  if (rc) {
    (void)hipStreamSynchronize(leaf->stream);
    rm.gathered = 0;
    rm.d_pts.reset();
    if (leaf != ctx) ctx->err = leaf->err;
    return rc;
  }
  rm.gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // the hand-over: the compacted array is the planner's input as it stands (svsdf_set_points_device's path)
  const size_t P = rm.gathered;
  rc = ctx->subs.empty() ? upload_shard_device(ctx, rm.d_pts, P, ctx->cfg.rank, ctx->cfg.world_size)
                         : upload_group_device(ctx, rm.d_pts, P);
  ctx->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (svsdf_ctx *s : ctx->subs) s->setup_ms = ctx->setup_ms;
  if (count) *count = P;
  return rc;
}

int svsdf_map_device_points(const svsdf_ctx *group, double *out_xyz, size_t capacity, size_t *count) {
  return on_device(const_cast<svsdf_ctx *>(group), __func__, [&](svsdf_ctx *ctx) -> int {
    const ResidentMap &rm = ctx->rmap;
    if (!rm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_points: no resident map (svsdf_map_build_device)");
    if (!count) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_points: null count");
    *count = rm.gathered;
    if (!out_xyz || rm.gathered == 0) return SVSDF_OK;   // the size query
    if (capacity < rm.gathered)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_map_device_points: capacity too small (query with out_xyz = NULL first)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out_xyz, rm.d_pts, 3 * rm.gathered * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SVSDF_OK;
  });
}

// plan_manager.cpp:132-140 and the loop header of :157; pure host
int svsdf_path_waypoints(size_t path_len, double grid_resolution, double traj_parlength, size_t *idx_out, size_t capacity,
                         size_t *count, int *index_gap) {
  std::vector<size_t> idx;
  int gap = 0;
  if (!count || !svsdf_host::path_waypoints(path_len, grid_resolution, traj_parlength, idx, &gap)) return SVSDF_ERR_INVALID;
  if (index_gap) *index_gap = gap;
  return deliver(Out<size_t>{idx, 1, idx_out, capacity, count}) ? SVSDF_OK : SVSDF_ERR_INVALID;
}

int svsdf_frontend_yaw_free(const svsdf_ctx *group, unsigned long long *mask_out, size_t capacity, int dims2[2]) {
  // (const: the error string is the only thing written)
  return on_device(const_cast<svsdf_ctx *>(group), __func__, [&](svsdf_ctx *ctx) -> int {
    const FrontMap &fm = ctx->fmap;
    if (!fm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_frontend_yaw_free: no map (svsdf_frontend_set_map)");
    if (dims2) { dims2[0] = fm.dev.X; dims2[1] = fm.dev.Y; }
    if (!mask_out) return SVSDF_OK;
    const size_t n = (size_t)fm.dev.X * fm.dev.Y;
    if (capacity < n) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_frontend_yaw_free: capacity too small (query with mask_out = NULL first)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(mask_out, fm.d_free, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SVSDF_OK;
  });
}

int svsdf_kernel_bfs(unsigned long long free_mask, int kernel_count, double father_yaw, double *child_yaw, int *kernel_index) {
  if (!child_yaw || !kernel_index) return -3;
  return kernel_bfs(free_mask, kernel_count, father_yaw, child_yaw, kernel_index);
}

int svsdf_astar_successors(svsdf_ctx *group, size_t n, const int *parent_ij, const double *parent_yaw, unsigned char *ok_out,
                           double *child_yaw_out, unsigned char *stage_out) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    if (!ctx->fmap.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_successors: no map (svsdf_frontend_set_map)");
    if (n == 0) return SVSDF_OK;
    if (!parent_ij || !parent_yaw || !ok_out || !child_yaw_out)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_successors: null argument");
    const FrontMapDev &fm = ctx->fmap.dev;
    for (size_t p = 0; p < n; ++p) {
      const int i = parent_ij[2 * p], j = parent_ij[2 * p + 1];
      if (i < 0 || i >= fm.X || j < 0 || j >= fm.Y)
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_successors: parent " + std::to_string(p) + " is outside the map");
      double cy;
      int ki;
      if (kernel_bfs(0ull, fm.kernel_count, parent_yaw[p], &cy, &ki) < 0)
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_successors: yaw of parent " + std::to_string(p) +
                                                " maps to a kernel index outside [0, kernel_count)");
    }
    HIPCHK(hipSetDevice(ctx->device));
    constexpr size_t kSuccParents = (size_t)1 << 18;       // parents per launch: 9 blocks each, well inside one grid dimension
    Staged<unsigned char> &succ = ctx->fstage.succ;
    const size_t want = std::min(n, kSuccParents);
    if (lay::succ_layout(want).bytes > succ.cap) {
      int rc = succ.reserve(ctx, lay::succ_layout(std::min(kSuccParents, want + want / 2)).bytes);
      if (rc) return rc;
    }
    hipStream_t st = ctx->stream;
    for (size_t p0 = 0; p0 < n; p0 += kSuccParents) {
      const size_t m = std::min(kSuccParents, n - p0);
      const lay::SuccLayout L = lay::succ_layout(m);   // one upload [yaw | ij], one read-back [child yaw | stage]
      unsigned char *h = succ.h, *d = succ.d;
      std::memcpy(h + L.yaw, parent_yaw + p0, m * sizeof(double));
      std::memcpy(h + L.ij, parent_ij + 2 * p0, 2 * m * sizeof(int));
      HIPCHK(hipMemcpyAsync(d, h, L.in_bytes(), hipMemcpyHostToDevice, st));
      if (!launch_k_succ(ctx->cfg.shape_id, (unsigned)(9 * m), st, ctx->sp, fm, lay::at<const int>(d, L.ij),
                         lay::at<const double>(d, L.yaw), lay::at<double>(d, L.child_yaw), d + L.stage))
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_successors: shape not compiled into this library");
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(h + L.child_yaw, d + L.child_yaw, L.out_bytes(), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::memcpy(child_yaw_out + 9 * p0, h + L.child_yaw, 9 * m * sizeof(double));
      const unsigned char *hs = h + L.stage;
      unsigned char *ok = ok_out + 9 * p0;   // (a local: byte stores through the captured pointer would reload it every time)
      for (size_t e = 0; e < 9 * m; ++e) ok[e] = hs[e] == 0 ? 1 : 0;
      if (stage_out) std::memcpy(stage_out + 9 * p0, hs, 9 * m);
    }
    return SVSDF_OK;
  });
}

// ---- A* search on the resident map ----------------------------------------------------------------------------------
void svsdf_astar_params_default(svsdf_astar_params *p) {
  if (!p) return;
  *p = svsdf_astar_params{};
  p->struct_size = (int)sizeof(svsdf_astar_params);
  p->start_yaw = 0.0;   // front_end_Astar.hpp:281
}

// the search's device blob for the resident map, at the first search on it (svsdf_layout::astar_layout), and the pinned state
static int astar_alloc(svsdf_ctx *ctx) {
  FrontMap &fm = ctx->fmap;
  if (fm.d_astar) return SVSDF_OK;
  const lay::AstarLayout L = lay::astar_layout((size_t)fm.dev.X * fm.dev.Y);
  if (L.open_cap > 0x7fffffffull) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: map too large");
  int rc = fm.d_astar.alloc(ctx, L.bytes);
  if (rc == SVSDF_OK && !ctx->fstage.h_astar) rc = ctx->fstage.h_astar.alloc(ctx, 1);
  if (rc) return rc;
  static_assert(sizeof(AstarState) <= lay::kAstarHead, "state header");
  AstarDev &a = fm.astar;
  unsigned char *b = fm.d_astar;
  a.st = lay::at<AstarState>(b, L.st);
  a.g = lay::at<double>(b, L.g); a.f = lay::at<double>(b, L.f); a.yaw = lay::at<double>(b, L.yaw);
  a.okey = lay::at<double>(b, L.okey);
  a.oseq = lay::at<unsigned long long>(b, L.oseq);
  a.path_yaw = lay::at<double>(b, L.path_yaw);
  a.father = lay::at<int>(b, L.father); a.ocell = lay::at<int>(b, L.ocell); a.path_cell = lay::at<int>(b, L.path_cell);
  a.id = lay::at<signed char>(b, L.id);
  a.open_cap = (int)L.open_cap;
  return SVSDF_OK;
}

// isInMap (Gridmap3D.cpp:43-71)
static bool astar_in_map(const FrontMapDev &fm, const double p[3]) {
  for (int d = 0; d < 3; ++d)
    if (p[d] < fm.bmin[d] || p[d] > fm.bmax[d]) return false;
  return true;
}
// getGridIndex (Gridmap3D.cpp:137-177) of a point inside the map, one axis
static int astar_axis_index(double p, double bmin, double res, int size) {
  int i = (int)std::floor((p - bmin) / res);
  if (i < 0) i = 0;
  if (i >= size) i = size - 1;
  return i;
}

int svsdf_astar_search(svsdf_ctx *group, const double start_xyz[3], const double end_xyz[3], const svsdf_astar_params *params,
                       double *path_xyyaw, int *path_ij, size_t capacity_cells, svsdf_astar_result *result) {
  return on_device(group, __func__, [&](svsdf_ctx *ctx) -> int {
    if (!ctx->fmap.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: no map (svsdf_frontend_set_map)");
    if (!start_xyz || !end_xyz || !result) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: null argument");
    svsdf_astar_params prm;
    svsdf_astar_params_default(&prm);
    if (params) {
      if (params->struct_size != (int)sizeof(svsdf_astar_params))
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: params->struct_size is not sizeof(svsdf_astar_params)");
      prm = *params;
    }
    if (result->struct_size != (int)sizeof(svsdf_astar_result))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: result->struct_size is not sizeof(svsdf_astar_result)");
    const FrontMapDev &fm = ctx->fmap.dev;
    {
      double cy;
      int ki;
      if (kernel_bfs(0ull, fm.kernel_count, prm.start_yaw, &cy, &ki) < 0)
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: start_yaw maps to a kernel index outside [0, kernel_count)");
    }
    if (prm.slice < 0) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: slice < 0");
    if (prm.max_expansions < 0) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: max_expansions < 0");
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(start_xyz[d]) || !std::isfinite(end_xyz[d]))
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: start or end not finite");
    *result = svsdf_astar_result{};
    result->struct_size = (int)sizeof(svsdf_astar_result);
    if (!astar_in_map(fm, start_xyz) || !astar_in_map(fm, end_xyz)) {   // front_end_Astar.hpp:249-254
      result->status = SVSDF_ASTAR_OUT_OF_MAP;
      return SVSDF_OK;
    }
    if (astar_axis_index(start_xyz[2], fm.bmin[2], fm.res, ctx->fmap.Z) != 0 || astar_axis_index(end_xyz[2], fm.bmin[2], fm.res, ctx->fmap.Z) != 0)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: the search is planar in layer 0; the z index of start or end is not 0");
    const int slice = prm.slice ? prm.slice : kAstarDefaultSlice;

    HIPCHK(hipSetDevice(ctx->device));
    int rc = astar_alloc(ctx);
    if (rc) return rc;
    const AstarDev &a = ctx->fmap.astar;
    const size_t cells = (size_t)fm.X * fm.Y;
    hipStream_t st = ctx->stream;
    ctx->fmap.searched = false;
    // AstarPathSearcher::reset (:154-163) + the search's own state
    AstarState *h = ctx->fstage.h_astar;
    *h = AstarState{};
    h->status = kAstarRunning;
    h->si = astar_axis_index(start_xyz[0], fm.bmin[0], fm.res, fm.X);
    h->sj = astar_axis_index(start_xyz[1], fm.bmin[1], fm.res, fm.Y);
    h->gi = astar_axis_index(end_xyz[0], fm.bmin[0], fm.res, fm.X);
    h->gj = astar_axis_index(end_xyz[1], fm.bmin[1], fm.res, fm.Y);
    h->max_expansions = (unsigned long long)prm.max_expansions;
    h->start_yaw = prm.start_yaw;
    h->pushes = 1ull;   // the start node's own openSet.insert (:283); the kernel counts the neighbours'
    HIPCHK(hipMemsetAsync(a.g, 0, 3 * cells * sizeof(double), st));       // g | f | yaw
    HIPCHK(hipMemsetAsync(a.father, 0xff, cells * sizeof(int), st));      // -1
    HIPCHK(hipMemsetAsync(a.id, 0, cells, st));
    HIPCHK(hipMemcpyAsync(a.st, h, sizeof(AstarState), hipMemcpyHostToDevice, st));
    unsigned long long launches = 0;
    do {
      if (!launch_k_astar(ctx->cfg.shape_id, st, ctx->sp, fm, a, slice))
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: shape not compiled into this library");
      HIPCHK(hipGetLastError());
      ++launches;
      HIPCHK(hipMemcpyAsync(h, a.st, sizeof(AstarState), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    } while (h->status == kAstarRunning);
    if (h->status < 0 || h->status > SVSDF_ASTAR_LIMIT)
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: internal error: the open set or the path outgrew X * Y + 1 entries");
    ctx->fmap.searched = true;
    result->status = h->status;
    result->path_len = h->status == SVSDF_ASTAR_FOUND ? (size_t)h->path_len : 0;
    result->expansions = h->expansions; result->pushes = h->pushes; result->relaxed_open = h->relaxed_open;
    result->reopened = h->reopened; result->launches = launches;
    for (int k = 0; k < 5; ++k) result->stage_counts[k] = h->stage_counts[k];
    result->g_goal = h->status == SVSDF_ASTAR_FOUND ? h->g_goal : 0.0;
    const size_t n = result->path_len;
    if ((path_xyyaw || path_ij) && n) {
      if (capacity_cells < n)
        return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_search: capacity_cells too small (result->path_len cells are needed)");
      std::vector<int> cell(n);
      std::vector<double> yaw(n);
      HIPCHK(hipMemcpyAsync(cell.data(), a.path_cell, n * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(yaw.data(), a.path_yaw, n * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (size_t k = 0; k < n; ++k) {
        const int i = cell[k] / fm.Y, j = cell[k] - i * fm.Y;
        if (path_ij) { path_ij[2 * k] = i; path_ij[2 * k + 1] = j; }
        if (path_xyyaw) {   // getGridCubeCenter (Gridmap3D.cpp:184-195), coord(2) = yaw (:381)
          path_xyyaw[3 * k] = (i + 0.5) * fm.res + fm.bmin[0];
          path_xyyaw[3 * k + 1] = (j + 0.5) * fm.res + fm.bmin[1];
          path_xyyaw[3 * k + 2] = yaw[k];
        }
      }
    }
    return SVSDF_OK;
  });
}

int svsdf_astar_nodes(const svsdf_ctx *group, signed char *id, double *g, double *f, double *yaw, int *father_cell,
                      size_t capacity, int dims2[2]) {
  // (const: the error string is the only thing written)
  return on_device(const_cast<svsdf_ctx *>(group), __func__, [&](svsdf_ctx *ctx) -> int {
    const FrontMap &fm = ctx->fmap;
    if (!fm.set) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_nodes: no map (svsdf_frontend_set_map)");
    if (dims2) { dims2[0] = fm.dev.X; dims2[1] = fm.dev.Y; }
    if (!id && !g && !f && !yaw && !father_cell) return SVSDF_OK;
    if (!fm.searched) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_nodes: no search on this map yet (svsdf_astar_search)");
    const size_t n = (size_t)fm.dev.X * fm.dev.Y;
    if (capacity < n) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_astar_nodes: capacity too small (query with all pointers NULL first)");
    const AstarDev &a = fm.astar;
    hipStream_t st = ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (id) HIPCHK(hipMemcpyAsync(id, a.id, n, hipMemcpyDeviceToHost, st));
    if (g) HIPCHK(hipMemcpyAsync(g, a.g, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (f) HIPCHK(hipMemcpyAsync(f, a.f, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (yaw) HIPCHK(hipMemcpyAsync(yaw, a.yaw, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (father_cell) HIPCHK(hipMemcpyAsync(father_cell, a.father, n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SVSDF_OK;
  });
}

// ---- mesh shapes (host) ------------------------------------------------------------------------------
static int outline_out(const std::vector<double> &xy, double *xy_out, size_t capacity_verts, size_t *count) {
  return deliver(Out<double>{xy, 2, xy_out, capacity_verts, count}) ? SVSDF_OK : SVSDF_ERR_INVALID;
}
int svsdf_mesh_outline(const double *V, size_t nv, const int *F, size_t nf, double z0, double *xy_out,
                       size_t capacity_verts, size_t *count, int *loops) {
  if (!V || !F || !count || !std::isfinite(z0)) return SVSDF_ERR_INVALID;
  std::vector<double> xy;
  if (!svsdf_host::mesh_outline(V, nv, F, nf, z0, xy, loops)) return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_mesh_outline: no closed cross-section at z0");
  return outline_out(xy, xy_out, capacity_verts, count);
}
static int section_out(const std::vector<double> &xy, const std::vector<int> &sizes, double *xy_out, size_t capacity_verts,
                       size_t *n_verts, int *loop_sizes, size_t capacity_loops, size_t *n_loops) {
  const bool ok = deliver(Out<double>{xy, 2, xy_out, capacity_verts, n_verts}, Out<int>{sizes, 1, loop_sizes, capacity_loops, n_loops});
  return ok && (xy_out == nullptr) == (loop_sizes == nullptr) ? SVSDF_OK : SVSDF_ERR_INVALID;   // both outputs, or neither
}
int svsdf_mesh_section(const double *V, size_t nv, const int *F, size_t nf, double z0, double *xy_out, size_t capacity_verts,
                       size_t *n_verts, int *loop_sizes, size_t capacity_loops, size_t *n_loops) {
  if (!V || !F || !n_verts || !n_loops || !std::isfinite(z0)) return SVSDF_ERR_INVALID;
  std::vector<double> xy;
  std::vector<int> sizes;
  if (!svsdf_host::mesh_section(V, nv, F, nf, z0, xy, sizes)) return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_mesh_section: no closed cross-section at z0");
  return section_out(xy, sizes, xy_out, capacity_verts, n_verts, loop_sizes, capacity_loops, n_loops);
}
int svsdf_mesh_section_obj(const char *obj_path, double z0, double *xy_out, size_t capacity_verts, size_t *n_verts,
                           int *loop_sizes, size_t capacity_loops, size_t *n_loops) {
  if (!obj_path || !n_verts || !n_loops || !std::isfinite(z0)) return SVSDF_ERR_INVALID;
  std::vector<double> V, xy;
  std::vector<int> F, sizes;
  if (!svsdf_host::read_obj(obj_path, V, F)) return fail(nullptr, SVSDF_ERR_INVALID, std::string("svsdf_mesh_section_obj: cannot read ") + obj_path);
  if (!svsdf_host::mesh_section(V.data(), V.size() / 3, F.data(), F.size() / 3, z0, xy, sizes))
    return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_mesh_section_obj: no closed cross-section at z0");
  return section_out(xy, sizes, xy_out, capacity_verts, n_verts, loop_sizes, capacity_loops, n_loops);
}
int svsdf_mesh_outline_obj(const char *obj_path, double z0, double *xy_out, size_t capacity_verts, size_t *count,
                           int *loops) {
  if (!obj_path || !count || !std::isfinite(z0)) return SVSDF_ERR_INVALID;
  std::vector<double> V, xy;
  std::vector<int> F;
  if (!svsdf_host::read_obj(obj_path, V, F)) return fail(nullptr, SVSDF_ERR_INVALID, std::string("svsdf_mesh_outline_obj: cannot read ") + obj_path);
  if (!svsdf_host::mesh_outline(V.data(), V.size() / 3, F.data(), F.size() / 3, z0, xy, loops))
    return fail(nullptr, SVSDF_ERR_INVALID, "svsdf_mesh_outline_obj: no closed cross-section at z0");
  return outline_out(xy, xy_out, capacity_verts, count);
}

// ---- swept-volume outline (what sw_calculate.cpp / SWM:321-336 produce for visual validation) ----------
int svsdf_swept_outline(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, double cell, double margin,
                        double *xy_out, size_t capacity_verts, size_t *n_verts, int *loop_sizes, size_t capacity_loops,
                        size_t *n_loops, svsdf_outline_stats *stats_out) {
  if (!ctx || !coeffs || !T || !n_verts || !n_loops) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_swept_outline: null argument");
  if (N < 1 || N > kMaxPieces || !(cell > 0.0) || !std::isfinite(cell) || !std::isfinite(margin))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_swept_outline: N, cell or margin out of range");
  if ((xy_out == nullptr) != (loop_sizes == nullptr))
    return fail(ctx, SVSDF_ERR_INVALID, "svsdf_swept_outline: xy_out and loop_sizes must both be given (fill) or both be NULL (size query)");
  const svsdf_ctx *base = leaf_of(ctx);
  if (base->host_only) return fail(ctx, SVSDF_ERR_NO_DEVICE, "host-only context: no device entry points");
  // the size query and the fill that follows it carry the same arguments: the second call copies the first one's result
  std::vector<double> key;
  key.reserve(19 * (size_t)N + 3);
  key.push_back((double)N); key.push_back(cell); key.push_back(margin);
  key.insert(key.end(), coeffs, coeffs + 18 * (size_t)N);
  key.insert(key.end(), T, T + N);
  OutlineCache &ol = ctx->outline;
  auto deliver_cached = [&]() -> int {
    if (stats_out) *stats_out = ol.stats;
    if (!deliver(Out<double>{ol.xy, 2, xy_out, capacity_verts, n_verts}, Out<int>{ol.loops, 1, loop_sizes, capacity_loops, n_loops}))
      return fail(ctx, SVSDF_ERR_INVALID, "svsdf_swept_outline: output capacity too small (query with xy_out = NULL first)");
    return SVSDF_OK;
  };
  if (ol.valid && ol.key.size() == key.size() && std::memcmp(ol.key.data(), key.data(), key.size() * sizeof(double)) == 0)
    return deliver_cached();
  // bounding box of the path (body origin), grown by the shape's bound radius: the swept volume lies inside
  double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
  for (int i = 0; i < N; ++i) {
    if (!(T[i] > 0.0) || !std::isfinite(T[i])) return fail(ctx, SVSDF_ERR_NONFINITE, "svsdf_swept_outline: bad duration");
    for (int q = 0; q <= 32; ++q) {
      const double sl = T[i] * (double)q / 32.0;
      for (int d = 0; d < 2; ++d) {
        double v = 0.0;
        for (int k = 5; k >= 0; --k) v = v * sl + coeffs[(size_t)d * 6 * N + (size_t)i * 6 + k];
        if (!std::isfinite(v)) return fail(ctx, SVSDF_ERR_NONFINITE, "svsdf_swept_outline: non-finite trajectory");
        lo[d] = std::min(lo[d], v); hi[d] = std::max(hi[d], v);
      }
    }
  }
  // (a quintic between samples 1/32 of a piece apart can leave the sampled box by a little: one more bound radius)
  const double grow = 2.0 * base->r_bound + std::max(margin, 0.0) + 4.0 * cell;
  svsdf_host::ContourGrid g;
  g.h = cell;
  g.levels = 4;
  g.x0 = lo[0] - grow; g.y0 = lo[1] - grow;
  const double wx = (hi[0] - lo[0]) + 2.0 * grow, wy = (hi[1] - lo[1]) + 2.0 * grow;
  if (wx / cell > 1e6 || wy / cell > 1e6) return fail(ctx, SVSDF_ERR_INVALID, "svsdf_swept_outline: more than 1e6 cells per side");
  g.nx = (long long)std::ceil(wx / cell); g.ny = (long long)std::ceil(wy / cell);
  // a private single-device context with the same shape and weights: the caller's resident cloud stays as it is
  svsdf_config c = base->cfg;
  c.n_devices = 0; c.rank = 0; c.world_size = 1; c.combine = SVSDF_COMBINE_AUTO; c.device = base->device;
  c.polygon_xy = base->poly_xy.empty() ? nullptr : base->poly_xy.data();
  c.polygon_nverts = (int)(base->poly_xy.size() / 2);
  c.polygon_loop_sizes = base->poly_loops.empty() ? nullptr : base->poly_loops.data();
  c.polygon_nloops = (int)base->poly_loops.size();
  svsdf_ctx *tmp = svsdf_create(&c);
  if (!tmp) return fail(ctx, SVSDF_ERR_INVALID, std::string("svsdf_swept_outline: ") + svsdf_last_error_string(nullptr));
  tmp->scaled = ctx->scaled;   // sw_calculate runs <useScale> too: the caller's scale schedule (svsdf_set_scale)
  tmp->scale = ctx->scale;
  std::vector<double> xyz, sdf;
  std::vector<long long> idx;
  const svsdf_host::FieldEval eval = [&](const std::vector<double> &xy, std::vector<double> &val) -> int {
    const size_t P = xy.size() / 2;
    xyz.resize(3 * P);
    for (size_t k = 0; k < P; ++k) { xyz[3 * k] = xy[2 * k]; xyz[3 * k + 1] = xy[2 * k + 1]; xyz[3 * k + 2] = 0.0; }
    int rc = svsdf_set_points(tmp, xyz.data(), P);
    if (rc) return rc;
    if (svsdf_num_points(tmp) != P) return SVSDF_ERR_INVALID;
    sdf.resize(P); idx.resize(P);
    rc = swept_field(tmp, N, coeffs, T, sdf.data());
    if (rc) return rc;
    rc = svsdf_shard_indices(tmp, idx.data());
    if (rc) return rc;
    val.assign(P, 0.0);
    for (size_t k = 0; k < P; ++k) {
      if (!std::isfinite(sdf[k])) return SVSDF_ERR_NONFINITE;   // (a NaN would silently read as "outside")
      val[(size_t)idx[k]] = sdf[k];
    }
    return 0;
  };
  std::vector<double> xy;
  std::vector<int> loops;
  svsdf_host::ContourStats st;
  const int rc = svsdf_host::swept_contour(g, eval, 1.5, xy, loops, &st);
  const std::string tmp_err = rc ? svsdf_last_error_string(tmp) : "";
  svsdf_destroy(tmp);
  if (rc) return fail(ctx, rc > 0 ? rc : SVSDF_ERR_INVALID, "svsdf_swept_outline: evaluation failed: " + tmp_err);
  ol.stats = svsdf_outline_stats{};
  ol.stats.nodes_evaluated = st.nodes_evaluated; ol.stats.dense_nodes = st.dense_nodes;
  ol.stats.cells_marched = st.cells_marched; ol.stats.batches = st.batches; ol.stats.open_chains = st.open_chains;
  ol.key.swap(key);
  ol.xy = xy;
  ol.loops = loops;
  ol.valid = true;
  return deliver_cached();
}

int svsdf_outline_extrude(const double *xy, const int *loop_sizes, size_t n_loops, double z0, double z1, int caps,
                          double *V_out, size_t capacity_verts, size_t *n_verts, int *F_out, size_t capacity_tris,
                          size_t *n_tris) {
  if (!n_verts || !n_tris || !std::isfinite(z0) || !std::isfinite(z1)) return SVSDF_ERR_INVALID;
  if (n_loops == 0) { *n_verts = 0; *n_tris = 0; return SVSDF_OK; }   // an empty outline extrudes to an empty surface
  if (!xy || !loop_sizes) return SVSDF_ERR_INVALID;
  for (size_t l = 0; l < n_loops; ++l)
    if (loop_sizes[l] < 3) return SVSDF_ERR_INVALID;
  std::vector<double> V;
  std::vector<int> F;
  svsdf_host::extrude_outline(xy, loop_sizes, n_loops, z0, z1, caps != 0, V, F);
  return deliver(Out<double>{V, 3, V_out, capacity_verts, n_verts}, Out<int>{F, 3, F_out, capacity_tris, n_tris}) ? SVSDF_OK : SVSDF_ERR_INVALID;
}

}  // extern "C"

// ---- optimizer driver (host) ---------------------------------------------------
void svsdf_lbfgs_params_default(svsdf_lbfgs_params *p) {
  if (!p) return;
  p->mem_size = 8; p->g_epsilon = 1.0e-5; p->past = 3; p->delta = 1.0e-6; p->max_iterations = 0;
  p->max_linesearch = 64; p->min_step = 1.0e-20; p->max_step = 1.0e+20; p->f_dec_coeff = 1.0e-4;
  p->s_curv_coeff = 0.9; p->cautious_factor = 1.0e-6; p->machine_prec = 1.0e-16;
}

int svsdf_lbfgs_minimize(int n, double *x, svsdf_evaluate_t eval, void *instance, svsdf_progress_t progress,
                         void *progress_user, const svsdf_lbfgs_params *params, double *final_cost,
                         int *iterations, int *evaluations) {
  if (!x || !eval) return SVSDF_LBFGSERR_INVALIDPARAMETERS;
  svsdf_lbfgs_params p;
  if (params) p = *params; else svsdf_lbfgs_params_default(&p);
  const svsdf_host::LbfgsResult r = svsdf_host::lbfgs_minimize(n, x, eval, instance, progress, progress_user, p);
  if (final_cost) *final_cost = r.fx;
  if (iterations) *iterations = r.iterations;
  if (evaluations) *evaluations = r.evaluations;
  return r.status;
}

int svsdf_optimize_traj(svsdf_ctx *ctx, double *x, int n, const svsdf_lbfgs_params *params,
                        svsdf_progress_t progress, void *progress_user, double *final_cost, int *iterations,
                        int *evaluations) {
  if (!ctx || !x || n < 1 || (n + 3) % 4 != 0) {
    fail(ctx, SVSDF_ERR_INVALID, "svsdf_optimize_traj: n must be N + 3(N-1)");
    return SVSDF_LBFGSERR_INVALIDPARAMETERS;
  }
  // As in the reference, the side outputs (svsdf_last_costs, MINCO state) are those of the LAST callback
  // evaluation -- after a failed line search that is a trial point, not the returned x -- and the objective is
  // history dependent once a trial's total duration reaches 300 s (stale traj_duration, sw_manager.hpp:380-384):
  // the value reported is the one the driver accepted, no re-evaluation is made here.
  const int rc = svsdf_lbfgs_minimize(n, x, svsdf_lmbm_evaluate, ctx, progress, progress_user, params, final_cost,
                                      iterations, evaluations);
  return rc;
}
