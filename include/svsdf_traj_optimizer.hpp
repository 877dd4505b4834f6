// svsdf_traj_optimizer.hpp -- C++ host-side mirror of the reference's TrajOptimizer for the
// SVSDF cost path, on top of the C ABI (svsdf_c.h).  Header-only; link with libsvsdf_hip.so.
//
// Same member names / callback signatures as the reference so that plan_manager code keeps
// compiling against it (BEO = src/planner_algorithm/include/planner_algorithm/back_end_optimizer.hpp):
//   TrajOptimizer::costFunctionLmbmParallel(void*, const double*, double*, const int)   BEO:344-408
//     == lmbm::lmbm_evaluate_t (src/utils/include/utils/lmbm.h:206-209)
//   TrajOptimizer::addSaftyPenaOnSweptVolumeParallelTrueSDF(ptr, T, coeffs, cost, gradT, gradC)
//                                                                                        BEO:774-869
//   cost_pos / cost_other / cost_total                                                   BEO:396-398
// With Eigen available the Eigen-typed overloads and the lbfgs::lbfgs_evaluate_t adapter
// (src/utils/include/utils/lbfgs.hpp:213-216) are compiled in as well.
#pragma once
#include <cstddef>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "svsdf_c.h"

// Eigen is optional.  SVSDF_EIGEN_HEADER lets a build point at another header providing Eigen::VectorXd /
// Eigen::MatrixX3d with data() and size() (tests/cpp/mini_eigen.hpp: this image has no Eigen).
#if defined(SVSDF_EIGEN_HEADER)
#include SVSDF_EIGEN_HEADER
#define SVSDF_HAVE_EIGEN 1
#elif defined(__has_include)
#if __has_include(<Eigen/Core>)
#include <Eigen/Core>
#define SVSDF_HAVE_EIGEN 1
#endif
#endif

namespace svsdf {

class TrajOptimizerHip {
 public:
  // --- Config-derived members (BEO:69-95) ---
  double rho = 3.8;
  double weight_p = 60.0;
  double safety_hor = 0.7;
  int threads_num = 30;  // kept for source compatibility; the GPU path ignores it
  std::string inputdata = "shapes/star.obj";
  double poly_params[3] = {0.0, 0.0, 0.0};
  std::string package_path;        // what ros::package::getPath("plan_manager") returns (Shape.hpp:283): prefix of inputdata
  std::string mesh_error;          // why context() returned nullptr for a mesh `inputdata` (cross-section too large)
  std::vector<double> polygon_xy;  // optional outline for the Polygon fallback; empty + an inputdata stem the shape
                                   // registry does not know -> the z = 0 section of that .obj mesh (BASELINE config 5)
  std::vector<int> polygon_loops;  // with polygon_xy: vertices per closed loop (empty: one loop)
  int device = -1;
  int rank = 0, world_size = 1;
  std::vector<int> devices;        // >= 2 entries: in-process multi-GPU (svsdf_config::n_devices / devices); 1 entry: that device
  int combine = SVSDF_COMBINE_AUTO;
  bool polygon_front_end = false;  // a Polygon context (mesh inputdata, polygon_xy) is created with
                                   // SVSDF_FLAG_POLYGON_YAW_KERNELS: svsdf_frontend_set_map / svsdf_astar_search work on it

  // --- optimisation state (BEO:44-60) ---
  int pieceN = 0, temporalDim = 0, spatialDim = 0;
  double initState[9] = {0}, finalState[9] = {0};  // 3x3 column-major
  int parallel_points_num = 0;
  std::vector<double> parallel_points;  // xyz AoS (Eigen::Vector3d layout)
  double cost_pos = 0.0, cost_other = 0.0, cost_total = 0.0;

  TrajOptimizerHip() = default;
  TrajOptimizerHip(const TrajOptimizerHip &) = delete;
  TrajOptimizerHip &operator=(const TrajOptimizerHip &) = delete;
  ~TrajOptimizerHip() { svsdf_destroy(ctx_); }

  // plan_manager.cpp:168-175
  void setPoints(const double *xyz_aos, std::size_t P) {
    parallel_points.assign(xyz_aos, xyz_aos + 3 * P);
    parallel_points_num = (int)P;
    points_dirty_ = true;
  }
  // first lines of optimize_traj_lmbm (back_end_optimizer.cpp:13-19); initS/finalS 3x3 col-major
  void setConditions(const double initS[9], const double finalS[9], int N) {
    pieceN = N; temporalDim = N; spatialDim = 3 * (N - 1);
    std::memcpy(initState, initS, sizeof(initState));
    std::memcpy(finalState, finalS, sizeof(finalState));
    // the context (resident cloud, launch plan, SweptVolumeManager's persistent traj_duration SWM:376-385)
    // survives successive optimisations; only the boundary states change
    if (ctx_ && svsdf_set_conditions(ctx_, initState, finalState) != SVSDF_OK) { svsdf_destroy(ctx_); ctx_ = nullptr; }
  }
  // Config-derived members (shape, weights, devices ...) may be edited between optimisations like the reference's public
  // members: context() compares them with what the live context was built from and rebuilds it on a mismatch.
  void resetContext() { svsdf_destroy(ctx_); ctx_ = nullptr; }

  // useScale + getScale (sw_manager.hpp:17, 495-503): the time-varying scale schedule of this optimiser (svsdf_set_scale;
  // nullptr or enabled = 0: rigid).  Checked by the library at once (on the live context, or on a host-only one when none
  // exists yet); kept across context rebuilds.
  int setScale(const svsdf_scale *s) {
    int rc;
    if (ctx_) {
      rc = svsdf_set_scale(ctx_, s);
    } else {
      svsdf_config cfg;
      svsdf_config_default(&cfg);
      cfg.flags = SVSDF_FLAG_HOST_ONLY;
      svsdf_ctx *probe = svsdf_create(&cfg);
      if (!probe) return SVSDF_ERR_INVALID;
      rc = svsdf_set_scale(probe, s);
      svsdf_destroy(probe);
    }
    if (rc != SVSDF_OK) return rc;
    has_scale_ = s != nullptr && s->enabled != 0;
    if (has_scale_) scale_ = *s;
    return SVSDF_OK;
  }
  int getScale(svsdf_scale *out) const {
    if (!out || out->struct_size != (int)sizeof(svsdf_scale)) return SVSDF_ERR_INVALID;
    if (has_scale_) { *out = scale_; return SVSDF_OK; }
    *out = svsdf_scale{};
    out->struct_size = (int)sizeof(svsdf_scale);
    out->c[0] = out->c[1] = 1.0;
    return SVSDF_OK;
  }

  // static double costFunctionLmbmParallel(void *ptr, const double *x, double *g, const int n)
  static double costFunctionLmbmParallel(void *ptr, const double *x_variable, double *g, const int n) {
    TrajOptimizerHip &obj = *static_cast<TrajOptimizerHip *>(ptr);
    svsdf_ctx *ctx = obj.context();
    if (!ctx || n != obj.temporalDim + obj.spatialDim) {
      if (g) std::memset(g, 0, sizeof(double) * (n > 0 ? n : 0));
      return std::numeric_limits<double>::infinity();
    }
    const double cost = svsdf_lmbm_evaluate(ctx, x_variable, g, n);
    double c3[3] = {0, 0, 0};
    svsdf_last_costs(ctx, c3);
    obj.cost_pos = c3[0]; obj.cost_other = c3[1]; obj.cost_total = c3[2];
    return cost;
  }

  // static void addSaftyPenaOnSweptVolumeParallelTrueSDF(ptr, T, coeffs, cost, gradT, gradC)
  // raw-pointer form: T[N], coeffs/gradC (6N) x 3 column-major; accumulates (+=).
  static int addSaftyPenaOnSweptVolumeParallelTrueSDF(void *ptr, const double *T, const double *coeffs, int N,
                                                      double &cost, double *gradT, double *gradC) {
    TrajOptimizerHip &obj = *static_cast<TrajOptimizerHip *>(ptr);
    svsdf_ctx *ctx = obj.context();
    if (!ctx) return SVSDF_ERR_NO_DEVICE;
    return svsdf_eval_penalty(ctx, N, coeffs, T, &cost, gradT, gradC);
  }

  // optimize_traj_lmbm (back_end_optimizer.cpp:3-95) with the library's L-BFGS driver in place of
  // lmbm::lmbm_optimize: initS/finalS 3x3 col-major, opt_x[N + 3(N-1)] in/out.  Returns the solver status
  // (>= 0 success, with 0 mapped to 1 like back_end_optimizer.cpp:62-65); final_cost may be null.
  int optimize_traj_lmbm(const double initS[9], const double finalS[9], double *opt_x, const int N,
                         double *final_cost = nullptr, const svsdf_lbfgs_params *param = nullptr) {
    setConditions(initS, finalS, N);
    svsdf_ctx *ctx = context();
    if (!ctx) return SVSDF_LBFGSERR_INVALIDPARAMETERS;
    int ret = svsdf_optimize_traj(ctx, opt_x, temporalDim + spatialDim, param, nullptr, nullptr, final_cost,
                                  &iter, nullptr);
    double c3[3] = {0, 0, 0};
    svsdf_last_costs(ctx, c3);  // of the last callback evaluation, like the reference's members
    cost_pos = c3[0]; cost_other = c3[1]; cost_total = c3[2];
    if (ret == 0) ret = 1;
    return ret;
  }
  int iter = 0;  // iterations of the last optimize_traj_lmbm (TrajOptimizer::iter, back_end_optimizer.hpp)

  // SweptVolumeManager::calculateSwept(U_, G_) (sw_manager.hpp:321-336 -> sw_calculate.cpp:4-305; unused in the release,
  // shown with vis->visMesh): vertices U (3 per row) and triangles G (3 zero-based indices per row) of the swept volume's
  // closed surface for the trajectory (T[N], coeffs (6N) x 3 column-major) -- the outline of its z = 0 section
  // (svsdf_swept_outline, cell size `cell`) extruded over [zmin, zmax] (the shipped meshes are slabs |z| <= 0.5), walls + caps.
  // outline_xy / loop_sizes (may be null) receive the closed polylines themselves.  Returns 0 or an SVSDF_ERR_* code.
  int calculateSwept(const double *T, const double *coeffs, int N, std::vector<double> &U, std::vector<int> &G,
                     double cell = 0.05, double zmin = -0.5, double zmax = 0.5, std::vector<double> *outline_xy = nullptr,
                     std::vector<int> *loop_sizes = nullptr) {
    svsdf_ctx *ctx = context();
    if (!ctx) return SVSDF_ERR_NO_DEVICE;
    std::size_t nv = 0, nl = 0;
    int rc = svsdf_swept_outline(ctx, N, coeffs, T, cell, 0.0, nullptr, 0, &nv, nullptr, 0, &nl, nullptr);
    if (rc) return rc;
    std::vector<double> xy(2 * nv);
    std::vector<int> sizes(nl);
    if (nv) {
      rc = svsdf_swept_outline(ctx, N, coeffs, T, cell, 0.0, xy.data(), nv, &nv, sizes.data(), nl, &nl, nullptr);
      if (rc) return rc;
    }
    std::size_t mv = 0, mf = 0;
    rc = svsdf_outline_extrude(xy.data(), sizes.data(), nl, zmin, zmax, 1, nullptr, 0, &mv, nullptr, 0, &mf);
    if (rc) return rc;
    U.assign(3 * mv, 0.0);
    G.assign(3 * mf, 0);
    if (mv) rc = svsdf_outline_extrude(xy.data(), sizes.data(), nl, zmin, zmax, 1, U.data(), mv, &mv, G.data(), mf, &mf);
    if (outline_xy) *outline_xy = xy;
    if (loop_sizes) *loop_sizes = sizes;
    return rc;
  }

#ifdef SVSDF_HAVE_EIGEN
  static void addSaftyPenaOnSweptVolumeParallelTrueSDF(void *ptr, const Eigen::VectorXd &T,
                                                       const Eigen::MatrixX3d &coeffs, double &cost,
                                                       Eigen::VectorXd &gradT, Eigen::MatrixX3d &gradC) {
    const int rc = addSaftyPenaOnSweptVolumeParallelTrueSDF(ptr, T.data(), coeffs.data(), (int)T.size(), cost,
                                                            gradT.data(), gradC.data());
    if (rc) throw std::runtime_error("svsdf_eval_penalty failed: " + std::to_string(rc));
  }
  // lbfgs::lbfgs_evaluate_t adapter (lbfgs.hpp:213-216): p_cost receives cost_pos
  static double costFunctionLbfgs(void *ptr, const Eigen::VectorXd &x, Eigen::VectorXd &g, double &p_cost) {
    const double f = costFunctionLmbmParallel(ptr, x.data(), g.data(), (int)x.size());
    p_cost = static_cast<TrajOptimizerHip *>(ptr)->cost_pos;
    return f;
  }
#endif

  svsdf_ctx *context() {
    const std::string key = config_key();
    if (ctx_ && key != built_key_) resetContext();
    if (!ctx_) {
      svsdf_config cfg;
      svsdf_config_default(&cfg);
      cfg.shape_id = polygon_xy.empty() ? svsdf_shape_id_from_inputdata(inputdata.c_str()) : (int)SVSDF_SHAPE_Polygon;
      std::vector<double> outline = polygon_xy;
      std::vector<int> loop_sizes = polygon_loops;
      if (cfg.shape_id == SVSDF_SHAPE_Polygon && outline.empty()) {
        // an .obj the shape registry does not know: its whole z = 0 section -- every closed loop (a hole, several solids:
        // round 5; rounds 3-4 refused such meshes) -- (the reference reads the same file with igl::read_triangle_mesh,
        // Shape.hpp:281-284); unreadable -> the reference's hard-coded rectangle (SWM:363-369)
        const std::string path = package_path.empty() ? inputdata : package_path + "/" + inputdata;
        std::size_t n = 0, nl = 0;
        if (svsdf_mesh_section_obj(path.c_str(), 0.0, nullptr, 0, &n, nullptr, 0, &nl) == SVSDF_OK && n >= 3) {
          if (n + nl > (std::size_t)SVSDF_MAX_POLY_VERTS) { mesh_error = path + ": the z = 0 cross-section has " + std::to_string(n) + " vertices (max " + std::to_string(SVSDF_MAX_POLY_VERTS) + ")"; return nullptr; }
          outline.resize(2 * n);
          loop_sizes.resize(nl);
          if (svsdf_mesh_section_obj(path.c_str(), 0.0, outline.data(), n, &n, loop_sizes.data(), nl, &nl) != SVSDF_OK) { outline.clear(); loop_sizes.clear(); }
        }
      }
      std::memcpy(cfg.poly_params, poly_params, sizeof(poly_params));
      cfg.safety_hor = safety_hor; cfg.weight_p = weight_p; cfg.rho = rho;
      std::memcpy(cfg.head_state, initState, sizeof(initState));
      std::memcpy(cfg.tail_state, finalState, sizeof(finalState));
      cfg.device = device; cfg.rank = rank; cfg.world_size = world_size;
      cfg.combine = combine;
      if (polygon_front_end && cfg.shape_id == SVSDF_SHAPE_Polygon) cfg.flags |= SVSDF_FLAG_POLYGON_YAW_KERNELS;
      if (devices.size() == 1 && combine != SVSDF_COMBINE_RCCL) cfg.device = devices[0];
      else if (!devices.empty() && devices.size() <= SVSDF_MAX_DEVICES) {
        cfg.n_devices = (int)devices.size();
        for (std::size_t k = 0; k < devices.size(); ++k) cfg.devices[k] = devices[k];
      }
      cfg.polygon_nverts = (int)(outline.size() / 2);
      cfg.polygon_xy = outline.empty() ? nullptr : outline.data();
      cfg.polygon_nloops = (loop_sizes.size() >= 2) ? (int)loop_sizes.size() : 0;
      cfg.polygon_loop_sizes = (loop_sizes.size() >= 2) ? loop_sizes.data() : nullptr;
      ctx_ = svsdf_create(&cfg);
      if (ctx_ && has_scale_ && svsdf_set_scale(ctx_, &scale_) != SVSDF_OK) { svsdf_destroy(ctx_); ctx_ = nullptr; }
      built_key_ = key;
      points_dirty_ = true;
    }
    if (ctx_ && points_dirty_) {
      if (svsdf_set_points(ctx_, parallel_points.data(), (std::size_t)parallel_points_num) != SVSDF_OK) return nullptr;
      points_dirty_ = false;
    }
    return ctx_;
  }

 private:
  // everything svsdf_create reads except the boundary states (those go through svsdf_set_conditions)
  std::string config_key() const {
    std::string k = inputdata + "|" + package_path + "|";
    auto add = [&k](const void *p, std::size_t n) { k.append(static_cast<const char *>(p), n); };
    add(&rho, sizeof rho); add(&weight_p, sizeof weight_p); add(&safety_hor, sizeof safety_hor);
    add(poly_params, sizeof poly_params); add(&device, sizeof device); add(&rank, sizeof rank);
    add(&world_size, sizeof world_size); add(&combine, sizeof combine);
    add(&polygon_front_end, sizeof polygon_front_end);
    if (!devices.empty()) add(devices.data(), devices.size() * sizeof(int));
    k += "|";
    if (!polygon_xy.empty()) add(polygon_xy.data(), polygon_xy.size() * sizeof(double));
    k += "|";
    if (!polygon_loops.empty()) add(polygon_loops.data(), polygon_loops.size() * sizeof(int));
    return k;
  }
  std::string built_key_;
  svsdf_ctx *ctx_ = nullptr;
  bool has_scale_ = false;
  svsdf_scale scale_{};
  bool points_dirty_ = true;
};

}  // namespace svsdf
