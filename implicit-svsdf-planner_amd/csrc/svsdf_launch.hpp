// svsdf_launch.hpp -- host-side launchers of the shape-templated kernels.
//
// The kernels are specialised per shape id (17 shapes x lane-group widths x GSIP bound modes: ~580 kernels).  They are
// compiled in SVSDF_NSLICES translation units (svsdf_shape_slice.hip with -DSVSDF_SLICE=k holds the shapes with
// id % SVSDF_NSLICES == k) so that the build runs in parallel; svsdf_pipeline.hip only sees these plain functions.
#pragma once
#include <hip/hip_runtime.h>

#include "svsdf_kernels.hpp"
#include "svsdf_frontend.hpp"
#include "svsdf_clearance.hpp"

namespace svsdf {

constexpr int kNSlices = 4;

struct SolveLaunch {   // arguments of k_solve<SHAPE, G, 1>
  const TrajDev *traj; const double *tk; const Pose *pose; const Chunk *chunks; ShapeParams sp; QuerySet qs;
  double *out_sdf, *out_t; int prune /* kSolve* bits */; BatchCtl *ctl; int work_idx; double cull_thresh;
  const double *rot; double slack_max;   // second exact cull (main points): per-chunk yaw allowance W_c h, max_c of the linear one
  const ScaleDev *scl = nullptr;         // not null: k_solve<SHAPE, G, 1, ScaleDev> under this scale schedule (G in kScaledLanes)
  const Pose *ltab = nullptr;            // layer-2 pose table, layer 3's behind it (k_layer_tables); kSolveLayer2 / kSolveLayer3 in `prune` say which the launch uses
};
struct RoundLaunch {   // arguments of k_round<SHAPE, LP, MODE>
  const TrajDev *traj; const Pose *pose; const Chunk *chunks; ShapeParams sp; const double *px, *py; GsipState gs;
  size_t stride; int it; double delta, band_delta; double *res_sdf, *res_t, *res_gx, *res_gy; BatchCtl *ctl;
  int clist_on;   // kListScans | kListCheap | kScanAnchors (svsdf_kernels.hpp)
};
struct TailLaunch {    // arguments of k_tail<SHAPE, MODE, WAVES>
  const TrajDev *traj; const double *tk; const Pose *pose; const Chunk *chunks; ShapeParams sp; const double *px, *py;
  GsipState gs; size_t stride; int it0, prev_mode; double delta, band_delta; int all_after, ppw;
  double *res_sdf, *res_t, *res_gx, *res_gy; BatchCtl *ctl; int clist_on, prune;   // clist_on: k_round's bits | kTailLocalState | kTailNoDuo; prune: kSolvePrune
  int latency;   // not a kernel argument: 1 = the instantiation that keeps its registers (kTailLatencyWaves per SIMD, no scratch)
};
struct ClassifyLaunch {   // arguments of k_classify<SHAPE>
  const TrajDev *traj; ShapeParams sp; const double *px, *py, *sdf, *t; double *res_sdf, *res_t, *res_gx, *res_gy;
  GsipState gs; BatchCtl *ctl; int *n_int; int icap;
  const ScaleDev *scl = nullptr;   // not null: k_classify<SHAPE, ScaleDev>
};
struct ClrLaunch {     // arguments of k_clr_level0<SHAPE> (L == 0: tp / ntp, mid, emit) and k_clr_level<SHAPE> (L >= 1: traj, in / n)
  const TrajDev *traj; ShapeParams sp; const double *px, *py; const long long *orig; unsigned P; const Pose *mid;
  const double *V, *W; double w, dur; int L; const ClrTilePair *tp; const ClrPair *in; unsigned n; double thr; int emit;
  ClrPair *out; unsigned out_cap; ClrRecord *rec; ClrPartial *partials;
  const ClrScale *scl = nullptr;   // not null: k_clr_level0 / k_clr_level<SHAPE, ClrScale> under this schedule and its per-interval bounds
};
struct PclrLaunch {    // arguments of k_pclr_level0<SHAPE> (L == 0: tp / ntp, mid, emit) and k_pclr_level<SHAPE> (L >= 1: traj, in / n)
  const TrajDev *traj; ShapeParams sp; const double *px, *py; unsigned P; const Pose *mid; const double *V, *W; double w, dur;
  int L; const ClrTilePair *tp; const ClrPair *in; unsigned n; PclrRule rule; int emit; PclrState s; PclrEval *ev;
  ClrPair *out; unsigned out_cap; PclrCounters *cnt;
  const ClrScale *scl = nullptr;   // not null: k_pclr_level0 / k_pclr_level<SHAPE, ClrScale>
};
// lane-group widths the scaled solve is instantiated for (§4c: a reduced plan space); scaled_lanes maps any width onto them
constexpr int kScaledLanes[3] = {4, 8, 32};
inline int scaled_lanes(int G) { return G >= 32 ? 32 : G >= 8 ? 8 : 4; }
// The rigid / scaled choice of a launch site: f() for the rigid kernel, f(*scl) under a scale schedule (S: ScaleDev, or the
// clearance kernels' ClrScale).  A generic lambda
// `[&](auto... scl)` then holds ONE launch expression for both: k_x<..., decltype(scl)...> with `scl...` among its arguments.
template <typename S, typename F>
auto with_scale(const S *scl, F &&f) { return scl ? f(*scl) : f(); }

// each returns false when the shape id is not compiled into the library (development builds)
bool launch_k_solve(int shape, int G, unsigned grid, unsigned block, size_t lds, hipStream_t st, const SolveLaunch &a);
bool launch_k_round(int shape, int lp, int mode, unsigned grid, size_t lds, hipStream_t st, const RoundLaunch &a);
bool launch_k_classify(int shape, unsigned grid, size_t lds, hipStream_t st, const ClassifyLaunch &a);
bool launch_k_tail(int shape, int mode, unsigned grid, size_t lds, hipStream_t st, const TailLaunch &a);
bool launch_k_rbound(int shape, unsigned grid, hipStream_t st, ShapeParams sp, double rmax, int nrad, int nang, double *out);
bool launch_k_subsw(int shape, dim3 grid, hipStream_t st, ShapeParams sp, const double *father, const double *child,
                    const unsigned long long *offs, const double *pts, const double *kt, int nkt, int *flag);
bool launch_k_shape_kernels(int shape, unsigned grid, hipStream_t st, ShapeParams sp, int ks, int count, double resu,
                            int size_side, double safemargin, const double *yaw, unsigned char *map);
bool launch_k_debug_sdf_at(int shape, unsigned grid, size_t lds, hipStream_t st, const TrajDev *traj, ShapeParams sp,
                           const double *pxy, const double *t, int n, double *out, const ScaleDev *scl = nullptr);
bool launch_k_succ(int shape, unsigned grid, hipStream_t st, ShapeParams sp, const FrontMapDev &fm, const int *parent_ij,
                   const double *parent_yaw, double *yaw_out, unsigned char *stage_out);
bool launch_k_astar(int shape, hipStream_t st, ShapeParams sp, const FrontMapDev &fm, const AstarDev &a, int slice);
bool launch_k_clr(int shape, unsigned grid, size_t lds, hipStream_t st, const ClrLaunch &a);
bool launch_k_pclr(int shape, unsigned grid, size_t lds, hipStream_t st, const PclrLaunch &a);
// shape-independent front-end kernels (svsdf_pipeline.hip)
void launch_k_pack_kernel_rows(hipStream_t st, const unsigned char *map, int ks, int count, unsigned long long *rows);
void launch_k_yaw_free(hipStream_t st, const unsigned long long *occ, int row_words, const unsigned long long *krows, int ks,
                       int count, int X, int Y, unsigned long long *free_out);

// per-slice entry points (defined by svsdf_shape_slice.hip, one set per slice)
#define SVSDF_DECLARE_SLICE(K)                                                                                              \
  bool launch_k_solve_s##K(int shape, int G, unsigned grid, unsigned block, size_t lds, hipStream_t st, const SolveLaunch &a); \
  bool launch_k_round_s##K(int shape, int lp, int mode, unsigned grid, size_t lds, hipStream_t st, const RoundLaunch &a);      \
  bool launch_k_classify_s##K(int shape, unsigned grid, size_t lds, hipStream_t st, const ClassifyLaunch &a);                  \
  bool launch_k_tail_s##K(int shape, int mode, unsigned grid, size_t lds, hipStream_t st, const TailLaunch &a);                \
  bool launch_k_rbound_s##K(int shape, unsigned grid, hipStream_t st, ShapeParams sp, double rmax, int nrad, int nang, double *out); \
  bool launch_k_subsw_s##K(int shape, dim3 grid, hipStream_t st, ShapeParams sp, const double *father, const double *child,    \
                           const unsigned long long *offs, const double *pts, const double *kt, int nkt, int *flag);         \
  bool launch_k_shape_kernels_s##K(int shape, unsigned grid, hipStream_t st, ShapeParams sp, int ks, int count, double resu,   \
                                   int size_side, double safemargin, const double *yaw, unsigned char *map);                   \
  bool launch_k_debug_sdf_at_s##K(int shape, unsigned grid, size_t lds, hipStream_t st, const TrajDev *traj, ShapeParams sp,    \
                                  const double *pxy, const double *t, int n, double *out, const ScaleDev *scl);                 \
  bool launch_k_succ_s##K(int shape, unsigned grid, hipStream_t st, ShapeParams sp, const FrontMapDev &fm,                      \
                          const int *parent_ij, const double *parent_yaw, double *yaw_out, unsigned char *stage_out);       \
  bool launch_k_astar_s##K(int shape, hipStream_t st, ShapeParams sp, const FrontMapDev &fm, const AstarDev &a, int slice);       \
  bool launch_k_clr_s##K(int shape, unsigned grid, size_t lds, hipStream_t st, const ClrLaunch &a);                            \
  bool launch_k_pclr_s##K(int shape, unsigned grid, size_t lds, hipStream_t st, const PclrLaunch &a);
SVSDF_DECLARE_SLICE(0)
SVSDF_DECLARE_SLICE(1)
SVSDF_DECLARE_SLICE(2)
SVSDF_DECLARE_SLICE(3)
#undef SVSDF_DECLARE_SLICE

}  // namespace svsdf
