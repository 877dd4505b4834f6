/*
 * svsdf_c.h -- C ABI of the MI355X-native SVSDF cost/gradient evaluator.
 *
 * Drop-in boundary for ONE hot path of ZJU-FAST-Lab/Implicit-SVSDF-Planner: the per-query-point
 * swept-volume-SDF safety penalty and its gradient evaluated inside the back-end optimizer's
 * cost callback.  Every entry point cites the reference interface it replaces; paths are
 * relative to the reference root, with
 *   BEO = src/planner_algorithm/include/planner_algorithm/back_end_optimizer.hpp
 *   SWM = src/swept_volume/include/swept_volume/sw_manager.hpp
 *   SHP = src/utils/include/utils/Shape.hpp
 *   MNC = src/utils/include/utils/minco.hpp
 *
 * Plain pointers and sizes only; no Eigen / torch / HIP types.  All matrices are COLUMN-major
 * exactly as the reference's Eigen objects store them.  One thread at a time per context (the
 * reference's LMBM driver is single-threaded and non-reentrant: src/utils/src/lmbm.cpp:4-6).
 *
 * The library needs a gfx950 device: every compute entry point returns a non-zero error code
 * (and svsdf_lmbm_evaluate returns +inf with g zeroed) when no HIP device is usable -- there is
 * no CPU fallback.
 */
#ifndef SVSDF_C_H
#define SVSDF_C_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Shape ids: registry order of SWM:187-235 (the reference keys the registry by the stem of
 * conf.inputdata, SWM:352-355), then the fallback Polygon (SWM:363-372). */
enum svsdf_shape_id {
  SVSDF_SHAPE_sdUnevenCapsule = 0,
  SVSDF_SHAPE_sdCutDisk = 1,
  SVSDF_SHAPE_sdTrapezoid = 2,
  SVSDF_SHAPE_sdRhombus = 3,
  SVSDF_SHAPE_star = 4,
  SVSDF_SHAPE_sdTunnel = 5,
  SVSDF_SHAPE_sdHorseshoe = 6,
  SVSDF_SHAPE_sdHeart = 7,
  SVSDF_SHAPE_sdOrientedVesica = 8,
  SVSDF_SHAPE_sdRoundedCross = 9,
  SVSDF_SHAPE_sdRoundedX = 10,
  SVSDF_SHAPE_bigX = 11,
  SVSDF_SHAPE_sdMoon = 12,
  SVSDF_SHAPE_sdPie = 13,
  SVSDF_SHAPE_sdPie2 = 14,
  SVSDF_SHAPE_sdArc = 15,
  SVSDF_SHAPE_Polygon = 16,
  SVSDF_SHAPE_COUNT = 17
};

#define SVSDF_MAX_PIECES 128       /* MINCO pieces per trajectory handled on the device (64 until round 5).  The reference has no
                                      cap (minco.hpp:433-513); what bounds a trajectory here beyond this is the LDS pose table: one pose
                                      per 0.15 s of duration (SWM:567), ~ 36 B each, in one block's share of the CU's 160 KB --
                                      SVSDF_ERR_INVALID "trajectory too long for the LDS pose table" otherwise */
#define SVSDF_MAX_POLY_VERTS 8190  /* Polygon outline vertices + one per loop of a multi-loop outline (the z = 0 outlines of
                                      the reference meshes have 77 ... 754) */
#define SVSDF_MAX_DEVICES 8        /* GPUs one context can drive (one xGMI node) */

/* Error codes (0 = ok).  HIP runtime errors are returned as SVSDF_ERR_HIP_BASE + hipError_t. */
enum svsdf_status {
  SVSDF_OK = 0,
  SVSDF_ERR_INVALID = 1,       /* bad argument (null ctx, N out of range, n != 4N-3, ...) */
  SVSDF_ERR_NO_DEVICE = 2,     /* no usable gfx950 device / HIP runtime unavailable */
  SVSDF_ERR_NO_POINTS = 3,     /* evaluate called before svsdf_set_points */
  SVSDF_ERR_NONFINITE = 4,     /* a non-finite value was produced on the device */
  SVSDF_ERR_RCCL = 5,          /* RCCL unavailable / failed (SVSDF_COMBINE_RCCL) */
  SVSDF_ERR_HIP_BASE = 1000
};

/* What the callee reads from TrajOptimizer / Config / SweptVolumeManager (BEO:50-95,
 * src/utils/include/utils/config.hpp:13-224). */
typedef struct svsdf_config {
  int shape_id;              /* enum svsdf_shape_id; see svsdf_shape_id_from_inputdata() */
  double poly_params[3];     /* Config::poly_params: shape offset x, y [m], yaw [deg]  SHP:281-294 */
  double safety_hor;         /* TrajOptimizer::safety_hor                              BEO:83 */
  double weight_p;           /* TrajOptimizer::weight_p                                BEO:77 */
  double rho;                /* TrajOptimizer::rho (time weight)                       BEO:48 */
  double head_state[9];      /* initState  3x3 col-major: col0 pos, col1 vel, col2 acc BEO:49 */
  double tail_state[9];      /* finalState 3x3 col-major                               BEO:50 */
  int device;                /* HIP device ordinal; -1 = current device */
  int polygon_nverts;        /* Polygon only: outline vertices (0 -> the 12 x 0.2 fallback  */
  const double *polygon_xy;  /*   rectangle of SWM:363-369); xy interleaved, copied.  For a mesh
                                (conf.inputdata = an .obj the shape registry does not know) pass
                                the outline svsdf_mesh_outline_obj() returns */
  int rank, world_size;      /* point sharding: this context keeps points k with
                                (sorted index k) % world_size == rank.  1 process per GPU. */
  int flags;                 /* SVSDF_FLAG_* */
  /* In-process multi-GPU (the reference is ONE process: the LMBM shim keeps its callback and instance in
   * file-static globals, src/utils/src/lmbm.cpp:4-6, and plan_manager.cpp:199 calls one optimizer): with
   * n_devices >= 2 the context drives devices[0..n_devices) from one host thread per device; device k keeps
   * stripe (rank * n_devices + k) of (world_size * n_devices) of the Morton order, every entry point fans the
   * evaluation out, sums the n_devices (19N+1)-double partials and synchronises before returning.
   * n_devices <= 1: the single device `device` (above).  A device may be listed more than once (several
   * stripes on one GPU; host combine only). */
  int n_devices;
  int devices[SVSDF_MAX_DEVICES];
  int combine;               /* SVSDF_COMBINE_*: how the per-device partials are summed */
  /* Polygon of several closed loops (a mesh section with a hole, two solids; svsdf_mesh_section): polygon_xy holds the
   * loops one after the other, polygon_loop_sizes[k] (>= 3) vertices each, summing to polygon_nverts.  The reference's
   * Polygon::getonlySDF (Shape.hpp:1448-1476) is the minimum of dis2Seg over all edges, negated on an odd count of
   * isCrossRayOnXDir over all edges: it does not care how the edges are chained, so the union of the loops' edges is
   * evaluated exactly like its single chain.  polygon_nloops <= 1 (or a NULL pointer): one loop, as the reference. */
  int polygon_nloops;
  const int *polygon_loop_sizes;
} svsdf_config;

#define SVSDF_COMBINE_AUTO 0 /* = HOST (measured: DESIGN.md "Multi-GPU") */
#define SVSDF_COMBINE_HOST 1 /* every device writes its partial to pinned host memory, fixed-order host sum */
#define SVSDF_COMBINE_RCCL 2 /* ncclAllReduce(ncclDouble, ncclSum) over an in-process communicator
                                (ncclCommInitAll), then one read-back; needs distinct devices */

#define SVSDF_FLAG_DEFAULT 0
#define SVSDF_FLAG_KEEP_INPUT_ORDER 1 /* do not Morton-sort the cloud at upload (debug) */
#define SVSDF_FLAG_HOST_ONLY 2        /* no device: only the host-side entry points work
                                         (svsdf_lmbm_prepare / svsdf_lmbm_finish, MINCO helpers);
                                         every device entry point fails with SVSDF_ERR_NO_DEVICE */

/* Piece-local time.  The reference subtracts the piece durations one after the other from t
 * (Trajectory::locatePieceIdx, trajectory.hpp:498-516).  Default (neither flag): the library does the same whenever
 * that can differ from t - (T_0+...+T_{i-1}) in a single subtraction, i.e. unless every duration is a coarse dyadic
 * number (multiple of 2^-20, like the 2.5 s of the BASELINE configs), in which case both forms are exact and equal and
 * the cheaper one runs.  svsdf_stats.piece_time_exact tells which form the last evaluation used. */
#define SVSDF_FLAG_EXACT_PIECE_TIME 4  /* always the reference's chain (O(piece index) per SDF evaluation) */
#define SVSDF_FLAG_FAST_PIECE_TIME 8   /* always the single subtraction: <= i ulp(t) away from the reference for generic
                                         durations, which flat stretches of SDF(t) amplify (differential fuzzing: gradient
                                         up to 5e-5 relative off, vs 1e-5 with the chain); round 1's behaviour */

/* Yaw kernels, and with them the whole front end, for a Polygon context (a given outline or the SWM:363-369 fallback
 * rectangle).  Without this flag svsdf_shape_kernels and svsdf_frontend_set_map refuse a Polygon: BasicShape::initShape
 * (Shape.hpp:386-430) calls getonlySDF(pos, Matrix3d), Polygon's two-argument overload takes a Matrix2d
 * (Shape.hpp:1477-1500), so the virtual call lands in the empty base body (Shape.hpp:267) and the reference's result is
 * undefined.  With it, cell (x, y) of yaw kernel k is occupied iff
 *   Polygon::getonlySDF((x c + y s, x (-s) + y c)) <= safemargin,   (s, c) = sincos(yaw_k):
 * the body of that overload (Shape.hpp:1484: the cell rotated by R_obj^T, then the same edge loop and the same crossing
 * parity as the one-argument form, Shape.hpp:1448-1476) with R_obj = the upper-left block of AngleAxisd(yaw_k, Z).  No
 * poly_params transform is applied, as in the one-argument form.  This is the reference's stated intent, not its
 * (undefined) behaviour.  Everything else is as for the analytic shapes: yaw table, generateByteKernel packing, the
 * limits of svsdf_frontend_set_map, stages 0 - 4, the A* ordering, slicing, counters.  On a context of any other shape
 * the flag is accepted and has no effect. */
#define SVSDF_FLAG_POLYGON_YAW_KERNELS 16
/* svsdf_min_clearance and svsdf_point_clearance under a scale schedule (svsdf_set_scale).  Without this flag the two entries
 * refuse a context with a schedule in force; with it they run the scaled search described with them (the bound of
 * svsdf_scale_bounds).  On a context without a schedule the flag changes nothing: the rigid search, the same kernels, the
 * same bits.  No other entry reads it. */
#define SVSDF_FLAG_SCALED_CLEARANCE 32

typedef struct svsdf_ctx svsdf_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* Replaces TrajOptimizer::setParam + SweptVolumeManager::init/initShape (SWM:339-374) for the
 * state this path reads.  Returns NULL on failure (see svsdf_last_error_string). */
svsdf_ctx *svsdf_create(const svsdf_config *cfg);
void svsdf_destroy(svsdf_ctx *ctx);
void svsdf_config_default(svsdf_config *cfg);
/* shape registry lookup as SWM:350-356 does it: stem of "shapes/star.obj" -> "star" -> id;
 * unknown stems give SVSDF_SHAPE_Polygon (the reference's fallback). */
/* Boundary states only (first lines of TrajOptimizer::optimize_traj_lmbm, back_end_optimizer.cpp:13-19):
 * keeps the context, the resident cloud, the launch plan and SweptVolumeManager's persistent
 * traj_duration (SWM:376-385) across optimisations. */
int svsdf_set_conditions(svsdf_ctx *ctx, const double head_state[9], const double tail_state[9]);
int svsdf_shape_id_from_inputdata(const char *inputdata);
const char *svsdf_shape_name(int shape_id);
const char *svsdf_last_error_string(const svsdf_ctx *ctx); /* ctx may be NULL */

/* ---- query points -------------------------------------------------------------------------- */
/* Replaces the fill of TrajOptimizer::parallel_points (src/plan_manager/src/plan_manager.cpp:
 * 168-175): P points, AoS xyz doubles (Eigen::Vector3d layout); z is ignored (BEO:790-791).
 * Copies; the cloud stays resident in HBM for all following evaluations. */
int svsdf_set_points(svsdf_ctx *ctx, const double *xyz_aos, size_t P);
/* Same, but xyz_aos is a DEVICE pointer on ctx's device (devices[0] of a multi-device context): inputs already
 * resident in HBM.  Both entry points plan the cloud on the device (bounding box -> Morton keys -> radix sort ->
 * gather of this context's stripe); svsdf_shard_plan below is the same plan computed on the host. */
int svsdf_set_points_device(svsdf_ctx *ctx, const double *d_xyz_aos, size_t P);
size_t svsdf_num_points(const svsdf_ctx *ctx);        /* points owned by this rank's shard */
/* Pure host: the original indices rank `rank` of `world_size` owns (Morton order, striped), in
 * the order the device stores them.  idx_out may be NULL to query the count. */
int svsdf_shard_plan(const double *xyz_aos, size_t P, int rank, int world_size, int flags,
                     long long *idx_out, size_t *count_out);

/* ---- the inner operator ---------------------------------------------------------------------- */
/* Replaces TrajOptimizer::addSaftyPenaOnSweptVolumeParallelTrueSDF (BEO:774-869):
 *   coeffs  : (6N) x 3 col-major, row 6i+k = coefficient of s^k of piece i (minco.getCoeffs())
 *   T       : N piece durations
 *   cost, gradT[N], gradC[(6N) x 3 col-major] are ACCUMULATED INTO (+=) like the reference.
 * Also performs SweptVolumeManager::updateTraj (SWM:376-385). Synchronises before returning. */
int svsdf_eval_penalty(svsdf_ctx *ctx, int N, const double *coeffs, const double *T,
                       double *cost, double *gradT, double *gradC);

/* Multi-process form (one process per GPU): leaves this rank's partial
 *   [ cost, gradC (18N, col-major), gradT (N) ]  = 19N + 1 doubles
 * in a device buffer owned by the context so the caller can all-reduce it in place (RCCL via
 * torch.distributed / ncclAllReduce), then hand it back to svsdf_accumulate_partial. */
int svsdf_eval_penalty_partial(svsdf_ctx *ctx, int N, const double *coeffs, const double *T,
                               double **d_partial, size_t *partial_len);
int svsdf_accumulate_partial(svsdf_ctx *ctx, int N, const double *partial_host,
                             double *cost, double *gradT, double *gradC);
/* Pure host: out[e] = partials[0][e] + partials[1][e] + ... in index order (the fixed-order sum the
 * multi-device context applies to its per-device partials; `partials` = G rows of `len` doubles). */
int svsdf_sum_partials(const double *partials, int G, size_t len, double *out);

/* ---- the full optimizer callback --------------------------------------------------------------- */
/* Same signature as lmbm_evaluate_t (src/utils/include/utils/lmbm.h:206-209); replaces
 * TrajOptimizer::costFunctionLmbmParallel (BEO:344-408) including MINCO forward/adjoint
 * (MNC:433-654) and the tau/xi maps (BEO:174-314).  x = [tau_0..tau_{N-1}, q_0(x,y,yaw), ...,
 * q_{N-2}], n = 4N - 3.  Returns the total cost and OVERWRITES g[0..n).  On a device error
 * returns +infinity with g zeroed (the reference has no error channel here). */
double svsdf_lmbm_evaluate(void *ctx, const double *x, double *g, const int n);
/* cost_pos, cost_other, cost_total of the last svsdf_lmbm_evaluate (BEO:396-398). */
int svsdf_last_costs(const svsdf_ctx *ctx, double costs3[3]);
/* Full callback split around the collective for the one-process-per-GPU form:
 * begin -> all-reduce the device partial -> finish. */
int svsdf_lmbm_begin(svsdf_ctx *ctx, const double *x, int n, double **d_partial, size_t *partial_len);
/* Host half of svsdf_lmbm_begin only: tau -> T, MINCO forward, energy partials (BEO:351-366);
 * writes the coefficients ((6N) x 3 col-major) and durations the device stage would receive. */
int svsdf_lmbm_prepare(svsdf_ctx *ctx, const double *x, int n, double *coeffs_out, double *T_out);
double svsdf_lmbm_finish(svsdf_ctx *ctx, const double *partial_host, double *g, int n);

/* ---- optimizer driver (host) ------------------------------------------------------- */
/* A limited-memory BFGS driver with the Lewis-Overton weak-Wolfe line search so that the callback can be
 * run end to end without the reference's Fortran LMBM (TrajOptimizer::optimize_traj_lmbm,
 * src/planner_algorithm/src/back_end_optimizer.cpp:3-95 -> lmbm::lmbm_optimize, src/utils/include/utils/lmbm.h:
 * 214-220).  Field names, defaults and status codes follow lbfgs_parameter_t / the LBFGS* enum of
 * src/utils/include/utils/lbfgs.hpp:33-160 (the solver the reference's mid end uses).  It is NOT the bundle
 * method: iterates differ from LMBM's, the objective and gradient it is fed are the same. */
typedef struct svsdf_lbfgs_params {
  int mem_size;           /* 8 */
  double g_epsilon;       /* 1e-5: stop when |g|_inf / max(1, |x|_inf) <= g_epsilon */
  int past;               /* 3 */
  double delta;           /* 1e-6: stop when the relative decrease over `past` iterations < delta */
  int max_iterations;     /* 0 = unlimited */
  int max_linesearch;     /* 64 */
  double min_step;        /* 1e-20 */
  double max_step;        /* 1e+20 */
  double f_dec_coeff;     /* 1e-4 */
  double s_curv_coeff;    /* 0.9 */
  double cautious_factor; /* 1e-6 */
  double machine_prec;    /* 1e-16 */
} svsdf_lbfgs_params;
enum svsdf_lbfgs_status {
  SVSDF_LBFGS_CONVERGENCE = 0, SVSDF_LBFGS_STOP = 1, SVSDF_LBFGS_CANCELED = 2,
  SVSDF_LBFGSERR_UNKNOWNERROR = -1024, SVSDF_LBFGSERR_INVALID_N, SVSDF_LBFGSERR_INVALID_MEMSIZE,
  SVSDF_LBFGSERR_INVALID_GEPSILON, SVSDF_LBFGSERR_INVALID_TESTPERIOD, SVSDF_LBFGSERR_INVALID_DELTA,
  SVSDF_LBFGSERR_INVALID_MINSTEP, SVSDF_LBFGSERR_INVALID_MAXSTEP, SVSDF_LBFGSERR_INVALID_FDECCOEFF,
  SVSDF_LBFGSERR_INVALID_SCURVCOEFF, SVSDF_LBFGSERR_INVALID_MACHINEPREC, SVSDF_LBFGSERR_INVALID_MAXLINESEARCH,
  SVSDF_LBFGSERR_INVALID_FUNCVAL, SVSDF_LBFGSERR_MINIMUMSTEP, SVSDF_LBFGSERR_MAXIMUMSTEP,
  SVSDF_LBFGSERR_MAXIMUMLINESEARCH, SVSDF_LBFGSERR_MAXIMUMITERATION, SVSDF_LBFGSERR_WIDTHTOOSMALL,
  SVSDF_LBFGSERR_INVALIDPARAMETERS, SVSDF_LBFGSERR_INCREASEGRADIENT
};
/* Same shape as lmbm_evaluate_t (lmbm.h:206-209): returns f(x), overwrites g[0..n). */
typedef double (*svsdf_evaluate_t)(void *instance, const double *x, double *g, const int n);
/* Called after every accepted iteration k (ls = evaluations of its line search); non-zero return cancels
 * (cf. lmbm_progress_t lmbm.h:211-213 and earlyExitLMBM, back_end_optimizer.hpp:1068-1085). */
typedef int (*svsdf_progress_t)(void *user, const double *x, const double *g, double fx, double step, int n,
                                int k, int ls);
void svsdf_lbfgs_params_default(svsdf_lbfgs_params *params);
/* Generic driver: minimise eval over R^n starting from x (in/out).  Returns a status of enum svsdf_lbfgs_status. */
int svsdf_lbfgs_minimize(int n, double *x, svsdf_evaluate_t eval, void *instance, svsdf_progress_t progress,
                         void *progress_user, const svsdf_lbfgs_params *params, double *final_cost,
                         int *iterations, int *evaluations);
/* optimize_traj_lmbm analogue: drives svsdf_lmbm_evaluate (points must be set) from x = [tau, q] in/out;
 * afterwards svsdf_lmbm_prepare(ctx, x, ...) gives the MINCO coefficients of the result (svsdf_last_costs
 * reflects the last callback evaluation, which is the returned point unless the final line search failed).  params may be NULL (defaults).  Returns a status of enum svsdf_lbfgs_status; values >= 0 mean a usable result. */
int svsdf_optimize_traj(svsdf_ctx *ctx, double *x, int n, const svsdf_lbfgs_params *params,
                        svsdf_progress_t progress, void *progress_user, double *final_cost, int *iterations,
                        int *evaluations);

/* ---- front-end consumers of the same shape SDFs (device) ------------------------- */
/* Replaces SweptVolumeManager::checkSubSWCollision (src/swept_volume/include/swept_volume/sw_manager.hpp:
 * 1171-1211), batched: the reference calls it once per A* edge from AstarPathSearcher::AstarGetSucc
 * (src/planner_algorithm/include/planner_algorithm/front_end_Astar.hpp:192-241) with the obstacle points of
 * getPointsInAABB2D around the child cell.  Edge e: father_states[3e..] / child_states[3e..] = (x, y, yaw),
 * obstacle points pts_xy[2*pts_offset[e] .. 2*pts_offset[e+1]) (pts_offset has n_edges+1 entries,
 * pts_offset[0] == 0).  free_out[e] = 1 where the reference returns true (no interpolated pose kt = 0,
 * 0.02, ..., <= 1 has sdf < 0 at any point), else 0.  Needs no trajectory and no svsdf_set_points. */
int svsdf_check_sub_sw_collision(svsdf_ctx *ctx, size_t n_edges, const double *father_states,
                                 const double *child_states, const size_t *pts_offset, const double *pts_xy,
                                 unsigned char *free_out);
/* Replaces BasicShape::initShape (src/utils/include/utils/Shape.hpp:386-430) + byteShapeKernel::
 * generateByteKernel (:194-216): per yaw index k (yaw_k from the reference's accumulated loop
 * `for (yaw = -PI; yaw < PI; yaw += 2*PI/kernel_count)`), cell (a, b) of the kernel_size^2 grid is occupied iff
 * getonlySDF((resu*a - side*resu, resu*b - side*resu), R(yaw_k)) <= safemargin
 * (safemargin = max(front_end_safeh, occupancy_resolution/2) at Shape.hpp:399).
 * map_out: kernel_count * kernel_size^2 bools [k][a][b]; bytes_out (may be NULL): kernel_count * kernel_size *
 * ((kernel_size+7)/8) bytes, bit (0x80 >> b%8) of byte [k][a][b/8]; yaw_out (may be NULL): kernel_count yaws;
 * loop_count (may be NULL): iterations the reference loop makes (kernel_count, or kernel_count+1 when
 * rounding lets the last yaw stay below PI -- the reference then writes past its arrays; only kernel_count
 * kernels are produced here).  Polygon -> SVSDF_ERR_INVALID (no such overload in the reference), unless the context
 * was created with SVSDF_FLAG_POLYGON_YAW_KERNELS (the definition is given there). */
int svsdf_shape_kernels(svsdf_ctx *ctx, int kernel_size, int kernel_count, double kernel_resolution,
                        double safemargin, unsigned char *map_out, unsigned char *bytes_out, double *yaw_out,
                        int *loop_count);

/* ---- query-point producer (host) ------------------------------------------------ */
/* Replaces, for the data this path consumes, PCSmapManager::rcvGlobalMapHandler
 * (src/map_manager/src/PCSmap_manager.cpp:88-210: cloud -> bounds -> occupancy grid with
 * `sta_threshold`) and the waypoint loop around getPointsInAABBOutOfLastOne
 * (src/plan_manager/src/plan_manager.cpp:156-175, PCSmap_manager.h:184-219).  xyz are float32
 * like pcl::PointXYZ.  svsdf_map_gather returns the occupied-voxel centres (deduplicated, ordered
 * by the reference's unified voxel id) ready for svsdf_set_points; out_xyz may be NULL to query
 * the count. */
typedef struct svsdf_map svsdf_map;
svsdf_map *svsdf_map_create(const float *xyz, size_t n, double resolution, int sta_threshold);
void svsdf_map_destroy(svsdf_map *map);
int svsdf_map_info(const svsdf_map *map, int dims[3], double bmin[3], double bmax[3], size_t *occupied);
int svsdf_map_gather(const svsdf_map *map, const double *centres_xyz, size_t ncentres, const double halfbd[3],
                     double *out_xyz, size_t capacity, size_t *count);
/* ASCII PCD v0.7, FIELDS x y z (src/plan_manager/pcds/map_*.pcd); xyz may be NULL to query n. */
int svsdf_pcd_read_ascii(const char *path, float *xyz, size_t capacity, size_t *n);

/* ---- query-point producer (device) ------------------------------------------------------------------- */
/* The same producer with the map resident on the device: cloud -> occupancy grid -> front-end bitmap -> waypoint-box
 * gather -> Morton-planned resident cloud, with no bulk data crossing back to the host.  Every step returns bit for bit
 * what svsdf_map_create / svsdf_map_info / svsdf_frontend_set_map / svsdf_map_gather + svsdf_set_points return.  The
 * resident map belongs to the context; a multi-device context keeps it on its first device, like the front end; a
 * SVSDF_FLAG_HOST_ONLY context returns SVSDF_ERR_NO_DEVICE from every entry that takes one.
 *
 * svsdf_map_build_device replaces PCSmapManager::rcvGlobalMapHandler (src/map_manager/src/PCSmap_manager.cpp:88-210) with
 * GridMap3D::createGridMap / isInMap / getGridIndex (src/map_manager/src/Gridmap3D.cpp:25-71, 137-177): bounds of the
 * float32 cloud widened to double, from +-999999999; dims = ceil((bmax - bmin) / resolution); a voxel is occupied when it
 * holds >= sta_threshold points.  xyz: n x 3 floats, in host memory (xyz_on_device = 0) or on the context's (first) device.
 * It replaces any earlier resident map; a front-end map set from the earlier one stays until the next set-map call.
 * n = 0 is accepted and reports what the host map reports (dims from the sentinel bounds, 0 cells); so is a flat cloud
 * (an axis with bmax == bmin: 0 cells).  SVSDF_ERR_INVALID with a message: a NaN or infinite coordinate (a deliberate
 * difference: the host builder casts floor(NaN) to int), a resolution that is not positive and finite, an axis or a product
 * X * Y * Z above 2^31 - 1 (the unified voxel id is an int), n >= 2^32. */
typedef struct svsdf_map_device_info {
  int struct_size;                 /* sizeof(svsdf_map_device_info), set by the caller */
  int dims[3];
  double bmin[3], bmax[3], resolution;
  int sta_threshold;
  size_t n_cloud, occupied, gathered;   /* gathered: points of the last svsdf_set_points_from_map */
  double build_ms, gather_ms;      /* host wall time of the two calls, synchronised */
} svsdf_map_device_info;
int svsdf_map_build_device(svsdf_ctx *ctx, const float *xyz, size_t n, int xyz_on_device, double resolution,
                           int sta_threshold);
int svsdf_map_device_get_info(const svsdf_ctx *ctx, svsdf_map_device_info *out);
/* The occupancy bytes, occ_out[(i * Y + j) * Z + k] (GridMap3D.h:129-130); capacity >= X * Y * Z. */
int svsdf_map_device_cells(const svsdf_ctx *ctx, unsigned char *occ_out, size_t capacity);
/* svsdf_frontend_set_map (below) from the resident map: layer k = 0 is packed into the inflated bitmap
 * (generateMapKernel2D, src/map_manager/include/map_manager/PCSmap_manager.h:81-108) on the device; everything after it is
 * the same code.  Same limits and messages, under this entry's name, plus "no resident map". */
int svsdf_frontend_set_map_device(svsdf_ctx *ctx, int kernel_size, int kernel_count, double safemargin);
/* Replaces the waypoint loop around getPointsInAABBOutOfLastOne (src/plan_manager/src/plan_manager.cpp:156-175,
 * PCSmap_manager.h:118-135, 184-219) with getGridCubeCenter / isIndexOccupied (Gridmap3D.cpp:184-195, 239-283), and the
 * svsdf_set_points that follows: the occupied voxels of every centre's box that lie outside the previous centre's box,
 * once each, ordered by unified voxel id, become the context's resident cloud through the planner of
 * svsdf_set_points_device (a multi-device context distributes its stripes as there).  "Original index"
 * (svsdf_shard_indices) is the position in that id-ordered list, exactly as after svsdf_map_gather + svsdf_set_points.
 * ncentres = 0 or an empty result gives a valid empty cloud; the launch plan is reset as by any svsdf_set_points;
 * svsdf_stats::setup_ms covers gather plus plan.  *count (may be NULL): the points gathered.  SVSDF_ERR_INVALID: no
 * resident map, a non-finite centre or half extent (the reference indexes with floor(NaN)).  On a map of zero cells the
 * result is empty (the host gather walks indices outside the grid there and returns (0, 0, 0) points). */
int svsdf_set_points_from_map(svsdf_ctx *ctx, const double *centres_xyz, size_t ncentres, const double halfbd[3],
                              size_t *count);
/* The id-ordered list of the last gather, i.e. what svsdf_map_gather returns; out_xyz may be NULL to query the count. */
int svsdf_map_device_points(const svsdf_ctx *ctx, double *out_xyz, size_t capacity, size_t *count);
/* The waypoint indices of generateTraj (plan_manager.cpp:132-140 and the loop header of :157); pure host, no context.
 * index_gap = ceil(traj_parlength / grid_resolution); while index_gap >= path_len - 1, traj_parlength /= 1.5 and again;
 * indices index_gap, 2 index_gap, ... < path_len - 1.  idx_out may be NULL to query the count; index_gap may be NULL.
 * The caller takes rows idx of the path (svsdf_astar_search's path_xyyaw: the z slot holds the yaw, as in the reference)
 * as the centres of svsdf_set_points_from_map.  SVSDF_ERR_INVALID for what the reference would not terminate on or would
 * misbehave on: path_len <= 2, traj_parlength <= 0, grid_resolution <= 0, non-finite values, capacity too small. */
int svsdf_path_waypoints(size_t path_len, double grid_resolution, double traj_parlength, size_t *idx_out,
                         size_t capacity, size_t *count, int *index_gap);

/* ---- front end: yaw-kernel free-space table and batched A* successor test (device) ---------- */
/* AstarPathSearcher::AstarGetSucc (src/planner_algorithm/include/planner_algorithm/front_end_Astar.hpp:192-241) tests
 * each of the 9 neighbours vi of a node in four steps: (1) isIndexValid(vi) && !isIndexOccupiedFlate(vi, 0)
 * (src/map_manager/src/Gridmap3D.cpp:73-133, 213-237); (2) checkKernelValue(father yaw, child yaw, vi)
 * (sw_manager.hpp:1158-1169), a breadth-first search over the yaw kernels around the father's yaw
 * (visit_kernels_by_distance, :1103-1156) that stops at the first kernel whose bit convolution kernelConv<true>
 * (:1033-1099) with the inflated map (generateMapKernel2D, src/map_manager/include/map_manager/PCSmap_manager.h:
 * 81-108) is empty -- that kernel decides the child's yaw; (3) getPointsInAABB2D(child centre, kernel_size/2+1,
 * kernel_size/2+1) (PCSmap_manager.h:137-158); (4) checkSubSWCollision(father, child, points) (sw_manager.hpp:
 * 1171-1211).  The entries below run all four on data resident on the device.
 *
 * svsdf_frontend_set_map: takes layer iz = 0 of the map's occupancy grid (what generateMapKernel2D and
 * getPointsInAABB2D read), builds the byte kernels of svsdf_shape_kernels on the device at the map's own resolution
 * (kernelConv overlays kernel cells on map cells one to one), and computes the yaw-free table: one 64-bit word per cell
 * (ix, iy), bit k set iff kernelConv<true>(k, (ix, iy, 0)) returns true -- the inflated map is (X + 2 side) x
 * (Y + 2 side) with side = (kernel_size - 1) / 2, the cell index itself is the box's minimum corner in it, outside the
 * map is free, and the bits the reference reads past a row only meet kernel columns >= kernel_size, which are zero.
 * The bitmap, the grid geometry and the table stay resident in the context until the next call or svsdf_destroy.
 * SVSDF_ERR_INVALID with a message: Polygon without SVSDF_FLAG_POLYGON_YAW_KERNELS (as in svsdf_shape_kernels), an even or non-positive kernel_size,
 * kernel_size > 63 or kernel_count > 64 (a kernel row and a cell's mask are one word each; the reference's yaml has
 * 17 and 18), a null or empty map.  A multi-device context uses its first device, like the other front-end entries. */
int svsdf_frontend_set_map(svsdf_ctx *ctx, const svsdf_map *map, int kernel_size, int kernel_count, double safemargin);
/* The yaw-free table, mask_out[ix * dims2[1] + iy]; mask_out may be NULL to query dims2 = {X, Y}. */
int svsdf_frontend_yaw_free(const svsdf_ctx *ctx, unsigned long long *mask_out, size_t capacity, int dims2[2]);
/* checkKernelValue + visit_kernels_by_distance (sw_manager.hpp:1103-1169) on one cell's word of the table; host only,
 * no context.  Returns 1 and writes *child_yaw, *kernel_index when a kernel is found, 0 when none (outputs untouched),
 * negative for a bad argument (outputs untouched).  The device code of svsdf_astar_successors calls the same function.
 * father_i = int(kernel_count * ((father_yaw + pi) / (2 * pi))) with pi = 3.1415926536 (sw_manager.hpp:20, not the PI
 * of the yaw table) truncates: fed the child yaws this function hands out it lands on i - 1 for some i (2 and 11 at 18
 * kernels).  An index outside [0, kernel_count) -- father_yaw >= pi, NaN, father_yaw <= -pi - 2 pi / kernel_count --
 * is an error (the reference indexes past its arrays).  Search order: pop, test, on failure push x - 1 then x + 1
 * (wrapped, unvisited only), give up after more than 10 pops: at most 11 kernels, s, s-1, s+1, ..., s-5, s+5.
 * child_yaw = 2 * pi * index / kernel_count - pi, evaluated left to right.  1 <= kernel_count <= 64. */
int svsdf_kernel_bfs(unsigned long long free_mask, int kernel_count, double father_yaw, double *child_yaw,
                     int *kernel_index);
/* The successor test of n nodes in one call: parent p = cell parent_ij[2p], parent_ij[2p+1] with yaw parent_yaw[p];
 * results at 9 p + 3 (i + 1) + (j + 1) for the neighbour (i, j), i and j from -1 to 1 (the reference's loop order,
 * centre included).  ok_out: 1 where the reference accepts the neighbour.  stage_out (may be NULL): 0 accepted,
 * 1 index invalid, 2 cell occupied, 3 no yaw kernel found, 4 sub-swept-volume collision.  child_yaw_out: the yaw
 * checkKernelValue chose, for stages 0 and 4; NaN elsewhere.  father = (centre of the parent cell, parent yaw), child =
 * (centre of the neighbour, chosen yaw), centres by getGridCubeCenter (Gridmap3D.cpp:184-195); obstacle points = centres
 * of the occupied layer-0 cells in the index box of getPointsInAABB2D, half extent kernel_size/2 + 1 METRES (integer
 * division, not scaled by the resolution).  SVSDF_ERR_INVALID: no map set, a parent outside the map or one whose yaw
 * svsdf_kernel_bfs rejects (the message names the first). */
int svsdf_astar_successors(svsdf_ctx *ctx, size_t n, const int *parent_ij, const double *parent_yaw,
                           unsigned char *ok_out, double *child_yaw_out, unsigned char *stage_out);

/* ---- front end: the A* search itself on the resident map (device) -------------------------------- */
/* Replaces AstarPathSearcher::AstarPathSearch + getPath (front_end_Astar.hpp:243-365, 367-390) and the per-search
 * AstarPathSearcher::reset (:154-163): the open-set loop runs on the device next to the map svsdf_frontend_set_map left
 * there, one workgroup per search, and every neighbour goes through the four stages of svsdf_astar_successors.
 *
 * Order: the reference's std::multimap<double, GridNode*> pops begin() -- the smallest fScore key and, among equal keys,
 * the entry inserted first.  The device pops the minimum over (key, insertion sequence number), which is that order.  A
 * node's key is the fScore it was inserted with: the id == 1 branch (:333-342) lowers gScore / fScore / father of an open
 * node but leaves its place in the queue, as in the reference.  A node's yaw is the one checkKernelValue handed out when
 * the node was first discovered (AstarGetSucc :231-234), whatever father it ends up with.  The start node is the
 * reference's separate startPtr (g = 0, yaw = start_yaw, no father); the map's own start cell only gets id = 1, g = 0,
 * f = h and never enters the queue.  The goal test is the index comparison at pop time, before expansion: start == goal
 * gives one cell and 0 expansions.  Edge cost sqrt(i*i + j*j); h = getHeu (:165-182) with dz = 0; no contraction.
 *
 * Slices: one launch makes at most `slice` pops and leaves the search state in device memory owned by the context; the
 * host relaunches until the status is final.  A pop is one removal from the open set: every expansion is one, and so is
 * the final pop that finds the goal; launches == ceil(pops / slice) with pops = expansions + (status == FOUND).  (An empty
 * open set and the expansion limit are noticed by the launch that made the last expansion.)  The result does not depend
 * on `slice`. */
typedef struct svsdf_astar_params {
  int struct_size;            /* sizeof(svsdf_astar_params) */
  double start_yaw;           /* yaw of the start node; the reference hard-codes 0.0 (front_end_Astar.hpp:281) */
  long long max_expansions;   /* stop with SVSDF_ASTAR_LIMIT after this many expansions; 0: no limit (the reference has none) */
  int slice;                  /* pops per launch; 0: the library's default (256) */
} svsdf_astar_params;
enum svsdf_astar_status {
  SVSDF_ASTAR_FOUND = 0,      /* the goal was popped (success_flag = true, :302-311) */
  SVSDF_ASTAR_EXHAUSTED = 1,  /* the open set ran empty (:360-361) */
  SVSDF_ASTAR_LIMIT = 2,      /* max_expansions expansions were made and the open set is not empty */
  SVSDF_ASTAR_OUT_OF_MAP = 3  /* isInMap (src/map_manager/src/Gridmap3D.cpp:43-71) fails for start or end (:249-254); no launch */
};
typedef struct svsdf_astar_result {
  int struct_size, status;    /* sizeof(svsdf_astar_result) (set by the caller), enum svsdf_astar_status */
  size_t path_len;            /* cells of the path, start and goal included; 0 unless FOUND */
  unsigned long long expansions;    /* calls of AstarGetSucc (:313) */
  unsigned long long pushes;        /* openSet.insert: the start node's (:283) and the neighbours' (:328, :354) */
  unsigned long long relaxed_open;  /* id == 1 updates (:335-340) */
  unsigned long long reopened;      /* id == -1 updates (:347-354); counted among the pushes too */
  unsigned long long launches;
  unsigned long long stage_counts[5];   /* successor slots by stage 0..4, as svsdf_astar_successors reports them */
  double g_goal;              /* gScore of the popped goal; 0 unless FOUND */
} svsdf_astar_result;
void svsdf_astar_params_default(svsdf_astar_params *p);
/* start_xyz / end_xyz: world points as AstarPathSearch(start, end) takes them; their cells by getGridIndex
 * (Gridmap3D.cpp:137-177).  path_xyyaw (3 doubles per cell: centre x, centre y, yaw -- what getPath returns; the start's
 * yaw is start_yaw) and path_ij (2 ints per cell) may each be NULL; with both NULL the call only reports path_len.
 * The search is planar in layer 0 like svsdf_astar_successors: a start or end whose z index is not 0 is
 * SVSDF_ERR_INVALID (the reference would stay in the start's layer and compare the goal's z index too; its demos have
 * z = 0).  SVSDF_ERR_INVALID also: no resident map, a wrong struct_size, a start_yaw svsdf_kernel_bfs rejects, slice < 0,
 * max_expansions < 0, and an output given with capacity_cells < path_len -- then *result is complete all the same and the
 * search state stays readable (svsdf_astar_nodes), so the call can be repeated with room.  A point outside the map is NOT
 * an error: SVSDF_OK with status SVSDF_ASTAR_OUT_OF_MAP.  Host-only contexts: SVSDF_ERR_NO_DEVICE.  A multi-device context
 * uses its first device.  The node records and the open set live in the context (sized at the first search on a map,
 * released with the map) and are reset at the start of every search (AstarPathSearcher::reset). */
int svsdf_astar_search(svsdf_ctx *ctx, const double start_xyz[3], const double end_xyz[3],
                       const svsdf_astar_params *params /* may be NULL */, double *path_xyyaw, int *path_ij,
                       size_t capacity_cells, svsdf_astar_result *result);
/* GridNodeMap as the last search left it (GridNode, front_end_Astar.hpp:10-51), [ix * Y + iy]: id (0 untouched, 1 open,
 * -1 closed), gScore, fScore, yaw, and the father as a cell ix * Y + iy (-1: none, -2: the start node).  Any pointer may be
 * NULL; with all NULL the call only reports dims2 = {X, Y}.  SVSDF_ERR_INVALID: no map, no search on this map yet,
 * capacity < X * Y. */
int svsdf_astar_nodes(const svsdf_ctx *ctx, signed char *id, double *g, double *f, double *yaw, int *father_cell,
                      size_t capacity, int dims2[2]);

/* ---- mesh shapes (host; BASELINE config 5: "arbitrary .obj mesh, no analytic shape SDF") ------------------------ */
/* The reference loads conf.inputdata with igl::read_triangle_mesh (src/utils/include/utils/Shape.hpp:281-313) and,
 * when the file's stem is not in its shape registry, plans with the generic Polygon shape over an outline
 * (sw_manager.hpp:350-372; the outline is hard-coded there).  Every query of the planar planner has z = 0
 * (BEO:790-791), so the part of a mesh it can see is the cross-section z = z0 = 0: these two entry points return that
 * outline (the longest closed loop; crossing points of the straddling triangles, chained through shared mesh edges) as
 * the xy-interleaved vertex list svsdf_config::polygon_xy takes.  xy_out may be NULL to query *count; loops (may be
 * NULL) receives the number of closed loops the section has (1 for one solid).
 * V: nv x 3 doubles, F: nf x 3 zero-based vertex indices.  The .obj reader takes `v` / `f` records (1-based or negative
 * indices, a/b/c forms, polygons fanned into triangles). */
int svsdf_mesh_outline(const double *V, size_t nv, const int *F, size_t nf, double z0, double *xy_out,
                       size_t capacity_verts, size_t *count, int *loops);
int svsdf_mesh_outline_obj(const char *obj_path, double z0, double *xy_out, size_t capacity_verts, size_t *count,
                           int *loops);
/* The whole section: every closed loop of z = z0, largest enclosed area first, as svsdf_config::polygon_xy /
 * polygon_loop_sizes / polygon_nloops take them (the planner then sees holes and separate solids, not just the largest
 * loop).  xy_out and loop_sizes may both be NULL to query the counts. */
int svsdf_mesh_section(const double *V, size_t nv, const int *F, size_t nf, double z0, double *xy_out, size_t capacity_verts,
                       size_t *n_verts, int *loop_sizes, size_t capacity_loops, size_t *n_loops);
int svsdf_mesh_section_obj(const char *obj_path, double z0, double *xy_out, size_t capacity_verts, size_t *n_verts,
                           int *loop_sizes, size_t capacity_loops, size_t *n_loops);

/* ---- swept-volume outline -------------------------------------------------------------------------------
 * What the reference's (unused) swept-volume surface extraction is for -- SweptVolumeManager::calculateSwept
 * (sw_manager.hpp:321-336) -> sw_calculate::calculation / getmesh (sw_calculate.cpp:4-305): a sparse-voxel continuation
 * with one serial gradient descent per voxel corner, then igl::marching_cubes; shown by vis->visMesh -- for this
 * planar planner: the boundary of the swept volume's z = 0 section, i.e. the zero set of the swept-volume implicit
 * function min over t of the shape SDF (getSDFofSweptVolume<false,true>, SWM:844-866: the hot path's argmin solve; the
 * reference's calculateSwept marches the same function, its scalarFunc SWM:1426-1446; the sign is the sign of the value
 * the optimizer is penalised with, SWM:921), as closed polylines with the inside on their left (outer boundaries
 * counter-clockwise, holes clockwise).  Batched on the GPU: a hierarchical narrow band
 * (coarse nodes first, then only cells whose four corners all lie within 1.5 cell diagonals of zero or change sign; cells across a found crossing are added until every chain closes) and marching
 * squares over the finest band cells of size `cell`; runs in a private context, the caller's resident cloud and launch
 * plan are untouched.  margin >= 0 widens the searched box (path bounding box + 2 shape bound radii + margin).
 * xy_out (interleaved, all loops one after the other) / loop_sizes (vertices per loop) may both be NULL to query the
 * counts.  stats (may be NULL): nodes evaluated vs what a dense grid of that cell size holds; open_chains > 0 means the
 * zero set left the searched box. */
typedef struct svsdf_outline_stats {
  unsigned long long nodes_evaluated, dense_nodes, cells_marched, batches;
  int open_chains;
} svsdf_outline_stats;
int svsdf_swept_outline(svsdf_ctx *ctx, int N, const double *coeffs, const double *T, double cell, double margin,
                        double *xy_out, size_t capacity_verts, size_t *n_verts, int *loop_sizes, size_t capacity_loops,
                        size_t *n_loops, svsdf_outline_stats *stats);

/* The mesh vis->visMesh("sweptmesh2D", ...) is given (SWM:331): the surface of the outline's extrusion over z in
 * [z0, z1] -- per loop of n vertices 2n mesh vertices (bottom ring, top ring) and 2n wall triangles with their normals
 * away from the inside; with caps != 0 also the bottom and top faces (every counter-clockwise loop triangulated with
 * the holes it contains, on the rings' own vertices): a closed, consistently oriented triangle surface like the
 * reference's marching-cubes output.  V_out: 3 doubles per vertex, F_out: 3 zero-based indices per triangle; both may
 * be NULL to query the counts.  Host only (no GPU). */
int svsdf_outline_extrude(const double *xy, const int *loop_sizes, size_t n_loops, double z0, double z1, int caps,
                          double *V_out, size_t capacity_verts, size_t *n_verts, int *F_out, size_t capacity_tris,
                          size_t *n_tris);

/* ---- certified minimum clearance (device) -----------------------------------------------------
 * A certified bracket lower <= c* <= upper on
 *   c* = min over p in the resident cloud, t in [0, sum T] of getSDFAtTimeStamp<false>(p, t)      (SWM:741-750),
 * the GLOBAL minimum over the whole cloud and the whole duration -- not the per-point local minimum the hot path's
 * argmin solve returns (svsdf_query_points: one basin per point, the one its seed fell into) and not the 51 sampled poses
 * of checkSubSWCollision (SWM:1171-1211).  With it a witness: sdf_at(point, t_witness) == upper, a value the device
 * evaluated, reproducible with svsdf_debug_sdf_at.  The search is a level-synchronous branch and bound over (point, time
 * interval) pairs on the device: [0, sum T] is cut into equal intervals at most 0.15 s wide; a pair of half width h
 * around m is bounded below by sdf_at(p, m) - h (V + W |p - x(m)|) with V, W the interval's svsdf_motion_bounds (the shape
 * SDF is 1-Lipschitz: svsdf_shape_selfcheck); a pair whose bound reaches upper - eps is settled, any other is halved.
 * Runs of 64 consecutive resident points are first tested as a whole by their bounding circle (tile_pairs /
 * tile_pairs_kept).  Results do not depend on pair_capacity, and two calls return identical structs except device_ms.
 * The call uploads the trajectory like svsdf_debug_sdf_at (same piece-time mode) and leaves the resident cloud, the
 * launch plan, svsdf_last_stats and the bits of every later evaluation as they were.  A multi-device context searches
 * every stripe on its own device; the host takes the smallest lower, the smallest upper with its witness (ties: the
 * smaller original index) and sums the counters (levels, device_ms: the largest).
 * Under a scale schedule (svsdf_set_scale) on a context created with SVSDF_FLAG_SCALED_CLEARANCE the value is
 * getSDFAtTimeStamp<true>(p, t) = sdf(u), u = R(t)^T S(t)^-1 (p - x(t)): the number the optimiser penalises against
 * safety_hor, and what svsdf_debug_sdf_at returns under the schedule (the witness reproduces with it bit for bit).  Its sign
 * is exact (p is inside the scaled robot at t iff the value is < 0); its magnitude is in SCALED BODY-FRAME units: for a
 * positive value v the world distance from p to the robot is at least (min_a (c_a - |A_a|)) * v.  The pair's bound is then
 *   sdf_sc(p, m) - h (V Imax + W |u(m)| + Q |p - x(m)|),   Imax, Q: the interval's svsdf_scale_bounds,
 * and the tile test divides the circle's distance to the pose by the interval's largest scale factor.  Everything
 * else -- intervals, levels, thresholds, budget, states, counters, the combination over devices -- is the rigid search's.
 * Returns SVSDF_ERR_NO_POINTS without a resident cloud, SVSDF_ERR_NO_DEVICE on a host-only context,
 * SVSDF_ERR_NONFINITE for a non-finite trajectory, SVSDF_ERR_INVALID with a message for a bad N, eps or struct_size, a
 * scale schedule in force on a context created without SVSDF_FLAG_SCALED_CLEARANCE (the bound is then the rigid one), a
 * total duration >= 300 s (the reference's stale-duration regime, SWM:376-385) and a context whose Lipschitz self-check
 * failed.  An empty resident cloud gives lower = upper = +infinity and point_index = -1. */
typedef struct svsdf_clearance_params {
  size_t struct_size;            /* sizeof(svsdf_clearance_params) */
  double eps;                    /* > 0, finite: converged when upper - lower <= eps (default 1e-3) */
  double target;                 /* NaN (default): none.  Otherwise the search stops after the first level at which
                                    lower >= target (SAFE) or upper < target (UNSAFE) */
  unsigned long long max_evals;  /* budget of SDF-at-time evaluations: a level that would exceed it is not started.
                                    0: 4 * P * ceil(sum T / 0.15).  Level 0 always runs.  A multi-device context gives
                                    every stripe its share by point count */
  size_t pair_capacity;          /* pairs one launch evaluates; a frontier buffer holds twice as many (every pair may
                                    split).  0: by cloud size.  Values below 64 (one tile) are raised to 64.  A larger
                                    frontier is processed in slices of the same level */
} svsdf_clearance_params;
enum { SVSDF_CLEARANCE_CONVERGED = 0, SVSDF_CLEARANCE_SAFE = 1, SVSDF_CLEARANCE_UNSAFE = 2, SVSDF_CLEARANCE_BUDGET = 3 };
typedef struct svsdf_clearance_result {
  int status, levels;            /* levels: levels evaluated, level 0 included */
  double lower, upper;           /* lower <= c* <= upper, always, whatever the status */
  double t_witness; long long point_index; double point_xy[2];   /* sdf_at(point, t_witness) == upper; index into the svsdf_set_points array */
  unsigned long long evals, pairs, tile_pairs, tile_pairs_kept;  /* SDF-at-time evaluations (the seed tile's included);
                                    (point, interval) pairs of levels >= 1; (tile, level-0 interval) pairs, and those
                                    the broad phase kept */
  double device_ms;              /* HIP-event time from the trajectory upload to the last level */
} svsdf_clearance_result;
void svsdf_clearance_params_default(svsdf_clearance_params *p);
int svsdf_min_clearance(svsdf_ctx *ctx, int N, const double *coeffs, const double *T,
                        const svsdf_clearance_params *params /* may be NULL */, svsdf_clearance_result *out);
/* The same question per point: for every point p of the svsdf_set_points array, in that array's order, a certified bracket
 *   lower[p] <= c_p <= upper[p],   c_p = min over t in [0, sum T] of getSDFAtTimeStamp<false>(p, t)      (SWM:741-750)
 * -- for an exterior point the swept-volume distance itself, for a colliding one how deep the collision is -- with
 * t_witness[p] the time of the evaluation the device made that gave upper[p] (svsdf_debug_sdf_at reproduces it bit for bit;
 * among all evaluations of p that attain upper[p], the one with the smallest t).  The search is svsdf_min_clearance's
 * (same intervals, same bound, same evaluations) with one running minimum per point instead of one: per-point values
 * U_p and settled bounds S_p live on the device as order-preserving integer keys of the doubles, lowered with integer
 * atomic minima (a minimum does not depend on arrival order: results are bit-reproducible), and a level settles a pair of
 * point p with bound lb iff lb >= min(U_p - eps, cap) -- under a target also iff lb >= target or U_p < target -- against
 * the U_p of before the level's first launch.  First every tile of 64 points is evaluated against the interval with its
 * smallest cheap bound (these count in evals); a (tile, interval) is kept iff its cheap bound is at most
 * min(cap, the tile's largest U_p).  state[p]:
 *   CONVERGED  upper - lower <= eps                    FAR     lower >= cap: not refined further
 *   SAFE       lower >= target                         UNSAFE  upper < target
 *   OPEN       max_evals or level 44 ended the search first; the bracket is valid all the same
 * (decided in the order UNSAFE, SAFE, FAR, CONVERGED).  lower, upper, t_witness, state: as many entries as the
 * svsdf_set_points array each, any may be NULL (a context with world_size > 1 writes the entries of its own shard only).
 * Results do not depend on pair_capacity; two calls return identical arrays and structs except device_ms.  Context state,
 * refusals (with this entry's name) and the empty cloud (counts of zero, lower = upper = +infinity, point_index = -1) are
 * svsdf_min_clearance's; in addition a NaN cap is SVSDF_ERR_INVALID.  A multi-device context searches every stripe on its
 * own device and scatters the stripes' points; its per-point brackets are valid but need not equal a single-device
 * context's bit for bit (the seed interval depends on the tile). */
typedef struct svsdf_point_clearance_params {
  size_t struct_size;            /* sizeof(svsdf_point_clearance_params) */
  double eps;                    /* > 0, finite (default 1e-3) */
  double cap;                    /* +infinity (default): none.  Clearance above cap is not refined */
  double target;                 /* NaN (default): none.  A point is finished once upper < target or lower >= target */
  unsigned long long max_evals;  /* as for svsdf_min_clearance; 0: 4 * P * ceil(sum T / 0.15).  The seed and level 0 always run */
  size_t pair_capacity;          /* as for svsdf_min_clearance */
} svsdf_point_clearance_params;
enum { SVSDF_POINT_CONVERGED = 0, SVSDF_POINT_FAR = 1, SVSDF_POINT_SAFE = 2, SVSDF_POINT_UNSAFE = 3, SVSDF_POINT_OPEN = 4,
       SVSDF_POINT_STATES = 5 };
typedef struct svsdf_point_clearance_result {
  int status, levels;            /* SVSDF_CLEARANCE_CONVERGED when no point is OPEN, else SVSDF_CLEARANCE_BUDGET */
  unsigned long long counts[SVSDF_POINT_STATES];   /* points in each state, indexed by SVSDF_POINT_* */
  double lower, upper;           /* the minimum over the points of lower[p], of upper[p] */
  double t_witness; long long point_index;         /* of that upper (ties: the smaller original index); -1: empty cloud */
  unsigned long long evals, pairs, tile_pairs, tile_pairs_kept;  /* as in svsdf_clearance_result; evals includes the seed's */
  double device_ms;              /* HIP-event time from the trajectory upload to the states */
} svsdf_point_clearance_result;
void svsdf_point_clearance_params_default(svsdf_point_clearance_params *p);
int svsdf_point_clearance(svsdf_ctx *ctx, int N, const double *coeffs, const double *T,
                          const svsdf_point_clearance_params *params /* may be NULL */, double *lower, double *upper,
                          double *t_witness, unsigned char *state, svsdf_point_clearance_result *out);
/* Host only, no context: rigorous bounds out2 = {max planar speed, max |yaw rate|} of the trajectory on
 * [ta, tb] intersected with [0, sum T] (coeffs, T as for svsdf_eval_penalty).  Per piece, the quartic velocity
 * polynomials restricted to the interval lie in the convex hull of their Bernstein coefficients (the bound of the exact
 * cull); the planar speed is the smaller of hypot(max |vx|, max |vy|) and the square root of the largest Bernstein
 * coefficient of the degree-8 polynomial vx^2 + vy^2.  Rounded up.  SVSDF_ERR_INVALID: N outside [1, SVSDF_MAX_PIECES],
 * tb < ta, a NaN bound of the interval, a non-positive duration; SVSDF_ERR_NONFINITE: a non-finite coefficient or duration. */
int svsdf_motion_bounds(int N, const double *coeffs, const double *T, double ta, double tb, double out2[2]);

/* ---- host-side MINCO helpers (MNC:397-655) ------------------------------------------------------- */
/* waypoints inPs: 3 x (N-1) col-major; out coeffs (6N) x 3 col-major. */
int svsdf_minco_coeffs(const double head_state[9], const double tail_state[9], int N,
                       const double *inPs, const double *T, double *coeffs);
void svsdf_forward_T(const double *tau, double *T, int N);   /* BEO:213-226 */
void svsdf_backward_T(const double *T, double *tau, int N);  /* BEO:228-241 */

/* ---- diagnostics ------------------------------------------------------------------------------------ */
/* Per-point results of getTrueSDFofSweptVolume<true> (SWM:916-1018) for the last trajectory
 * given to this context, in the ORIGINAL input order of this rank's shard: sdf[P], tstar[P],
 * grad_xy[2P] (any may be NULL).  Runs the device pipeline for (N, coeffs, T) first. */
int svsdf_query_points(svsdf_ctx *ctx, int N, const double *coeffs, const double *T,
                       double *sdf, double *tstar, double *grad_xy);
/* Work counters of the last evaluation. */
typedef struct svsdf_stats {
  unsigned long long points;          /* main queries in this shard */
  unsigned long long interior_points; /* points that entered the GSIP loop */
  unsigned long long solves;          /* argmin solves executed (main + selected GSIP samples) */
  unsigned long long gsip_samples;    /* GSIP circle samples emitted (the reference solves all of them) */
  unsigned long long sdf_evals;       /* SDF-at-time evaluations executed by the argmin kernel k_solve (layer-1 table
                                         evaluations + full evaluations: polynomial, sincos, transform, shape) */
  unsigned long long scan_evals;      /* of which layer-1 table evaluations (transform + shape only) */
  double device_ms;                   /* HIP-event time of the whole device pipeline (profiling on) */
  double solve_ms;                    /* HIP-event time during which >= 1 k_solve launch was executing (profiling on) */
  unsigned int solve_launches;        /* k_solve launches of the last evaluation */
  unsigned int gsip_iterations;       /* GSIP iterations that had work (rounds + supplementary) */
  unsigned long long culled_points;   /* main queries proven inactive (sdf > safety_hor) without a solve */
  int gsip_bound_mode;                /* 0 = cheap chunk bound, 1 = table scan of every GSIP sample, 2 = lazy: table scan of
                                         the samples within the selection band of the cheap bound only, 3 = anchor scans */
  int bound_mode_decided;             /* 1 once the mode is fixed for this point set (after <= 1 evaluation) */
  double bound_ratio;                 /* GSIP solves / samples of the deciding evaluation (rule: > 0.5 -> full) */
  int n_devices;                      /* devices that took part (1 unless svsdf_config::n_devices > 1) */
  int combine;                        /* SVSDF_COMBINE_* used by the last evaluation */
  double combine_ms;                  /* host wall time from "all devices done" to "summed partial on the host" */
  double setup_ms;                    /* host wall time of the last svsdf_set_points (sort + upload) */
  int piece_time_exact;               /* 0: single-subtraction piece-local time (exactly equivalent for this trajectory's
                                         durations, or forced by SVSDF_FLAG_FAST_PIECE_TIME); 1, 2: the reference's chain */
  double solve_ms_sum;                /* plain sum of the k_solve launch durations (solve_ms merges the intervals of
                                         launches that ran concurrently on different streams) (profiling on) */
  unsigned long long round_scan_evals; /* layer-1 table evaluations executed by k_round (seed scans of the GSIP samples
                                          in the scanning bound modes; transform + shape only); NOT part of sdf_evals */
  double round_ms;                    /* HIP-event time during which >= 1 k_round launch was executing (profiling on) */
  double round_ms_sum;                /* plain sum of the k_round launch durations (profiling on) */
  int batches;                        /* point batches (concurrent streams) the last evaluation ran as */
  unsigned long long speculative_evals; /* of sdf_evals: halving-ladder candidates evaluated BEHIND the accepted one (the
                                          lane group evaluates G candidates per step; the reference's sequential loop
                                          stops at the accepted one) */
  int plan_settled;                   /* 1 once bound mode, batch count and launch widths are fixed for this point set:
                                         the first evaluations after svsdf_set_points decide them (<= 6 evaluations, all
                                         with identical results); steady-state timing starts here */
  int tail_iter;                      /* GSIP iteration from which the fused tail kernel (k_tail: every remaining iteration of a
                                         batch in one launch, a half-wave owns a point until it is finished) took over; -1: none */
  unsigned int tail_launches;         /* k_tail launches of the last evaluation (one per batch) */
  unsigned long long tail_points;     /* GSIP points still active when the tail took over */
  double tail_ms;                     /* HIP-event time during which >= 1 k_tail launch was executing (profiling on) */
  double tail_ms_sum;                 /* plain sum of the k_tail launch durations (profiling on) */
  double shader_clock_mhz;            /* shader clock the evaluation ran at, measured by the kernel itself: cycles of the
                                         shader-clock counter (s_memtime) per cycle of the constant-rate counter (s_memrealtime,
                                         hipDeviceAttributeWallClockRate) over the life of the first wave of the main solve; a
                                         multi-device context reports its slowest device; 0 when nothing ran */
  double fanout_ms;                   /* multi-device contexts: host wall time of the evaluation that is neither a device's
                                         pipeline nor the combine -- waking the per-device threads (post -> the last thread
                                         starts) + joining them (the last thread done -> the caller runs again) */
} svsdf_stats;
int svsdf_last_stats(const svsdf_ctx *ctx, svsdf_stats *out);

/* Launch record of the last evaluation: which kernel instantiation every device launch of it ran, with what the launch
 * decided at run time.  Tests use it to prove which instantiation a configuration reaches instead of inferring it from
 * the size rules.  The library fills a fixed array per evaluation (no allocation); launches beyond
 * SVSDF_LAUNCH_REC_CAP are counted but not recorded. */
#define SVSDF_LAUNCH_REC_CAP 512
enum svsdf_kernel_kind {
  SVSDF_KERNEL_PREP = 0,      /* k_prep: pose table, chunk bounds and anchors */
  SVSDF_KERNEL_SOLVE = 1,     /* k_solve<shape, G>: argmin solves (main points or selected GSIP samples) */
  SVSDF_KERNEL_CLASSIFY = 2,  /* k_classify<shape>: exterior gradient / GSIP initialisation */
  SVSDF_KERNEL_ROUND = 3,     /* k_round<shape, LP, MODE>: one GSIP iteration of the launch chain */
  SVSDF_KERNEL_TAIL = 4,      /* k_tail<shape, MODE, WAVES>: every GSIP iteration from `iter` on */
  SVSDF_KERNEL_REDUCE = 5,    /* k_reduce: assembly of the per-point terms (+ final sum when `fused`) */
  SVSDF_KERNEL_FINAL = 6,     /* k_final: fixed-order sum of the block partials */
  SVSDF_KERNEL_FINISH = 7,    /* k_finish: suffix sum and counters */
  /* the scaled path (svsdf_set_scale): the launches that run S(t) arithmetic */
  SVSDF_KERNEL_SOLVE_SCALED = 8,     /* k_solve<shape, G, 1, ScaleDev>: rigid scan, scaled descent; G in {4, 8, 32} */
  SVSDF_KERNEL_CLASSIFY_SCALED = 9,  /* k_classify<shape, ScaleDev>: exterior gradient at the scaled body-frame point */
  SVSDF_KERNEL_REDUCE_SCALED = 10,   /* k_reduce<ScaleDev>: assembly with the position gradient under S(t*) */
  SVSDF_KERNEL_LAYER_TABLES = 11     /* k_layer_tables: pose tables of scan layers 2 / 3 (targ[0]: 2 or 3; only when the plan builds them) */
};
typedef struct svsdf_launch_rec {
  int struct_size;      /* bytes of this record the library wrote (see svsdf_last_launches) */
  int kernel;           /* svsdf_kernel_kind */
  int shape;            /* compiled shape id the kernel is specialised for: 0 ... 16, 17 = Polygon with its edges in LDS;
                           -1 for the shape-independent kernels */
  int targ[3];          /* template arguments: solve {G, 1, 0}; round {LP, MODE, 0}; tail {MODE, WAVES, 0}; else 0 */
  int iter;             /* solve: work index (0 main solve, i + 1 the samples of GSIP iteration i); round / tail: GSIP
                           iteration (tail: the first one); else 0 */
  int batch;            /* point batch (stream) of the launch; 0 for the main-stream kernels */
  int solo;             /* solve: one query per wave (fused pass) */
  int points_per_wave;  /* tail: points a wave owns (1 or 2) */
  int local_state;      /* tail: the GSIP state of the wave's points is kept in LDS */
  int duo;              /* tail: with one point per wave, both half-waves own it */
  int anchors;          /* round / tail: seed scans evaluate the anchors first */
  int fused;            /* reduce: one launch assembles and sums (no k_final / k_finish) */
  long long work;       /* queries (solve), points (round, tail, classify, reduce) the grid was sized for */
  unsigned int grid, block;
  unsigned long long lds_bytes;   /* dynamic LDS per block */
} svsdf_launch_rec;
/* Copies up to `cap` records of the last evaluation (svsdf_eval_penalty, svsdf_query_points, a callback, ...) into `out`
 * and sets *count to the number of launches that evaluation made -- more than SVSDF_LAUNCH_REC_CAP when some were not
 * recorded.  When cap > 0, out[0].struct_size must hold the caller's sizeof(svsdf_launch_rec): records are written with
 * that stride, each truncated to the smaller of the two sizes, so that the record can grow.  Single-device contexts only
 * (a multi-device context returns SVSDF_ERR_INVALID). */
int svsdf_last_launches(const svsdf_ctx *ctx, svsdf_launch_rec *out, int cap, int *count);

/* Time-varying robot scale: the reference's useScale path (sw_manager.hpp:17, getScale :495-503).  With a schedule set,
 * S(t) = diag(s_x(t), s_y(t), 1) with s_a(t) = c[a] + sin(omega[a] * t + phase[a]) * amp[a]  (a = 0: x, 1: y).
 * The reference's worked example  s_x = 0.8 + sin(1.5 t - 1.0) * 0.6,  s_y = sin(1.8 t) * 0.4 + 0.8  is
 * c = {0.8, 0.8}, amp = {0.6, 0.4}, omega = {1.5, 1.8}, phase = {-1.0, 0.0}, bit for bit; a constant scale is amp = 0.
 * What the reference computes with useScale = true, and so what the library computes under a schedule:
 *   - the seed scan (choiceTInit, all four layers) stays RIGID (sw_manager.hpp:567-570 call the rigid overloads);
 *   - the descent (gradientDescent) evaluates the shape SDF at u = (Rt^T S(t)^-1) (p - x(t));
 *   - the exterior gradient is the body-frame finite difference at that u at t*;
 *   - the assembly's position gradient is -L' (-(S^-1)^T R g) at S(t*); the yaw gradient keeps the rigid form
 *     (back_end_optimizer.hpp:1050, 1062).
 * getDotScale / the analytic time derivative are never read on this path (sw_manager.hpp:806).
 * Honoured by svsdf_eval_penalty(_partial), svsdf_lmbm_evaluate and the lmbm_* split, svsdf_query_points,
 * svsdf_optimize_traj, svsdf_swept_outline, svsdf_debug_sdf_at (the scaled value and body-frame point) and, on a context
 * created with SVSDF_FLAG_SCALED_CLEARANCE, svsdf_min_clearance and svsdf_point_clearance (without the flag they refuse a
 * schedule).  The front-end
 * entries (svsdf_check_sub_sw_collision, svsdf_shape_kernels) stay rigid, as in the reference.
 * The scaled path runs a reduced launch plan: solve widths 4 / 8 / 32, the launch chain only (no fused tail), no culls, and
 * every GSIP sample solved; svsdf_get_plan reports it.  The schedule belongs to the context: it survives svsdf_set_points /
 * svsdf_set_conditions and reaches every device of a multi-device context.
 * svsdf_set_scale(ctx, NULL) or enabled = 0 restores the rigid path.  SVSDF_ERR_INVALID with a message: struct_size is not
 * sizeof(svsdf_scale), a non-finite parameter, or c[a] - |amp[a]| <= 0 (s_a(t) could reach 0: S singular, the case the
 * reference warns about at sw_manager.hpp:493).  svsdf_get_scale needs out->struct_size = sizeof(svsdf_scale); with no
 * schedule it reports enabled = 0 and the identity (c = 1, amp = 0). */
typedef struct svsdf_scale {
  int struct_size;     /* sizeof(svsdf_scale) */
  int enabled;         /* 0: rigid (the same as NULL) */
  double c[2];         /* c_x, c_y */
  double amp[2];       /* A_x, A_y */
  double omega[2];     /* w_x, w_y (rad / s) */
  double phase[2];     /* phi_x, phi_y (rad) */
} svsdf_scale;
int svsdf_set_scale(svsdf_ctx *ctx, const svsdf_scale *scale);
int svsdf_get_scale(const svsdf_ctx *ctx, svsdf_scale *out);
/* Host only, no context (the companion of svsdf_motion_bounds for the certified clearance under a schedule): rigorous bounds
 *   out4 = { Smin = inf min_a s_a (rounded down), Smax = sup max_a s_a (rounded up),
 *            Imax = sup max_a 1 / s_a (rounded up), Q = sup max_a |s_a'| / s_a^2 (rounded up) }     over t in [ta, tb],
 * s_a' = A_a w_a cos(w_a t + phi_a).  The ranges of sin and |cos| over the argument interval [w_a ta + phi_a, w_a tb + phi_a]
 * (widened by its own rounding) come from its endpoints and the extrema it contains; an interval a period long gives the
 * full range.  NULL or enabled = 0 gives {1, 1, 1, 0}, and so does c = 1, amp = 0.  SVSDF_ERR_INVALID with a message: what
 * svsdf_set_scale refuses, tb < ta, a NaN or infinite bound of the interval, a null out4. */
int svsdf_scale_bounds(const svsdf_scale *scale, double ta, double tb, double out4[4]);

/* Launch plan of the resident point set.  Every field only moves TIME: each setting returns the same bits (cost, gradient
 * and per-point results).  By default everything follows deterministic rules: the first evaluation
 * after svsdf_set_points runs with the cheap GSIP bound and decides the bound mode from its counters, the batch count
 * follows from mode and shard size, the second evaluation records the launch widths; `settled` is 1 from then on.
 * svsdf_set_plan pins fields (the AUTO value leaves a field to its rule) for this and every later point set of the
 * context; svsdf_get_plan reports what is in force.  Multi-device contexts apply / report per device (get: device 0). */
#define SVSDF_PLAN_AUTO (-1)
typedef struct svsdf_plan {
  int bound_mode;       /* GSIP upper-bound mode: 0 cheap chunk bound, 1 table scan of every sample, 2 lazy, 3 anchor scans (every
                           third sample, the others only if their Lipschitz bound reaches the selection band); SVSDF_PLAN_AUTO */
  int batches;          /* concurrent point batches 1..8; SVSDF_PLAN_AUTO: by rule; -2: measured (three HIP-event timings
                           per candidate count, best median) */
  int lanes_per_query;  /* lanes of the main solve's lane groups: 1, 2, 4, 8, 16, 32; SVSDF_PLAN_AUTO: by shard size */
  int tail_iter;        /* GSIP iteration from which the fused tail kernel runs: >= 0; -2: never; SVSDF_PLAN_AUTO: by rule
                           (get under a scale schedule: -2, and lanes_per_query the scaled width 4 / 8 / 32) */
  int settled;          /* get only: 1 once nothing is left to decide for the resident point set */
  int layer_tables;     /* pose tables of scan layers 2 / 3 for the argmin solves: 0 none, 2 layer 2, 3 layers 2 and 3;
                           SVSDF_PLAN_AUTO: both when the previous evaluation's solve count pays for building them */
} svsdf_plan;
int svsdf_get_plan(const svsdf_ctx *ctx, svsdf_plan *out);
int svsdf_set_plan(svsdf_ctx *ctx, const svsdf_plan *plan);
/* In-process multi-device contexts (svsdf_config::n_devices >= 2, or 1 with SVSDF_COMBINE_RCCL): switch how the devices'
 * partials are summed -- SVSDF_COMBINE_HOST (fixed-order sum of the pinned partials) or SVSDF_COMBINE_RCCL (one
 * ncclAllReduce per device thread; the communicator is created on first use, distinct devices required).  Both give the
 * sum of the same G partials; the host form is bit-reproducible, RCCL's order is the library's.  Replaces, for this one
 * sum, what the reference does in its OpenMP critical section (back_end_optimizer.hpp:855-863). */
int svsdf_set_combine(svsdf_ctx *ctx, int combine);
/* Devices driven by the context, combine mode in force, and the rank count of the RCCL communicator as reported by the
 * communicator itself (ncclCommCount; 0 when none exists).  Any out pointer may be NULL. */
int svsdf_group_info(const svsdf_ctx *ctx, int *n_devices, int *combine, int *rccl_ranks);
/* One stripe of a multi-device context (k < n_devices; a single-device context has the one stripe 0): the device it lives
 * on, its point count, the counters / times of ITS part of the last evaluation and the launch plan it follows.  Any out
 * pointer may be NULL.  What an 8-GPU run is judged by -- stripe balance (device_ms max / mean), the plan every stripe
 * picked -- can so be read per stripe; with several stripes on one GPU (svsdf_config::devices repeating an ordinal)
 * svsdf_set_group_serial(ctx, 1) makes every stripe's device_ms its own. */
int svsdf_group_stripe(const svsdf_ctx *ctx, int k, int *device, size_t *points, svsdf_stats *stats, svsdf_plan *plan);
/* Diagnostic: serial != 0 runs the stripes' evaluations one after the other instead of concurrently (same results). */
int svsdf_set_group_serial(svsdf_ctx *ctx, int serial);
/* Shape bound used by the exact scan pruning and the exact cull: out2[0] = R with sdf_shape(q) >= |q| - R
 * (analytic circumradius of the shape + |offset|, Shape.hpp:281-294 / :531-1476), out2[1] = the largest
 * |q| - sdf_shape(q) found on a polar grid out to 60 m at context creation (self-check: <= out2[0]). */
int svsdf_shape_bound(const svsdf_ctx *ctx, double out2[2]);
/* The same two numbers plus out3[2] = the 1-Lipschitz self-check of the shape SDF taken on the same grid at context
 * creation: 0 when |sdf(q') - sdf(q)| <= |q' - q| held for every sampled pair (true of every exact distance function,
 * Shape.hpp:531-1476), otherwise the largest excess found -- the context then runs without the value-based second cull
 * and without the anchor GSIP bound mode, the two devices that rest on that property (same results, more work). */
int svsdf_shape_selfcheck(const svsdf_ctx *ctx, double out3[3]);
/* Per-launch HIP-event timing of the dominant (argmin solve) kernel on the library's own
 * streams; off by default (also env SVSDF_PROFILE=1).  Fills device_ms / solve_ms / solve_ms_sum.
 * enable = 2: additionally runs the point batches one after the other while profiling (a single batch), so that a
 * launch's duration is its own cost rather than stretched by the other batches' kernels it normally overlaps with;
 * enable = 0 restores the split.
 * enable = 3: device_ms only -- the span between the first and the last event of the evaluation, which are recorded
 * anyway; no per-launch events (they cost ~ 5 % of a 500 k-point evaluation), solve_ms / round_ms stay 0. */
int svsdf_set_profiling(svsdf_ctx *ctx, int enable);
/* Self-check: number of n equispaced arguments in [lo, hi] for which the kernels' inlined sincos
 * differs by even one bit from the ROCm device library's sincos (must be 0); -1 on error. */
long long svsdf_debug_sincos_mismatches(svsdf_ctx *ctx, double lo, double hi, int n);
/* Self-check: number of the n operands x for which the kernels' square root without range scaling differs by even one
 * bit from sqrt (must be 0); -1 on error.  flavour 0: the helper for radicands that are never zero, 1: the one that keeps
 * +0 on its fast path.  The helpers decide per wave of 64 consecutive operands: one operand outside [2^-767, inf) sends
 * its whole wave through sqrt itself, so a caller that wants the fast path exercised keeps such operands apart. */
long long svsdf_debug_sqrt_mismatches(svsdf_ctx *ctx, const double *x, size_t n, int flavour);
/* Test hook: device plus pinned allocations this library has made in this process and not yet freed, over all contexts;
 * *bytes (optional) their total size.  Every allocation goes through one owner type that counts; a context that has been
 * destroyed leaves the count where it was before svsdf_create. */
long long svsdf_debug_live_allocations(long long *bytes);
/* Diagnostic / test: getSDFAtTimeStamp<false> (sw_manager.hpp:741-750) of n (point, time) pairs on the device, through
 * the code the solve kernels inline.  points_xy: n x 2, t: n; out8: n x 8 = sdf, pose x, y, cos(yaw), sin(yaw), body-frame
 * x, y of the point, piece-time mode (0 cumulative, 1 / 2 the reference's chain).  Under a scale schedule
 * (svsdf_set_scale): getSDFAtTimeStamp<true>, the scaled sdf and the scaled body-frame point u.  The unit of work of the whole path:
 * tests compare it bit for bit with the oracle in device-arithmetic mode for every shape. */
int svsdf_debug_sdf_at(svsdf_ctx *ctx, int N, const double *coeffs_colmajor, const double *T, size_t n,
                       const double *points_xy, const double *t, double *out8);
/* Original indices (into the array given to svsdf_set_points) of this rank's shard, in the
 * order svsdf_query_points reports them. */
int svsdf_shard_indices(const svsdf_ctx *ctx, long long *idx_out);

#ifdef __cplusplus
}
#endif
#endif
