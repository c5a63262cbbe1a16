/*
 * icp_engine.h — C-ABI of the ICP driver in libicp_hip.so: the drop-in for the reference's
 * engine API and CLI entry point, running the device path of icp_hip.h underneath.
 *
 * Reference interfaces these entry points replace:
 *   icp_params                ICPParameters            core/icpengine.h:13-19
 *   icp_iteration_record      IterationResult          core/icpengine.h:24-32
 *   icp_result                ICPResult                core/icpengine.h:37-44
 *   icp_engine_register       ICPEngine::setParameters + registerPointClouds (+ stop via the
 *                             stop flag, signals via hooks)   core/icpengine.h:60-75,
 *                             icpengine.cpp:24-66, :117-394
 *   icp_engine_register_devices  the same over several GPUs of one process
 *   icp_engine_run            the same loop on an existing (possibly multi-GPU) context
 *   icp_cli_icp               void ICP(PointCloud&, const PointCloud&, int, double,
 *                             double[3][3], double[3], vector<Matrix4d>*)
 *                             icp_registration.cpp:443-622
 *   icp_cli_icp_devices       the same over several GPUs of one process
 *   icp_best_fit_transform    computeBestFitTransform / best_fit_transform
 *                             icpengine.cpp:76-115, icp_registration.cpp:389-440 (host)
 *   icp_jacobi_svd3           Eigen::JacobiSVD<Matrix3d> as used at icpengine.cpp:93 (host)
 *
 * Points are AoS xyz doubles (the layout of std::vector<Point3D>, pointcloud.h:12-23).
 * Matrices are row-major. Return codes are those of icp_hip.h plus ICP_ENGINE_* below.
 */
#ifndef ICP_ENGINE_H
#define ICP_ENGINE_H

#include <stdint.h>

#include "icp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ICP_ENGINE_CANCELLED (-10)   /* stop() observed: finished(false, "用户取消")          */
#define ICP_ENGINE_TOO_FEW (-11)     /* valid pairs < 3: finished(false, "有效点对不足")       */

/* status of a finished run */
#define ICP_STATUS_MAX_ITERATIONS 0
#define ICP_STATUS_CONVERGED 1
#define ICP_STATUS_DIVERGED 2 /* rmse > 1.1 * previous (icpengine.cpp:311-314)          */
#define ICP_STATUS_TOO_FEW 3
#define ICP_STATUS_CANCELLED 4

/* flags */
#define ICP_FLAG_NO_EARLY_STOP 1 /* benchmark mode: never stop on convergence/divergence */

typedef struct icp_params {
  int32_t max_iterations;   /* 50     */
  double tolerance;         /* 1e-6   */
  double sigma_multiplier;  /* 3.0    */
  int32_t octree_max_points;/* 10     */
  int32_t octree_max_depth; /* 20     */
  int32_t rules;            /* ICP_RULES_ENGINE / ICP_RULES_CLI */
  int32_t flags;
} icp_params;

typedef struct icp_iteration_record {
  int32_t iteration;
  double rmse;
  int32_t valid_points;
  int32_t outlier_points;
  double transform[16];        /* cumulative, row-major */
  double rotation_angle_deg;   /* acos((tr-1)/2) in degrees (NaN-prone like the reference) */
  double translation_distance;
  int32_t has_transform;       /* 0 for the engine's convergence record (icpengine.cpp:293-301) */
  double mean, std, threshold;
  double increment[16];        /* this iteration's T (row-major) */
} icp_iteration_record;

typedef struct icp_result {
  int32_t success;
  int32_t status;
  int32_t total_iterations;
  double final_rmse;
  double final_R[9];
  double final_t[3];
  int32_t n_history;     /* records written (<= capacity) */
  char message[160];
} icp_result;

typedef struct icp_engine_hooks {
  void* user;
  void (*on_iteration)(void* user, const icp_iteration_record* rec); /* iterationCompleted  */
  void (*on_progress)(void* user, int iteration, int total, double rmse); /* progressUpdated */
  void (*on_log)(void* user, const char* message);                   /* logMessage          */
  const volatile int32_t* stop_flag; /* ICPEngine::stop(): checked once per iteration      */
} icp_engine_hooks;

void icp_params_default(icp_params* p);

/* Full registration on one GPU (device ordinal; -1 = the calling thread's current HIP device).
 * src is rewritten in place on success (engine rules) or always (CLI rules), as the reference. */
int icp_engine_register(const icp_params* p, double* src_xyz, int64_t n_src, const double* tgt_xyz,
                        int64_t n_tgt, int device, icp_result* res, icp_iteration_record* history,
                        int32_t history_cap, const icp_engine_hooks* hooks);

/* The same on several GPUs of this process (icp_hip_create_multi: the source sharded over the
 * devices, the octree replicated, RCCL all-gathers of the two per-iteration records when the ids
 * are distinct, an in-process host gather when they repeat). n_devices = 1 is icp_engine_register. */
int icp_engine_register_devices(const icp_params* p, double* src_xyz, int64_t n_src, const double* tgt_xyz,
                                int64_t n_tgt, int n_devices, const int* device_ids, icp_result* res,
                                icp_iteration_record* history, int32_t history_cap, const icp_engine_hooks* hooks);

/* The loop on a context that already holds target + this rank's source shard (icp_hip.h).
 * Every rank of a communicator calls it in lockstep; decisions are identical on all ranks.
 * The resident source is left transformed; fetch it with icp_hip_get_source. */
int icp_engine_run(icp_hip_ctx* ctx, const icp_params* p, icp_result* res, icp_iteration_record* history,
                   int32_t history_cap, const icp_engine_hooks* hooks);

/* Steppable form of the same loop (one call = one loop body of icpengine.cpp:159-368):
 * create on a ready context, step until *done != 0, then finish (applies the pending T and
 * fills the result). icp_engine_run == create + step* + finish. */
typedef struct icp_session icp_session;
int icp_session_create(icp_hip_ctx* ctx, const icp_params* p, const icp_engine_hooks* hooks, icp_session** out);
/* rec (optional) receives the record of this iteration when one is produced (*produced = 1). */
int icp_session_step(icp_session* s, icp_iteration_record* rec, int32_t* produced, int32_t* done);
/* Up to k steps in one call (no records returned; hooks still fire); stops early when the loop
 * is done. *steps_done = steps taken. Same as calling icp_session_step k times. */
int icp_session_step_n(icp_session* s, int32_t k, int32_t* steps_done, int32_t* done);
/* icp_session_step_n that also stores each step's host wall time (ms, steady clock; the step
 * returns when its record is on the host, so this is the whole iteration). step_ms[k]. */
int icp_session_step_n_timed(icp_session* s, int32_t k, int32_t* steps_done, int32_t* done, double* step_ms);
/* The error metric of a session's steps. ICP_METRIC_POINT (the default) is the reference's
 * point-to-point loop. ICP_METRIC_PLANE takes the same decisions from the same statistics
 * (convergence, divergence and too-few on the point-to-point RMSE, before the fit), but its
 * increment is the point-to-plane step: icp_hip_plane_sums about the iterate's centroid_src, then
 * icp_plane_solve; an iteration whose solve refuses takes the SVD step instead. A plane session
 * steps on the host (never the device-resident loop) and needs normals on the context
 * (ICP_HIP_ENOTREADY without them; ICP_HIP_EINVAL on a multi-device context or one with a
 * communicator). Call it before the first step: later it returns ICP_HIP_EINVAL.
 * ICP_METRIC_GICP is generalized ICP ("plane-to-plane", icp_hip.h): the same decisions again, the
 * increment from icp_hip_gicp_sums about the iterate's centroid_src with the context's epsilon
 * (icp_hip_set_gicp_epsilon) and R_src = the rotation of the session's cumulative transform before
 * the step, then icp_gicp_solve, and the SVD step when the solve refuses. It steps on the host and
 * needs normals of the target and of the source (ICP_HIP_ENOTREADY without either, and when the
 * resident source has been moved since its normals were made: they are in the frame of that
 * moment, which must be the session's start); ICP_HIP_EINVAL on a multi-device context or one with
 * a communicator. */
#define ICP_METRIC_POINT 0
#define ICP_METRIC_PLANE 1
#define ICP_METRIC_GICP 2
int icp_session_set_metric(icp_session* s, int32_t metric);
/* The last step of a plane session: its sums (zeros when the step computed none: a stop, or a
 * point session) and whether the plane solve gave the increment. Either output may be null. */
int icp_session_last_plane(const icp_session* s, icp_plane_sums* out, int32_t* used_plane);
/* The same for a generalized-ICP session. */
int icp_session_last_gicp(const icp_session* s, icp_gicp_sums* out, int32_t* used);
/* icp_engine_run with a metric. */
int icp_engine_run_metric(icp_hip_ctx* ctx, const icp_params* p, int32_t metric, icp_result* res,
                          icp_iteration_record* history, int32_t history_cap, const icp_engine_hooks* hooks);
/* The correspondence rejector of a session's steps. ICP_REJECT_SIGMA (the default) is the
 * reference's cull, d <= mean + k std: the session is then exactly what it is without this call.
 * With ICP_REJECT_TRIM (param = the fraction of the finite pairs kept, in (0, 1]) or
 * ICP_REJECT_MAX_DIST (param = the largest residual of a valid pair, > 0 and finite) a step
 *   1. runs icp_hip_iterate as every session does (and pays for its cull),
 *   2. takes its threshold t from icp_hip_residual_select(fraction, 0) (TRIM; 0 when no residual is
 *      finite) or from param (MAX_DIST),
 *   3. takes icp_hip_pair_sums(t), and
 *   4. takes the loop's decisions (convergence, divergence, too few) and the best fit from that
 *      call's rmse, valid, centroids and H in place of the cull's, by the same code.
 * With ICP_METRIC_PLANE a step that fits takes icp_hip_plane_sums_at(origin = the pair sums'
 * centroid_src, t), then icp_plane_solve, and the SVD increment when the solve refuses; with
 * ICP_METRIC_GICP icp_hip_gicp_sums_at and icp_gicp_solve in the same way. The record of
 * the iteration carries t as threshold, the rejector's valid_points, outlier_points and rmse, and the
 * iterate's own mean and std. Such a session steps on the host (never the device-resident loop).
 * Call it before the first step: later it returns ICP_HIP_EINVAL, as it does for another mode, a
 * param outside the mode's range, and for TRIM or MAX_DIST on a multi-device context or one with a
 * communicator. */
#define ICP_REJECT_SIGMA    0   /* the reference's cull: the default */
#define ICP_REJECT_TRIM     1   /* param = fraction kept, (0, 1] */
#define ICP_REJECT_MAX_DIST 2   /* param = largest residual of a valid pair, > 0, finite */
int icp_session_set_rejection(icp_session* s, int32_t mode, double param);
/* icp_engine_run with its options in a versioned record, so that the next option needs no entry
 * point of its own: set version = ICP_RUN_OPTIONS_VERSION (icp_run_options_default does); another
 * version is ICP_HIP_EINVAL. metric as icp_session_set_metric, reject and reject_param as
 * icp_session_set_rejection. The defaults give icp_engine_run. */
#define ICP_RUN_OPTIONS_VERSION 1u
typedef struct icp_run_options {
  uint32_t version;
  int32_t metric;       /* ICP_METRIC_* */
  int32_t reject;       /* ICP_REJECT_* */
  double reject_param;
} icp_run_options;
void icp_run_options_default(icp_run_options* opt);
int icp_engine_run_options(icp_hip_ctx* ctx, const icp_params* p, const icp_run_options* opt, icp_result* res,
                           icp_iteration_record* history, int32_t history_cap, const icp_engine_hooks* hooks);
int icp_session_finish(icp_session* s, icp_result* res);
/* Current cumulative transform (row-major 4x4). */
void icp_session_transform(const icp_session* s, double T_cum[16]);
void icp_session_destroy(icp_session* s);

/* CLI ICP(): octree 10/20, best init 1e20, threshold mean + 3 std, final R/t = the LAST
 * INCREMENTAL transform (icp_registration.cpp:616-621), cumulative transforms appended to
 * iteration_transforms (cap x 16, row-major) when non-null. */
int icp_cli_icp(double* src_xyz, int64_t n_src, const double* tgt_xyz, int64_t n_tgt, int max_iterations,
                double tolerance, double final_R[9], double final_t[3], double* iteration_transforms,
                int32_t cap, int32_t* n_transforms, int device);

/* icp_cli_icp on several GPUs of this process (as icp_engine_register_devices). */
int icp_cli_icp_devices(double* src_xyz, int64_t n_src, const double* tgt_xyz, int64_t n_tgt, int max_iterations,
                        double tolerance, double final_R[9], double final_t[3], double* iteration_transforms,
                        int32_t cap, int32_t* n_transforms, int n_devices, const int* device_ids);

/* Host helpers (no GPU needed). */
void icp_jacobi_svd3(const double H[9], double U[9], double S[3], double V[9]);
void icp_best_fit_transform(const double* a_xyz, const double* b_xyz, int64_t n, double T[16]);
void icp_best_fit_from_stats(const icp_iter_stats* st, double T[16]);
void icp_mat4_mul(const double A[16], const double B[16], double C[16]);

#ifdef __cplusplus
}
#endif
#endif
