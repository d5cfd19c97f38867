/* include/slam2d/karto_correct.h -- C-ABI of the MI355X Karto pose-correction stage (lesson6, config 5): the
 * per-scan refresh after SetSensorPose (LocalizedRangeScan::Update, Karto.h:5362-5416, reached from Mapper.cpp:1032
 * and :2044) and MapperGraph::CorrectPoses (Mapper.cpp:1397-1414, called from TryCloseLoop at :1038) for a fleet of
 * device-resident graphs WITHOUT the host: which scans and which graphs are meant is read from the records the
 * earlier stages left in device memory (kp_intake of karto_process.h, ke_job and ke_closure of karto_link.h), never
 * from a count on the host.  One kernel flattens the records into rows, and the row-indexed calls of the contexts
 * follow on the same stream:
 *
 *   kl_refresh_device        (karto_loop.h)  the scans' reference positions
 *   kt_refresh_device        (karto.h)       the scans' prepared points, in up to two matcher contexts
 *   spa_compute_rows_device  (spa.h)         SpaSolver::Compute for the graphs whose closure was accepted
 *   spa_export_poses_device  (spa.h)         CorrectPoses' loop: the optimised poses into the scan pool
 *
 * It replaces the per-graph loops over kl_set_scans_device, kt_set_scans_device, spa_compute_device and
 * spa_device_poses, whose graph, first scan and count are host integers.
 *
 * No call here synchronises with the host or copies, apart from the uploads of pending HOST edits in the contexts
 * it drives (kl_refresh_device, spa_compute_rows_device); only kc_get_info and kc_get_kernel_times wait.
 * Conventions as in karto_edit.h: plain C types, int status, kc_last_error().  A scan of graph g with state id `scan`
 * lives in pool slot pool_offset[g] + scan; the laser offset is identity, so the pool pose is the pose handed to
 * SetSensorPose.
 */
#ifndef SLAM2D_KARTO_CORRECT_H
#define SLAM2D_KARTO_CORRECT_H

#include <stddef.h>
#include <stdint.h>

#include "karto.h"
#include "karto_link.h"
#include "karto_loop.h"
#include "karto_process.h"
#include "spa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KC_OK 0
#define KC_EINVAL (-1)
#define KC_EHIP (-2)
#define KC_ENOMEM (-3)
#define KC_ENODEV (-4)
#define KC_ERANGE (-5) /* more records than the context's max_rows */

#define KC_MAX_ROWS 4096 /* KL_REFRESH_MAX_ROWS */

typedef struct kc_ctx kc_ctx;

const char *kc_version(void);
const char *kc_last_error(void);

/* A fleet of n_graphs graphs of up to max_scans scans; graph g's scan i is pool slot pool_offset[g] + i (host int
 * [n_graphs]; NULL: g * max_scans).  Scratch rows for max_rows (1 .. KC_MAX_ROWS) records per call. */
int kc_create(kc_ctx **out, int n_graphs, int max_scans, const int *pool_offset, int max_rows);
int kc_destroy(kc_ctx *ctx);

/* In the three calls below kl and either kt may be NULL (that context is then left alone); d_pool_ranges
 * double[pool_scans][n_readings] and d_pool_poses double[pool_scans][3] are the scan pool, which may be a matcher's
 * own (kt_pool_device: its refresh is then in place).  All work goes to hip_stream (NULL: the context's).
 * Launches per call: one kc_flatten_kernel and one kernel per context given.
 *
 * kc_refresh_intake_device: the scans the last intake accepted.  d_intake kp_intake[count] (kp_result_device),
 * record i of graph g_first + i; a record names its scan only with `accepted` set and status KP_OK. */
int kc_refresh_intake_device(kc_ctx *ctx, const kp_intake *d_intake, int g_first, int count, kl_ctx *kl, kt_ctx *kt_seq,
                             kt_ctx *kt_loop, const double *d_pool_ranges, const double *d_pool_poses, int pool_scans,
                             void *hip_stream);
/* kc_refresh_jobs_device: the scan of every job row (AddEdges' weighted mean, Mapper.cpp:2044); with d_closures
 * non-NULL only where d_closures[j].chain >= 0 (the fine pose write of TryCloseLoop, Mapper.cpp:1032).  The slot is
 * the job's own pool_offset + scan. */
int kc_refresh_jobs_device(kc_ctx *ctx, const ke_job *d_jobs, const ke_closure *d_closures, int count, kl_ctx *kl,
                           kt_ctx *kt_seq, kt_ctx *kt_loop, const double *d_pool_ranges, const double *d_pool_poses,
                           int pool_scans, void *hip_stream);
/* kc_correct_poses_device: CorrectPoses for the graphs of the job rows whose closure was accepted (chain >= 0, linked
 * or not: Mapper.cpp:1032-1038).  In order: the flatten; spa_compute_rows_device; spa_export_poses_device into
 * d_pool_poses by the context's pool_offset; kl_refresh_device over every scan of those graphs (rows {g, 0, -1,
 * pool_offset[g]}); kt_refresh_device on each matcher with the rows kl resolved.  spa may not be NULL; a matcher
 * needs kl (only the loop-search context knows the graphs' scan counts on the device). */
int kc_correct_poses_device(kc_ctx *ctx, const ke_job *d_jobs, const ke_closure *d_closures, int count, spa_ctx *spa,
                            const spa_params *params, kl_ctx *kl, kt_ctx *kt_seq, kt_ctx *kt_loop,
                            const double *d_pool_ranges, double *d_pool_poses, int pool_scans, void *hip_stream);

/* Totals since kc_create or the last call of this function: scans the refresh calls' records named, records whose
 * graph kc_correct_poses_device corrected, and records refused here (a graph >= n_graphs, a scan outside [0,
 * max_scans)).  What a context refuses it counts itself (kl_get_refresh_info, kt_get_refresh_info,
 * spa_get_rows_info).  Waits.  Any output may be NULL. */
int kc_get_info(kc_ctx *ctx, int *n_scans_refreshed, int *n_graphs_corrected, int *n_refused);

int kc_set_timing(kc_ctx *ctx, int enable);
/* Accumulated device time per kernel of THIS stage (the contexts time their own): names kc_kernel_name(i),
 * i < kc_num_kernels(). */
int kc_num_kernels(void);
const char *kc_kernel_name(int i);
int kc_get_kernel_times(kc_ctx *ctx, double *ms_out, int64_t *launches_out, int reset);

#ifdef __cplusplus
}
#endif

#endif
