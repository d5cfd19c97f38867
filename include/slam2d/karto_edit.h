/* include/slam2d/karto_edit.h -- C-ABI of the MI355X Karto graph-edit stage (lesson6, config 5): the AddVertex /
 * AddNode calls of Mapper::Process (Mapper.cpp:2053) and the AddEdge / AddConstraint calls of LinkScans
 * (Mapper.cpp:1104-1121) applied to the two device-resident pose graphs WITHOUT the host: the intake records of
 * karto_process.h (kp_result_device) and the link records of karto_link.h (ke_result_device) are flattened into
 * edit rows by one kernel and handed to kl_edit_*_device (karto_loop.h) and spa_edit_*_device (spa.h) on the same
 * stream.  It replaces kp_commit_vertices and ke_commit, which wait for the stage and copy its records back.
 *
 *   kd_commit_vertices_device   kp_plan_vertices' rule (csrc/karto_process_commit.h)
 *   kd_commit_edges_device      ke_plan_commit's rule (csrc/karto_link_commit.h)
 *
 * Differences from the host commits, both stated in karto_loop.h: a vertex whose expected id differs from the
 * graph's scan count is REFUSED (the host adds it and then reports the mismatch), and a refused row does not end
 * the commit -- the rows after it are still applied.  kd_get_info counts the refused rows.
 *
 * No call here synchronises with the host or copies unless a graph of kl or spa has pending host edits
 * (kl_edit_vertices_device).  Conventions as in karto_loop.h: plain C types, int status, kd_last_error().
 */
#ifndef SLAM2D_KARTO_EDIT_H
#define SLAM2D_KARTO_EDIT_H

#include <stddef.h>
#include <stdint.h>

#include "karto_link.h"
#include "karto_loop.h"
#include "karto_process.h"
#include "spa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KD_OK 0
#define KD_EINVAL (-1)
#define KD_EHIP (-2)
#define KD_ENOMEM (-3)
#define KD_ENODEV (-4)
#define KD_ERANGE (-5) /* more rows than the context's max_rows */

typedef struct kd_ctx kd_ctx;

const char *kd_version(void);
const char *kd_last_error(void);

/* Scratch for max_rows edit rows per call: count records for kd_commit_vertices_device, count * max_links link
 * records for kd_commit_edges_device. */
int kd_create(kd_ctx **out, int max_rows);
int kd_destroy(kd_ctx *ctx);

/* d_intake kp_intake[count] (kp_result_device): per record i with accepted set and status KP_OK, one vertex on
 * graph g_first + i with the expected id `scan`, and -- only where that vertex was added -- one node (id = scan,
 * pose = corrected) on the same graph of spa (spa may be NULL).  One flatten launch, kl_edit_vertices_device, a
 * tally launch, spa_edit_nodes_device, a tally launch; all on hip_stream (NULL: the context's). */
int kd_commit_vertices_device(kd_ctx *ctx, const kp_intake *d_intake, int g_first, int count, kl_ctx *kl,
                              spa_ctx *spa, void *hip_stream);

/* d_jobs_out / d_links / max_links are ke_result_device's.  Jobs [first_job, first_job + count) with status KE_OK
 * or KE_SINGULAR give, per record among their first min(n_links, max_links) with status KE_OK, in order, one edge
 * row (graph, from, to) and one constraint (from, to, diff, precision) that is applied only where the edge was
 * new: kl_edit_edges_device's is_new array is spa_edit_constraints_device's mask.  spa may be NULL. */
int kd_commit_edges_device(kd_ctx *ctx, const ke_job_out *d_jobs_out, const ke_link *d_links, int max_links,
                           int first_job, int count, kl_ctx *kl, spa_ctx *spa, void *hip_stream);

/* Totals since kd_create or the last call of this function: vertices added, new edges, rows refused by either
 * graph context.  Waits.  Any output may be NULL. */
int kd_get_info(kd_ctx *ctx, int *n_vertices, int *n_new_edges, int *n_refused);

int kd_set_timing(kd_ctx *ctx, int enable);
/* Accumulated device time per kernel of THIS stage (the graph contexts time their own: kl_get_kernel_times):
 * names kd_kernel_name(i), i < kd_num_kernels(). */
int kd_num_kernels(void);
const char *kd_kernel_name(int i);
int kd_get_kernel_times(kd_ctx *ctx, double *ms_out, int64_t *launches_out, int reset);

#ifdef __cplusplus
}
#endif

#endif
