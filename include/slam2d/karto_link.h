/* include/slam2d/karto_link.h -- C-ABI of the MI355X Karto graph-linking stage (lesson6, config 5): the accept /
 * reject decisions, the constraints and the corrected pose of one Mapper::Process step, for a fleet of pose graphs,
 * from the device-resident results of the matcher (karto.h) and of the candidate search (karto_loop.h).
 *
 * Reference: open_karto's MapperGraph (lesson6/lib/open_karto/src/Mapper.cpp) and the node's SpaSolver.  Each entry
 * point replaces these reference members:
 *
 *   ke_add_edges_device    MapperGraph::AddEdges with one sensor per graph                   Mapper.cpp:902-973
 *                          LinkScans, LinkNearChains' response test, LinkChainToScan         Mapper.cpp:1104-1167
 *                          LinkInfo::Update                                                   Mapper.h:138-152
 *                          SpaSolver::AddConstraint's precision matrix                        spa_solver.cc:70-91
 *                          ComputeWeightedMean                                                Mapper.cpp:1288-1330
 *   ke_loop_coarse_device  TryCloseLoop's coarse test and its tmpScan                         Mapper.cpp:1003-1012
 *   ke_loop_fine_device    TryCloseLoop's fine test, pScan->SetSensorPose(bestPose)           Mapper.cpp:1023-1032
 *   ke_close_device        LinkChainToScan(candidateChain, pScan, bestPose, covariance)       Mapper.cpp:1035
 *   ke_commit              AddEdge's rIsNewEdge deciding LinkScans' AddConstraint             Mapper.cpp:1107-1120
 *
 * Out of scope (the caller keeps them): HasMovedEnough and the running-scan buffer (the caller names the running
 * scans' chain to kl_closest_device; karto_process.h decides both on the device and writes the ke_job rows and that
 * chain); the first-scan linking to other sensors (Mapper.cpp:924-954: one sensor per
 * graph); AddVertex / AddNode (the caller's, before AddEdges, as in Mapper::Process); graph edits on the device (the
 * graphs of kl_ctx and spa_ctx are host-mirrored: ke_commit edits them on the host from small fixed-size records).
 * Parity with the compiled library is UNPINNED as for karto_loop.h (open_karto needs boost): the results equal the
 * CPU restatement tests/ref/karto_link_ref.c bit for bit, and that restatement equals a literal transcription of the
 * reference members (tests/ref/karto_link_plain.py).
 *
 * ARITHMETIC.  IEEE double, no FMA contraction; sin / cos / atan2 are csrc/detmath.h's sdm_sin / sdm_cos / sdm_atan2.
 * Every operation is written as the reference writes it, left to right:
 *
 *   Matrix3::FromAxisAngle(0, 0, 1, r), literally (Karto.h:2392-2421): with c = cos r, s = sin r, m = 1.0 - c
 *       [0][0] = 0*0*m + c        [0][1] = 0*0*m - 1*s      [0][2] = 0*1*m + 0*s
 *       [1][0] = 0*0*m + 1*s      [1][1] = 0*0*m + c        [1][2] = 0*1*m - 0*s
 *       [2][0] = 0*1*m - 0*s      [2][1] = 0*1*m + 0*s      [2][2] = 1*1*m + c
 *     so [2][2] = (1 - c) + c, which is not 1.0 in general, and the zero entries carry the signs these expressions
 *     give them.
 *   Matrix3::Inverse (Karto.h:2445-2493): the cofactors i of InverseFast, fDet = m00*i00 + m01*i10 + m02*i20, then
 *     every entry multiplied by 1.0 / fDet.  Where the reference asserts, fabs(fDet) <= 1e-14, and for a NaN
 *     determinant, this library refuses: !(fabs(fDet) > 1e-14) is KE_SINGULAR.
 *   math::NormalizeAngle (Math.h:182-210) as written, its two while loops and the (kt_int32u) casts of
 *     angle / -KT_2PI and angle / KT_2PI included.  The reference does not terminate, or casts out of range, for a
 *     non-finite angle or one of 2^32 rad and more: such an angle gives NaN here.
 *   LinkInfo::Update (Mapper.h:138-152): diff = Transform(pose1, Pose2()).TransformPose(pose2), with SetTransform's
 *     three branches (Karto.h:2909-2935): pose1 == Pose2() exactly (identity rotation, zero transform); pose1 at the
 *     origin position (the transform's position is Pose2()'s); the general case, position Pose2() - R * pose1 with
 *     R = FromAxisAngle(0, 0, 1, 0.0 - h1) and Matrix3 * Pose2 (Karto.h:2574-2583).  TransformPose (Karto.h:2881-2887)
 *     is transform + R * pose2 for the position and NormalizeAngle(h2 + (0.0 - h1)) for the heading.
 *     The covariance is (R1 * cov) * R1.Transpose() with R1 = FromAxisAngle(0, 0, 1, -h1) and Matrix3::operator*
 *     (Karto.h:2552-2567): each entry a[r][0]*b[0][c] + a[r][1]*b[1][c] + a[r][2]*b[2][c].
 *   SpaSolver::AddConstraint (spa_solver.cc:70-91): precision = Inverse() of that covariance, then its upper
 *     triangle copied over the lower.
 *   ComputeWeightedMean (Mapper.cpp:1288-1330): the inverses in list order; sumOfInverses summed entry by entry in
 *     list order from the zero matrix; inverted; per item weight = invSum * inverse_i, accumulated += weight * pose_i
 *     with Pose2::operator+= (Karto.h:2117-2121: the position added, the heading NormalizeAngle(h + h_i)) from
 *     Pose2(); thetaX += cos, thetaY += sin in list order from 0.0, each divided by (double)n; the heading is
 *     atan2(thetaY, thetaX).
 *
 * Conventions as in karto_loop.h: plain C types, int status (KE_OK / negative), ke_last_error().  A pose is
 * double[3] = x, y, heading (rad); a matrix is row-major double[9].  Every device array an entry point takes is
 * read with its indices checked against the sizes the call names; an index out of range gives KE_EINVAL in the
 * job's (or the call's info) status and is never followed.
 */
#ifndef SLAM2D_KARTO_LINK_H
#define SLAM2D_KARTO_LINK_H

#include <stddef.h>
#include <stdint.h>

#include "karto.h"      /* kt_result */
#include "karto_loop.h" /* kl_closest, kl_source, kl_near_chain, kl_loop_chain, kl_ctx */
#include "spa.h"        /* spa_ctx */

#ifdef __cplusplus
extern "C" {
#endif

#define KE_OK 0
#define KE_EINVAL (-1)
#define KE_EHIP (-2)
#define KE_ENOMEM (-3)
#define KE_ENODEV (-4)
#define KE_ERANGE (-5)   /* a job needs more than the context's max_links link records: nothing of it is written */
#define KE_SINGULAR (-6) /* Matrix3::Inverse would have asserted (or the determinant is NaN) */

#define KE_MAX_LINKS 64

/* ke_link.kind */
#define KE_PREV 0    /* LinkScans(previous scan, scan, scanPose, rCovariance)                  Mapper.cpp:915 */
#define KE_RUNNING 1 /* LinkChainToScan(running scans, scan, scanPose, rCovariance)            Mapper.cpp:962 */
#define KE_NEAR 2    /* LinkChainToScan(near chain, scan, mean, covariance)                    Mapper.cpp:1146 */
#define KE_LOOP 3    /* LinkChainToScan(candidateChain, scan, bestPose, covariance)            Mapper.cpp:1035 */

#define KE_WRITE_POSE 1 /* flags bit 0: also write the new pose into the pool pose array at the scan's slot */

/* ke_get_loop_info status bits */
#define KE_LOOP_OVERFLOW 1 /* more accepted matches than capacity (or base scans than base_capacity): the first kept */
#define KE_LOOP_EINVAL 2   /* a match with an index out of range was met: it is not accepted */

typedef struct ke_params {
    double link_match_minimum_response_fine;   /* Mapper default 0.8 (Mapper.cpp:1517-1564) | mapper_params.yaml 0.1 */
    double loop_match_minimum_response_coarse; /* 0.8 | 0.35 */
    double loop_match_maximum_variance_coarse; /* 0.4^2 | 3^2: the value Mapper stores, the SQUARE of the ROS
                                                  parameter (Mapper.cpp:1871-1874) */
    double loop_match_minimum_response_fine;   /* 0.8 | 0.45 */
} ke_params;

/* One AddEdges call.  The scan is scan `scan` of graph `graph`, pool slot pool_offset + scan; a from-scan f of the
 * same graph is pool slot pool_offset + f.  prev: the previous scan's index, or -1 for a graph's first scan.
 * seq_result: the index of its sequential match in d_seq (rCovariance; read only when prev >= 0).  running: the
 * index in d_running of the kl_closest of its running scans, or -1 (read only when prev >= 0: the running scans are
 * linked in AddEdges' else branch, Mapper.cpp:955-963).  Its near matches are
 * [near_first, near_first + near_count) of the near batch.  ke_close_device reads graph, scan and pool_offset. */
typedef struct ke_job {
    int graph, scan, pool_offset, prev, seq_result, running, near_first, near_count;
} ke_job;

/* status KE_OK: diff = LinkInfo's pose difference, precision = AddConstraint's matrix.  status KE_SINGULAR: the
 * rotated covariance has no inverse; diff and precision are all +0.0 and ke_commit skips the record. */
typedef struct ke_link {
    int from, to, kind, status;
    double diff[3];
    double precision[9];
} ke_link;

/* status KE_OK; KE_SINGULAR (an inverse of ComputeWeightedMean is singular: pose is the unchanged pose and the pool
 * is not written; the link records are emitted all the same); KE_ERANGE (more than max_links records needed);
 * KE_EINVAL (an index of the job out of range).  With KE_ERANGE and KE_EINVAL n_links = n_means = 0, no link record
 * and no pool pose is written, and pose is the unchanged pose (+0.0 when the scan's own slot is out of range).
 * n_links counts the job's records, the KE_SINGULAR ones included.  pose: the weighted mean, or the unchanged pose
 * when the mean list is empty (n_means = 0). */
typedef struct ke_job_out {
    int n_links, n_means, status, graph;
    double pose[3];
} ke_job_out;

/* chain: the slot's first chain, in chain order, that was accepted coarse and not rejected fine, or -1 (pose and
 * covariance are then +0.0, resume and fine -1); resume: that chain's kl_loop_chain.resume; fine: the fine match.
 *
 * After an accepted closure the reference moves every pose (CorrectPoses, Mapper.cpp:1038), so the slot's later
 * chains are stale: the caller commits the closure, runs the optimiser, refreshes the scans and queries again with
 * kl_query.start_num = resume, which is what start_num is for. */
typedef struct ke_closure {
    int chain, resume, fine, pad_;
    double pose[3];
    double covariance[9];
} ke_closure;

typedef struct ke_ctx ke_ctx;

const char *ke_version(void);
const char *ke_last_error(void);
/* Mapper::InitializeParameters defaults (0.8, 0.8, 0.4 * 0.4, 0.8) | the node's mapper_params.yaml (0.1, 0.35,
 * 3.0 * 3.0, 0.45) */
void ke_default_params(ke_params *params);
void ke_node_params(ke_params *params);

/* Link rows for max_jobs jobs of at most max_links (1 .. KE_MAX_LINKS) records each, scans of n_readings (1 ..
 * 4096) readings, and loop batches of at most max_matches coarse matches.  params NULL means ke_default_params;
 * link_match_minimum_response_fine - KL_TOLERANCE is computed here, once, in double. */
int ke_create(ke_ctx **out, const ke_params *params, int n_readings, int max_jobs, int max_links, int max_matches);
int ke_destroy(ke_ctx *ctx);

/* STAGE 1.  AddEdges for `count` (<= max_jobs) jobs, one wave each, one launch, no host synchronisation.
 *
 * d_pool_poses double[pool_scans][3]: the layout of kt_pool_device / spa_device_poses; the scan's own sensor pose
 * and every from-scan's.  d_seq kt_result[n_seq]: the sequential matches.  d_running kl_closest[n_running] (NULL
 * with n_running 0).  d_near kt_result[n_near] with d_near_source kl_source[n_near], the near batch of
 * kl_emit_batch_device(KL_NEAR_CHAINS) and its matches; d_near_chains and chain_stride from kl_result_device;
 * n_slots: the search slots d_near_chains holds (d_near_source[].slot < n_slots).
 *
 * Job j writes link row j (ke_link[max_links]) and ke_job_out j, in the reference's call order:
 *   KE_PREV     when prev >= 0: LinkScans(prev, scan, scanPose, rCov);
 *   KE_RUNNING  when prev >= 0, running >= 0 and d_running[running].linked: LinkScans(closest, scan, scanPose, rCov);
 *   KE_NEAR     for each near match in order with response > link_min - KL_TOLERANCE (Mapper.cpp:1141): its mean
 *               and covariance join the mean list, and if its chain has KL_CHAIN_LINKED the record is
 *               LinkScans(chain.closest, scan, mean, cov).
 * The mean list is [scanPose, rCov] when prev >= 0, then the accepted near matches.  With KE_WRITE_POSE the
 * weighted mean is also written to d_pool_poses at the scan's slot (the caller's next kt_set_scans_device /
 * kl_set_scans_device sees it without a copy); d_pool_poses is then written, otherwise only read.  Two jobs of one
 * launch must not name the same scan, nor one the other's from-scan, when KE_WRITE_POSE is set.
 * This stage is latency-bound: a few hundred dependent double operations per job. */
int ke_add_edges_device(ke_ctx *ctx, int count, const ke_job *d_jobs, double *d_pool_poses, int pool_scans,
                        const kt_result *d_seq, int n_seq, const kl_closest *d_running, int n_running,
                        const kt_result *d_near, const kl_source *d_near_source, int n_near,
                        const kl_near_chain *d_near_chains, int chain_stride, int n_slots, int flags,
                        void *hip_stream);

/* STAGE 2, coarse.  Over the coarse results d_coarse[m], m < min(*d_n_matches, max_matches), of the batch
 * kl_emit_batch_device(KL_LOOP_CHAINS) produced (d_query, d_base_begin, d_base_index as emitted): match m is
 * accepted when response > min_coarse && covariance[0] < max_var && covariance[4] < max_var (Mapper.cpp:1003-1005).
 * The accepted matches are compacted, order kept, into kt_match_batch_device's arrays for the fine match: fine
 * match f has d_fine_query[f] = tmp_first + f, base list d_fine_base_index[d_fine_base_begin[f] ..
 * d_fine_base_begin[f + 1]) = the chain's base list, and d_fine_of[f] = m.  Row f of d_tmp_ranges
 * double[capacity][n_readings] and d_tmp_poses double[capacity][3] holds the query scan's ranges (read from
 * d_pool_ranges double[pool_scans][n_readings] at d_query[m]) and the coarse mean: tmpScan.SetSensorPose(bestPose).
 * Rows f >= the fine count hold +inf ranges and a +0.0 pose, so the caller passes all `capacity` rows to
 * kt_set_scans_device(first = tmp_first).  *d_n_fine (device, one int) is the fine count.
 * Sizes: d_fine_query int[capacity], d_fine_base_begin int[capacity + 1], d_fine_of int[capacity],
 * d_fine_base_index int[base_capacity].  More accepted matches than capacity, or more base scans than
 * base_capacity, sets KE_LOOP_OVERFLOW (ke_get_loop_info) and keeps the first matches that fit.
 * Two launches, no host synchronisation. */
int ke_loop_coarse_device(ke_ctx *ctx, int max_matches, const int *d_n_matches, const kt_result *d_coarse,
                          const int *d_query, const int *d_base_begin, const int *d_base_index,
                          const double *d_pool_ranges, int pool_scans, int tmp_first, int capacity,
                          int base_capacity, int *d_fine_query, int *d_fine_base_begin, int *d_fine_base_index,
                          int *d_fine_of, int *d_n_fine, double *d_tmp_ranges, double *d_tmp_poses,
                          void *hip_stream);
/* The last coarse call's accepted count before the capacity cut, and its status bits (waits for it). */
int ke_get_loop_info(ke_ctx *ctx, int *total_accepted, int *status);

/* STAGE 2, fine.  For each of the `count` search slots: the first fine match f < min(*d_n_fine, capacity), in
 * order, whose coarse match d_fine_of[f] has d_source[].slot == the slot and whose fine result is not rejected.
 * The reference rejects when fineResponse < min_fine (Mapper.cpp:1023), so a match is accepted when
 * !(response < min_fine): a NaN response is accepted.  d_source kl_source[max_matches] is the coarse batch's (its
 * matches are ordered by slot, as kl_emit_batch_device emits them); d_loop_chains and chain_stride from
 * kl_result_device.  d_closures ke_closure[count].  With KE_WRITE_POSE the accepted pose is written to
 * d_pool_poses at the query scan's pool slot d_query[m] (pScan->SetSensorPose(bestPose)); d_query and d_pool_poses
 * may be NULL without the flag.  One launch, stream-ordered. */
int ke_loop_fine_device(ke_ctx *ctx, int count, int capacity, const int *d_n_fine, const kt_result *d_fine,
                        const int *d_fine_of, int max_matches, const kl_source *d_source, const int *d_query,
                        const kl_loop_chain *d_loop_chains, int chain_stride, ke_closure *d_closures,
                        double *d_pool_poses, int pool_scans, int flags, void *hip_stream);

/* STAGE 3.  Slot s (job row s; d_jobs[s] names graph, scan and pool_offset) with d_closures[s].chain >= 0 and
 * d_closest[s].linked set emits one KE_LOOP record LinkInfo(closest's sensor pose, closure pose, covariance), from
 * = d_closest[s].closest; d_closest is what kl_closest_device gave for the accepted chain after the scan was
 * refreshed at its new pose.  ke_job_out s: n_links 0 or 1, n_means 0, pose = the closure's pose (the scan's pool
 * pose when there is no closure).  One launch, stream-ordered. */
int ke_close_device(ke_ctx *ctx, int count, const ke_job *d_jobs, const ke_closure *d_closures,
                    const kl_closest *d_closest, const double *d_pool_poses, int pool_scans, void *hip_stream);

/* The link rows and job outputs of the last stage-1 or stage-3 call: rows [first_job, first_job + count) copied to
 * links_out ke_link[count][max_links] and jobs_out ke_job_out[count] (either may be NULL; waits for the stage).
 * Only the first n_links records of a row are defined. */
int ke_get_links(ke_ctx *ctx, int first_job, int count, ke_link *links_out, ke_job_out *jobs_out);
/* The same on the device: ke_link[max_jobs][max_links], ke_job_out[max_jobs]; any output may be NULL. */
int ke_result_device(ke_ctx *ctx, const ke_link **d_links, const ke_job_out **d_jobs_out, int *max_links);

/* HOST COMMIT.  Waits for the stage, copies rows [first_job, first_job + count) back and, per job with status
 * KE_OK or KE_SINGULAR, per record in order with status KE_OK, calls kl_add_edge(graph, from, to, &is_new) and,
 * only when the edge is new, spa_add_constraint(graph, from, to, diff, precision, NULL), as LinkScans does
 * (Mapper.cpp:1107-1120): the spa ids are the scan indices.  The common duplicate, the running chain's closest scan
 * being the previous scan, therefore adds one edge and one constraint.  spa may be NULL (edges only).
 * *n_new_edges (may be NULL) counts the new edges.  It adds no vertex and no node.  The first failing call ends the
 * commit with KE_EINVAL and its message; the edits before it stay. */
int ke_commit(ke_ctx *ctx, kl_ctx *kl, spa_ctx *spa, int first_job, int count, int *n_new_edges);

int ke_set_timing(ke_ctx *ctx, int enable);
/* Accumulated device time per kernel: names ke_kernel_name(i), i < ke_num_kernels(). */
int ke_num_kernels(void);
const char *ke_kernel_name(int i);
int ke_get_kernel_times(ke_ctx *ctx, double *ms_out, int64_t *launches_out, int reset);

#ifdef __cplusplus
}
#endif

#endif
