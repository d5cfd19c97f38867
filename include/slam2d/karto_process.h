/* include/slam2d/karto_process.h -- C-ABI of the MI355X Karto scan-intake stage (lesson6, config 5): what
 * Mapper::Process does before and between the device stages of karto.h, karto_loop.h and karto_link.h, for a fleet
 * of pose graphs with one sensor each: is this scan used, which scans is it matched against, and every array that
 * joins the stages.
 *
 * Reference: open_karto's Mapper and the node (lesson6/lib/open_karto, lesson6/src).  Each entry point replaces these
 * reference members:
 *
 *   kp_intake_device       the odometry carry, Transform(lastOdom, lastCorrected).TransformPose   Mapper.cpp:2021-2025
 *                          Mapper::HasMovedEnough                                                 Mapper.cpp:2087-2120
 *                          the node's readings loop with its inverted-laser reversal              karto_slam.cc:415-434
 *                          SetOdometricPose / SetCorrectedPose of a new scan                      karto_slam.cc:439-440
 *   kp_apply_match_device  pScan->SetSensorPose(bestPose)                                         Mapper.cpp:2044
 *                          the pose SpaSolver::AddNode reads                                      spa_solver.cc:63-68
 *   kp_commit_vertices     AddVertex / AddNode                                                    Mapper.cpp:2053
 *   kp_advance_device      ScanManager::AddRunningScan with its trim loop                         Mapper.h:1365-1386
 *                          SetLastScan                                                            Mapper.cpp:2073
 *
 * Out of scope: a laser offset other than identity (as in every other Karto header); more than one sensor per
 * graph; LaserRangeFinder::Validate (the reading count is the context's); tf and the map -> odom transform (the
 * advance record holds GetCorrectedPose(), which the node feeds to it); graph edits on the device (vertices go
 * through kp_commit_vertices, as edges go through ke_commit); a call that chains every stage.
 * Parity with the compiled library is UNPINNED as for karto_link.h: the results equal the CPU restatement
 * tests/ref/karto_process_ref.c bit for bit, and that restatement equals a literal transcription of the reference
 * members (tests/ref/karto_process_plain.py).
 *
 * MODEL.  A graph's scan i lives in pool slot pool_offset[g] + i of caller-owned arrays double[pool_scans][n_readings]
 * (ranges) and double[pool_scans][3] (sensor poses): the layouts of kt_pool_device and spa_device_poses.  With the
 * identity offset a scan's pool pose is its GetSensorPose().  Per graph the context keeps on the device: n_scans, the
 * last scan's odometric pose and time, and the running scans as (run_begin, run_length): with one sensor they are
 * always a contiguous tail of the graph's scans, because AddRunningScan pushes at the back and erases at the front.
 *
 * ARITHMETIC.  IEEE double, no FMA contraction; sin / cos / atan2 are csrc/detmath.h's.  NormalizeAngle,
 * FromAxisAngle and Matrix3 * Pose2 are the statements of karto_link.h (ARITHMETIC there; a non-finite angle
 * normalises to NaN).  On top of them, literally:
 *
 *   Transform(p1, p2) (SetTransform, Karto.h:2909-2935): p1 == p2 exactly gives the identity rotation and the zero
 *     transform; otherwise R = FromAxisAngle(0, 0, 1, h2 - h1) and the position is p2 - R * p1 (Pose2::operator-,
 *     its heading normalised and then dropped) when p1.x != 0 || p1.y != 0, else p2's; the transform's heading is
 *     h2 - h1.  TransformPose(s) (Karto.h:2881-2887) is transform + R * s (Pose2::operator+) for the position and
 *     NormalizeAngle(s.h + transform.h) for the heading.
 *   GetSensorAt(p) (Karto.h:5310-5313) = Transform(Pose2(), p).TransformPose(Pose2()).
 *   SetSensorPose(s) (Karto.h:5289-5300) with the offset Pose2(): offsetLength = sqrt(0*0 + 0*0), angleoffset =
 *     atan2(0, 0), correctedHeading = NormalizeAngle(s.h), worldSensorOffset = (offsetLength * cos(correctedHeading +
 *     angleoffset - 0), offsetLength * sin(the same), 0), corrected = s - worldSensorOffset (Pose2::operator-).
 *   HasMovedEnough (Mapper.cpp:2087-2120): time - lastTime >= minimum_time_interval; else with both sensor poses
 *     GetSensorAt(odometric pose): fabs(NormalizeAngle(h - lastH)) >= minimum_travel_heading; else
 *     Square(lastX - x) + Square(lastY - y) >= Square(minimum_travel_distance) - KT_TOLERANCE.  A NaN never passes >=.
 *   AddRunningScan (Mapper.h:1365-1386): push, then erase the front while size > scan_buffer_size || d2(front,
 *     back) > Square(scan_buffer_maximum_scan_distance) - KT_TOLERANCE, d2 = Square(fx - bx) + Square(fy - by) over
 *     the CURRENT pool poses.  Strict >: a NaN distance keeps the scan.
 *
 * Conventions as in karto_link.h: plain C types, int status (KP_OK / negative), kp_last_error().  Every device array
 * an entry point takes is read with its indices checked against the sizes the call names.
 */
#ifndef SLAM2D_KARTO_PROCESS_H
#define SLAM2D_KARTO_PROCESS_H

#include <stddef.h>
#include <stdint.h>

#include "karto.h"      /* kt_result */
#include "karto_link.h" /* ke_job */
#include "karto_loop.h" /* kl_query, kl_closest_item, kl_source, kl_ctx, KL_MAX_SCANS */
#include "spa.h"        /* spa_ctx */

#ifdef __cplusplus
extern "C" {
#endif

#define KP_OK 0
#define KP_EINVAL (-1)
#define KP_EHIP (-2)
#define KP_ENOMEM (-3)
#define KP_ENODEV (-4)
#define KP_ERANGE (-5) /* kp_intake.status: the graph already holds max_scans scans */

typedef struct kp_params {
    double minimum_time_interval;             /* Mapper default 3600 (Mapper.cpp:1468-1515) | mapper_params.yaml 3600 */
    double minimum_travel_distance;           /* 0.2 | 0.2 */
    double minimum_travel_heading;            /* DegreesToRadians(10) | 0.174 */
    double scan_buffer_maximum_scan_distance; /* 20 | 100 */
    int scan_buffer_size;                     /* 70 | 110 */
    int inverted;                             /* 0: the node's lasers_inverted_ for this fleet's laser */
} kp_params;

/* One graph's candidate scan of a round.  row indexes d_ranges_f32 float[n_rows][n_readings] (the LaserScan's
 * ranges); row < 0: no scan for this graph this round.  odom: the odometric pose getOdomPose gave. */
typedef struct kp_candidate {
    int row;
    int pad_;
    double time;
    double odom[3];
} kp_candidate;

/* What kp_intake_device decided for candidate i (graph g_first + i), completed by kp_apply_match_device.
 * status: KP_OK; KP_EINVAL (row >= n_rows, or the scan's pool slot >= pool_scans); KP_ERANGE (the graph is full).
 *   A candidate with a status other than KP_OK is not accepted and never truncated.
 * accepted: 1 when the scan enters the graph.  An absent candidate (row < 0) has status KP_OK, accepted 0, prev -1
 *   and +0.0 poses; a rejected one (HasMovedEnough false) has status KP_OK, accepted 0 and its poses.
 * scan: the scan's index in its graph (n_scans before it), or -1 when not accepted.  prev: the last scan, or -1.
 * job: its row in the ke_job / kl_query arrays, or -1.  seq: its row in the sequential batch and the
 *   kl_closest_item array, or -1 (not accepted, or a first scan).
 * run_begin, run_length: the graph's running scans before this scan.
 * match_status: 0 until kp_apply_match_device stores d_seq[seq].status here (KP_EINVAL: seq >= n_seq).
 * corrected: the scan's corrected pose: odom for a first scan, else the odometry carry; after
 *   kp_apply_match_device the corrected pose SetSensorPose(bestPose) gives: the pose AddNode reads.
 * sensor: GetSensorAt(corrected), the scan's pool pose; after kp_apply_match_device the matched pose. */
typedef struct kp_intake {
    int status, accepted, scan, prev, job, seq, run_begin, run_length, match_status, pad_;
    double corrected[3];
    double sensor[3];
} kp_intake;

/* What kp_advance_device left for candidate i: the graph's running scans and scan count after the call (unchanged
 * when the candidate was not accepted: accepted 0, corrected +0.0), and GetCorrectedPose() of the scan at its final
 * pool pose, by SetSensorPose's formula. */
typedef struct kp_advanced {
    int run_begin, run_length, n_scans, accepted;
    double corrected[3];
} kp_advanced;

typedef struct kp_state {
    int n_scans, run_begin, run_length, pad_;
    double last_time;
    double last_odom[3];
} kp_state;

typedef struct kp_ctx kp_ctx;

const char *kp_version(void);
const char *kp_last_error(void);
/* Mapper::InitializeParameters defaults (3600, 0.2, DegreesToRadians(10), 20, 70) | the node's mapper_params.yaml
 * (3600, 0.2, 0.174, 100, 110); inverted 0 */
void kp_default_params(kp_params *params);
void kp_node_params(kp_params *params);

/* A fleet of n_graphs graphs of up to max_scans (<= KL_MAX_SCANS) scans of n_readings (1 .. 4096) readings;
 * pool_offset int[n_graphs] (host; NULL: g * max_scans).  params NULL means kp_default_params.  The thresholds
 * Square(d) - KT_TOLERANCE are computed here, once, in double.  KP_EINVAL for scan_buffer_size < 1, for a buffer
 * distance with !(Square(d) - KT_TOLERANCE >= 0.0) (the reference would erase the last running scan and call
 * front() on an empty vector), for a NaN gate parameter, n_readings outside 1 .. 4096, max_scans < 1 or
 * > KL_MAX_SCANS, or a negative pool offset.  Every graph starts empty. */
int kp_create(kp_ctx **out, const kp_params *params, int n_graphs, int n_readings, int max_scans,
              const int *pool_offset);
int kp_destroy(kp_ctx *ctx);

/* STAGE 1.  Candidates d_candidates[i], i < count, of graphs [g_first, g_first + count): three launches, no host
 * synchronisation.  The graph state is not changed: a second call with the same inputs writes the same bits.
 *
 * Per present candidate (one wave each): the corrected pose -- odom for a graph without scans, else the last
 * scan's corrected pose recomputed from its CURRENT pool pose by SetSensorPose's formula (CorrectPoses may have moved
 * it) and Transform(lastOdom, lastCorrected).TransformPose(odom) -- then HasMovedEnough.  A rejected candidate
 * writes nothing but its record.  An accepted scan gets index n_scans; row pool_offset + n_scans of d_pool_ranges
 * is written from its float row (reversed when `inverted`), and GetSensorAt(corrected) to its pool pose.
 *
 * Outputs, compacted over the accepted candidates with their order kept:
 *   d_query, d_base_begin, d_base_index: kt_match_batch_device's arrays over the accepted scans that have a last
 *     scan: match s matches pool slot d_query[s] against the graph's running scans, front to back, as pool slots.
 *     Sizes int[count], int[count + 1], int[base_capacity]; base_capacity >= count * min(scan_buffer_size,
 *     max_scans) (KP_EINVAL otherwise: a window is never truncated).  *d_n_seq (device, one int): the match count.
 *   d_jobs ke_job[count]: {g, scan, pool_offset, prev = scan - 1 or -1, seq_result = running = seq or -1, 0, 0}.
 *   d_queries kl_query[count]: {g, scan, 0, -1, -1}, in job order.  *d_n_jobs (device, one int): the job count.
 *   d_closest_items kl_closest_item[count]: {g, scan, run_begin, run_length}, in seq order.
 * Rows past the counts are not written.  d_jobs, d_queries, d_closest_items may each be NULL. */
int kp_intake_device(kp_ctx *ctx, int g_first, int count, const kp_candidate *d_candidates,
                     const float *d_ranges_f32, int n_rows, double *d_pool_ranges, double *d_pool_poses,
                     int pool_scans, int *d_query, int *d_base_begin, int *d_base_index, int base_capacity,
                     int *d_n_seq, ke_job *d_jobs, kl_query *d_queries, int *d_n_jobs,
                     kl_closest_item *d_closest_items, void *hip_stream);

/* STAGE 2.  Per accepted candidate of the last intake with a seq index: d_seq[seq].mean is written to its pool pose
 * (SetSensorPose(bestPose)) and the record's sensor and corrected poses follow it.  A match whose status is not
 * KT_OK (KT_ERANGE) leaves the pose as predicted; its status goes to match_status.  One launch, stream-ordered. */
int kp_apply_match_device(kp_ctx *ctx, const kt_result *d_seq, int n_seq, double *d_pool_poses, int pool_scans,
                          void *hip_stream);

/* HOST COMMIT of the vertices.  Waits for the last intake / apply call, copies the records back and, per accepted
 * candidate in order, calls kl_add_vertex(kl, g, &id) and spa_add_node(spa, g, scan, corrected): id must equal the
 * scan index (KP_EINVAL otherwise, the edits before it stay).  spa may be NULL.  *n_added (may be NULL) counts the
 * vertices added. */
int kp_commit_vertices(kp_ctx *ctx, kl_ctx *kl, spa_ctx *spa, int *n_added);

/* Fill near_first / near_count of the last intake's job rows from kl_emit_batch_device(KL_NEAR_CHAINS)'s d_source
 * (ordered by slot; slot = job index) and *d_n_matches (clamped to max_matches): after this the second
 * ke_add_edges_device call needs no host-built jobs.  One launch, stream-ordered. */
int kp_bind_near_device(kp_ctx *ctx, ke_job *d_jobs, const kl_source *d_source, const int *d_n_matches,
                        int max_matches, void *hip_stream);

/* STAGE 3, after ke_add_edges_device(KE_WRITE_POSE) and before any loop-closure pose write.  Per accepted candidate
 * of the last intake (one wave each): AddRunningScan -- the new front is the first f >= front with back - f + 1 <=
 * scan_buffer_size && !(d2(f, back) > thr), 64 values of f tested per round -- then n_scans + 1 and SetLastScan's
 * odometric pose and time.  kp_advanced i is written for every candidate.  One launch, stream-ordered. */
int kp_advance_device(kp_ctx *ctx, const double *d_pool_poses, int pool_scans, void *hip_stream);

/* The last intake's records [first, first + count) and the last advance's (either may be NULL; waits). */
int kp_get_intake(kp_ctx *ctx, int first, int count, kp_intake *out, kp_advanced *advanced_out);
/* The same on the device: kp_intake[n_graphs] and kp_advanced[n_graphs] (indexed by candidate), kp_state[n_graphs]
 * (indexed by graph), the two counts int[2] = jobs, seq matches; any output may be NULL. */
int kp_result_device(kp_ctx *ctx, const kp_intake **d_intake, const kp_advanced **d_advanced,
                     const kp_state **d_state, const int **d_counts);
int kp_get_state(kp_ctx *ctx, int g, kp_state *out);
/* Seed a graph that already has scans: KP_EINVAL unless 0 <= n_scans <= max_scans, and either n_scans == 0 (then
 * the window must be empty) or 1 <= run_length <= min(scan_buffer_size, n_scans) and run_begin + run_length ==
 * n_scans.  Waits for the context's device work. */
int kp_set_state(kp_ctx *ctx, int g, const kp_state *state);
int kp_clear_graph(kp_ctx *ctx, int g);

int kp_set_timing(kp_ctx *ctx, int enable);
/* Accumulated device time per kernel: names kp_kernel_name(i), i < kp_num_kernels(). */
int kp_num_kernels(void);
const char *kp_kernel_name(int i);
int kp_get_kernel_times(kp_ctx *ctx, double *ms_out, int64_t *launches_out, int reset);

#ifdef __cplusplus
}
#endif

#endif
