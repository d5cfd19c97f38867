/* include/slam2d/karto_loop.h -- C-ABI of the MI355X Karto loop-closure and near-chain candidate search (lesson6,
 * config 5): which scans a new scan is matched against, decided on the device for a fleet of pose graphs.
 *
 * Reference: open_karto's MapperGraph (lesson6/lib/open_karto/src/Mapper.cpp) on the scans' reference poses, the
 * barycentres LocalizedRangeScan::Update computes (lesson6/lib/open_karto/include/open_karto/Karto.h:5362-5416).
 * Each entry point replaces one reference member:
 *
 *   kl_add_vertex          MapperGraph::AddVertex (the scan's state id is the vertex count before the call)
 *   kl_add_edge            MapperGraph::AddEdge                                              Mapper.cpp:1075-1101
 *   kl_set_scans[_device]  LocalizedRangeScan::Update, the barycentre only                   Karto.h:5374-5416
 *   kl_refresh_device      the same for scans named by rows of device memory (after SetSensorPose at Mapper.cpp:1032,
 *                          :2044, and for every scan of a graph in CorrectPoses, Mapper.cpp:1397-1414)
 *   kl_search[_device]     FindNearLinkedScans (BreadthFirstTraversal::Traverse with NearScanVisitor)
 *                                                                       Mapper.cpp:1278-1286, Mapper.h:568-637
 *                          FindPossibleLoopClosure, every call of TryCloseLoop's while loop  Mapper.cpp:1333-1394
 *                          FindNearChains, LinkNearChains' size filter                       Mapper.cpp:1170-1275, :1131
 *                          GetClosestScanToPose / LinkChainToScan's distance test on a near chain
 *                                                                       Mapper.cpp:1054-1073, :1152-1167
 *   kl_closest_device      GetClosestScanToPose / LinkChainToScan's test for the running scans (Mapper.cpp:962)
 *                          and for a loop chain after SetSensorPose(bestPose) (Mapper.cpp:1032-1035)
 *   kl_emit_batch_device   the candidate chains as the arrays kt_match_batch_device (karto.h) takes
 *   kl_edit_vertices_device / kl_edit_edges_device   AddVertex / AddEdge again, applied by kernels to rows of
 *                          device memory ("GRAPH EDITS ON THE DEVICE" below; karto_edit.h feeds them)
 *
 * ONE sensor only: the node has one laser, so a graph's scans are one sensor's and a scan's state id is its index.
 *
 * Out of scope here: the accept / reject thresholds of TryCloseLoop and LinkNearChains on response and variance,
 * LinkScans with the optimiser's AddConstraint and ComputeWeightedMean are karto_link.h's (ke_*), which consumes
 * this header's results on the device; the running-scan buffer (AddRunningScan) is karto_process.h's (kp_*), which
 * writes the kl_query rows and the running chain's kl_closest_item; more than one sensor stays with the caller.
 * open_karto needs boost, absent from this image,
 * so parity with the compiled library is UNPINNED, as for the matcher (karto.h), the grid (karto_grid.h) and the
 * optimiser (spa.h): the results equal the CPU restatement tests/ref/karto_loop_ref.c bit for bit, and that
 * restatement equals a literal transcription of the reference members (tests/ref/karto_loop_plain.py).
 *
 * Arithmetic: IEEE double without FMA contraction; sin / cos are csrc/detmath.h's.  A squared distance is
 * Square(dx) + Square(dy) (Karto.h:1011-1032).  The barycentre's sum starts from +0.0 and adds the valid points in
 * beam order, one at a time; each component is then divided by the count (Karto.h:1098-1101).
 *
 * Limits: a graph holds at most KL_MAX_SCANS = 4096 scans (the search keeps its per-scan state in one workgroup's
 * LDS).  A context asked for more, and a graph grown beyond its context's max_scans or max_edges, is refused with
 * KL_ERANGE, never truncated.
 *
 * Conventions as in karto.h and spa.h: plain C types, int status (KL_OK / negative), kl_last_error().  A pose is
 * double[3] = x, y, heading (rad); the laser offset is identity.
 */
#ifndef SLAM2D_KARTO_LOOP_H
#define SLAM2D_KARTO_LOOP_H

#include <stddef.h>
#include <stdint.h>

#include "karto.h" /* kt_laser */

#ifdef __cplusplus
extern "C" {
#endif

#define KL_OK 0
#define KL_EINVAL (-1)
#define KL_EHIP (-2)
#define KL_ENOMEM (-3)
#define KL_ENODEV (-4)
#define KL_ERANGE (-5) /* more scans or edges than the context (or KL_MAX_SCANS) holds */

#define KL_MAX_SCANS 4096
#define KL_TOLERANCE 1e-06 /* KT_TOLERANCE, open_karto/Math.h:41 */

#define KL_LOOP_CHAINS 0
#define KL_NEAR_CHAINS 1

#define KL_CHAIN_LONG 1   /* kl_near_chain.flags bit 0: length >= loop_match_minimum_chain_size (Mapper.cpp:1131) */
#define KL_CHAIN_LINKED 2 /* bit 1: d2[closest] < link * link + KL_TOLERANCE (Mapper.cpp:1163) */

#define KL_EMIT_OVERFLOW 1 /* kl_get_emit_info status: more matches than capacity, the first capacity emitted */

typedef struct kl_params {
    double link_scan_maximum_distance;   /* Mapper default 10.0 (Mapper.cpp:1462-1545) | mapper_params.yaml 1.5 */
    double loop_search_maximum_distance; /* 4.0 | 10.0 */
    int loop_match_minimum_chain_size;   /* 10 | 5 */
    int use_scan_barycenter;             /* 1 | 1 */
} kl_params;

/* pScan, rStartNum of the first FindPossibleLoopClosure call, and the visible prefix of the graph: the first
 * n_scans scans and the first n_edges edges (-1: all), so that a replay of one graph runs as many queries in one
 * launch.  An adjacency entry whose edge or whose other end lies outside the prefix is skipped. */
typedef struct kl_query {
    int graph, scan, start_num, n_scans, n_edges;
} kl_query;

typedef struct kl_result {
    int status;           /* KL_OK, or KL_EINVAL: graph, scan (scan >= n_scans), start_num or a prefix out of range;
                             every count is then 0 and the slot's lists are not written */
    int n_scans;          /* visible scans: the d2 entries */
    int n_near_link;      /* FindNearLinkedScans(pScan, link_scan_maximum_distance) */
    int n_near_loop;      /* FindNearLinkedScans(pScan, loop_search_maximum_distance) */
    int n_loop_chains;
    int n_near_chains;
    int loop_index_total; /* the loop chains' lengths, summed */
    int n_near_long;      /* near chains with KL_CHAIN_LONG */
    int near_index_total; /* their lengths, summed */
    int pad_;
} kl_result;

/* One non-empty return of FindPossibleLoopClosure: scans [begin, begin + length); resume is the rStartNum the call
 * leaves behind -- the index of the out-of-range scan that ended the chain (the return precedes the increment), or
 * n_scans for the chain that runs to the end of the scans (returned at any non-empty length, Mapper.cpp:1393). */
typedef struct kl_loop_chain {
    int begin, length, resume, pad_;
} kl_loop_chain;

/* One chain of FindNearChains: scans [begin, begin + length); closest is GetClosestScanToPose over the chain
 * (strict <: the first minimum wins); flags KL_CHAIN_LONG | KL_CHAIN_LINKED.  closest and KL_CHAIN_LINKED hold for
 * the scan's reference position at the search, which LinkNearChains does not move. */
typedef struct kl_near_chain {
    int begin, length, closest, flags;
} kl_near_chain;

typedef struct kl_closest_item {
    int graph, scan, begin, length;
} kl_closest_item;

/* closest: the chain's scan nearest to `scan`'s current reference position, or -1 (item out of range, or no
 * squared distance below DBL_MAX); linked: 1 when d2[closest] < link * link + KL_TOLERANCE. */
typedef struct kl_closest {
    int closest, linked;
} kl_closest;

/* kl_emit_batch_device's d_source_out element */
typedef struct kl_source {
    int slot, chain;
} kl_source;

typedef struct kl_ctx kl_ctx;

const char *kl_version(void);
const char *kl_last_error(void);
/* Mapper::InitializeParameters defaults (Mapper.cpp:1462-1545) | the node's mapper_params.yaml */
void kl_default_params(kl_params *params);
void kl_node_params(kl_params *params);

/* A fleet of max_graphs graphs of up to max_scans (<= KL_MAX_SCANS) scans and max_edges edges each, and result
 * slots for max_queries queries per search.  params NULL means kl_default_params.  The thresholds d * d -
 * KL_TOLERANCE and d * d + KL_TOLERANCE are computed here, once, in double. */
int kl_create(kl_ctx **out, const kt_laser *laser, const kl_params *params, int max_graphs, int max_scans,
              int max_edges, int max_queries);
int kl_destroy(kl_ctx *ctx);

/* AddVertex: *state_id (may be NULL) is the scan count before the call. */
int kl_add_vertex(kl_ctx *ctx, int g, int *state_id);
/* AddEdge with its dedupe rule: the edge is old (*is_new = 0, nothing added) only if source's edge list already
 * holds an edge whose target is `target`, so a -> b does not block b -> a.  source == target is KL_EINVAL.  A
 * vertex's adjacency is its edge list in insertion order (an edge is appended to its source's list, then to its
 * target's, Mapper.h:304-309), each entry the other end of the edge (GetAdjacentVertices, Mapper.h:251-272). */
int kl_add_edge(kl_ctx *ctx, int g, int source, int target, int *is_new);
/* Bulk form, no dedupe: n_scans vertices and the edges ends int[n_edges][2] = source, target, in insertion order. */
int kl_set_graph(kl_ctx *ctx, int g, int n_scans, int n_edges, const int *ends);
int kl_clear_graph(kl_ctx *ctx, int g);
int kl_get_counts(kl_ctx *ctx, int g, int *n_scans, int *n_edges);
/* Graph g's scan i is pool slot offset + i in what kl_emit_batch_device writes (0 initially). */
int kl_set_pool_offset(kl_ctx *ctx, int g, int offset);

/* Recompute the reference position of scans [first, first + count) of graph g (first + count <= max_scans) from
 * ranges double[count][n_readings] and poses double[count][3]: the layouts of kt_pool_device and
 * spa_device_poses, so the optimiser's output feeds this call with no copy.  A reading is valid when
 * minimum_range <= r <= range_threshold (math::InRange: inclusive, false for NaN); with no valid reading, or with
 * use_scan_barycenter == 0, the reference position is the sensor position.  The other scans keep theirs. */
int kl_set_scans(kl_ctx *ctx, int g, int first, int count, const double *ranges, const double *poses);
int kl_set_scans_device(kl_ctx *ctx, int g, int first, int count, const double *d_ranges, const double *d_poses,
                        void *hip_stream);
/* out double[count][2] */
int kl_get_reference(kl_ctx *ctx, int g, int first, int count, double *out);

/* The same refresh for scans that ROWS OF DEVICE MEMORY name, so that a fleet round needs no count on the host: row i
 * recomputes the reference position of scans [first, first + count) of `graph`, scan first + j from row pool_first + j
 * of d_pool_ranges double[pool_scans][n_readings] and d_pool_poses double[pool_scans][3].  The value written is
 * kl_set_scans_device's, bit for bit; scans named by no row keep theirs.  One launch, stream-ordered, with no host
 * synchronisation and no copy -- unless a graph has pending HOST edits, which are uploaded first (the only case in
 * which the call waits).
 *
 * count < 0: through the graph's last scan as the DEVICE header has it (n_scans - first, or 0 when that is negative).
 * graph < 0: the row is skipped.  A row is refused, writes nothing and is counted (kl_get_refresh_info) for a graph
 * >= max_graphs or first < 0 (KL_EINVAL), and for scans beyond max_scans or a pool slot outside [0, pool_scans)
 * (KL_ERANGE); an explicit count is bounded by max_scans only, as kl_set_scans_device's is.  d_resolved_out[i] (may
 * be NULL) is {pool_first, the count applied}, {0, 0} for a skipped or refused row.  Two rows that name the same scan
 * must name the same pool slot for it.  More than KL_REFRESH_MAX_ROWS rows are refused with KL_ERANGE at the call.
 *
 * SLAM2D_REFRESH_WG (read once, at kl_create; one whole decimal integer, anything else is refused there with
 * KL_EINVAL): > 0 caps the launch at that many workgroups. */
#define KL_REFRESH_MAX_ROWS 4096
typedef struct kl_refresh_row {
    int graph, first, count, pool_first;
} kl_refresh_row;
/* d_resolved_out's element; the layout of HIP's int2 (this header stays plain C) */
typedef struct kl_refresh_span {
    int pool_first, count;
} kl_refresh_span;
int kl_refresh_device(kl_ctx *ctx, int n_rows, const kl_refresh_row *d_rows, const double *d_pool_ranges,
                      const double *d_pool_poses, int pool_scans, kl_refresh_span *d_resolved_out, void *hip_stream);
/* Rows kl_refresh_device refused since the last call of this function, and the status of the first of them in
 * (call, row) order (KL_OK: none).  Waits. */
int kl_get_refresh_info(kl_ctx *ctx, int *n_refused, int *first_status);

/* `count` (<= max_queries) queries, one workgroup each, one launch, no host synchronisation; query i's results go
 * to slot i and stay on the device until the next search.  Only graphs edited since their last search cost more:
 * they are uploaded first, which waits for the context's previous device work.  kl_search takes host queries and
 * waits. */
int kl_search(kl_ctx *ctx, int count, const kl_query *queries);
int kl_search_device(kl_ctx *ctx, int count, const kl_query *d_queries, void *hip_stream);

/* Results of slot `slot` of the last search (each waits for it).  d2 double[n_scans]; near lists int[n_near_*] in
 * the reference's breadth-first visiting order; any output may be NULL. */
int kl_get_result(kl_ctx *ctx, int slot, kl_result *result);
int kl_get_d2(kl_ctx *ctx, int slot, double *d2);
int kl_get_near(kl_ctx *ctx, int slot, int *near_link, int *near_loop);
int kl_get_chains(kl_ctx *ctx, int slot, kl_loop_chain *loop_chains, kl_near_chain *near_chains);
/* The same on the device: kl_result[max_queries], double[max_queries][max_scans], int[max_queries][max_scans]
 * twice, and the chain arrays [max_queries][*chain_stride]; any output may be NULL. */
int kl_result_device(kl_ctx *ctx, const kl_result **d_results, const double **d_d2, const int **d_near_link,
                     const int **d_near_loop, const kl_loop_chain **d_loop_chains,
                     const kl_near_chain **d_near_chains, int *chain_stride);

/* closest and the link flag of `count` chains against their scans' CURRENT reference positions (refresh the one
 * scan with kl_set_scans_device first); d_out kl_closest[count].  One launch, stream-ordered. */
int kl_closest_device(kl_ctx *ctx, int count, const kl_closest_item *d_items, kl_closest *d_out, void *hip_stream);

/* Compact the chains of the last search's first `count` slots into kt_match_batch_device's arrays, as pool slots
 * (kl_set_pool_offset): match m matches d_query_out[m] against d_base_index_out[d_base_begin_out[m] ..
 * d_base_begin_out[m + 1]); d_source_out[m] names its slot and chain.  which = KL_LOOP_CHAINS: every loop chain;
 * KL_NEAR_CHAINS: the near chains with KL_CHAIN_LONG.  Matches are ordered by slot, then by chain order.
 * Sizes: d_query_out int[capacity], d_base_begin_out int[capacity + 1], d_source_out kl_source[capacity],
 * d_base_index_out int[min(count, capacity) * max_scans] (a slot's chains are disjoint ranges of one graph's
 * scans).  *d_n_matches (device, one int) is the number emitted: more matches than capacity sets KL_EMIT_OVERFLOW
 * (kl_get_emit_info) and emits the first capacity of them.  Two launches, no host synchronisation. */
int kl_emit_batch_device(kl_ctx *ctx, int count, int which, int capacity, int *d_query_out, int *d_base_begin_out,
                         int *d_base_index_out, kl_source *d_source_out, int *d_n_matches, void *hip_stream);
/* The last emit's match count before the capacity cut, and its status (waits for it). */
int kl_get_emit_info(kl_ctx *ctx, int *total_matches, int *status);

/* GRAPH EDITS ON THE DEVICE.  The same edits as kl_add_vertex / kl_add_edge, applied by kernels, stream-ordered,
 * with no host synchronisation and no copy -- unless a graph has pending HOST edits, which are uploaded first (the
 * only case in which these calls wait).  They leave the context's device arrays (header, edge list, adjacency) as
 * host edits followed by the upload would have.  All row arrays are device memory; any output array may be NULL.
 * One workgroup per row; the first row that names a graph leads it and applies all its rows in row order, so rows
 * of several graphs may be interleaved.  The cost grows with count and with the touched graphs' sizes.
 *
 * A device edit leaves the host's copy of the graphs behind.  kl_add_vertex, kl_add_edge and kl_get_counts then
 * first pull their graph back (they wait and copy its header and edge list); kl_set_graph and kl_clear_graph
 * overwrite it.
 *
 * kl_edit_vertices_device: row i adds one vertex to graph d_graph[i] (negative: the row is skipped, status KL_OK,
 * id -1).  d_id_out[i] is the scan count before the row, or -1 when it is refused: with d_expect_id non-NULL and
 * d_expect_id[i] >= 0, KL_EINVAL unless that count equals it; KL_ERANGE when the graph holds max_scans scans;
 * KL_EINVAL for a graph >= max_graphs.
 *
 * kl_edit_edges_device: AddEdge's rule exactly as kl_add_edge states it, earlier rows of the same call included.
 * d_is_new_out[i] is 1 or 0 (0 for skipped and refused rows).  Refusals are kl_add_edge's: an end that is not a
 * vertex, or a self edge, KL_EINVAL; max_edges reached, KL_ERANGE.  A refused row changes nothing and the LATER
 * ROWS, OF THAT GRAPH TOO, ARE STILL APPLIED: the host ke_commit ends at its first failure, this path does not. */
typedef struct kl_edge_row {
    int graph, source, target, pad_;
} kl_edge_row;

int kl_edit_vertices_device(kl_ctx *ctx, int count, const int *d_graph, const int *d_expect_id, int *d_id_out,
                            int *d_status_out, void *hip_stream);
int kl_edit_edges_device(kl_ctx *ctx, int count, const kl_edge_row *d_rows, int *d_is_new_out, int *d_status_out,
                         void *hip_stream);
/* Rows the device edits refused since the last call of this function, and the status of the first of them in
 * (call, row) order (KL_OK: none).  Waits. */
int kl_get_edit_info(kl_ctx *ctx, int *n_refused, int *first_status);
/* Inspection: uploads pending host edits, waits, and copies graph g's DEVICE arrays back: ends int[n_edges][2],
 * adj_off int[n_scans + 1], adj int[2 n_edges][2] (other end, edge index).  Any output may be NULL. */
int kl_download_graph(kl_ctx *ctx, int g, int *n_scans, int *n_edges, int *ends_out, int *adj_off_out, int *adj_out);

int kl_set_timing(kl_ctx *ctx, int enable);
/* Accumulated device time per kernel: names kl_kernel_name(i), i < kl_num_kernels(). */
int kl_num_kernels(void);
const char *kl_kernel_name(int i);
int kl_get_kernel_times(kl_ctx *ctx, double *ms_out, int64_t *launches_out, int reset);

#ifdef __cplusplus
}
#endif

#endif
