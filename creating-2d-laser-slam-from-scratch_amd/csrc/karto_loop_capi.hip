// karto_loop_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_loop.h) of the Karto loop-closure
// and near-chain candidate search.  The search runs in karto_loop_kernels.hip; the host keeps each graph's edge lists
// (karto_loop_graph.h) and uploads an edited graph before the next search.  Without a usable HIP device kl_create
// fails with KL_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_graph_mirror.h"
#include "karto_loop_graph.h"
#include "scan_refresh_plan.h"
#include "karto_loop_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError kl_err;
S2D_ASSERT_STATUS_CODES(KL);

constexpr int KL_MAX_GRAPHS = 1 << 16;
constexpr int KL_MAX_EDGES = 1 << 20;
constexpr int KL_MAX_QUERIES = 1 << 20;

enum { L_REFERENCE, L_SEARCH, L_CLOSEST, L_EMIT_SCAN, L_EMIT_WRITE, L_REFRESH, L_EDIT_VERTICES, L_EDIT_EDGES, L_NUM };
const char *const l_names[L_NUM] = {"kl_reference_kernel", "kl_search_kernel", "kl_closest_kernel", "kl_emit_scan_kernel",
                                    "kl_emit_write_kernel", "kl_refresh_kernel", "kl_edit_vertices_kernel",
                                    "kl_edit_edges_kernel"};
static_assert(L_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
static_assert(KL_REFRESH_MAX_ROWS == REFRESH_MAX_ROWS, "the plan header's row limit");
static_assert(KL_WAVES == REFRESH_WAVES, "the plan header's scans per workgroup");
static_assert(sizeof(kl_refresh_span) == sizeof(int2) && sizeof(kl_refresh_row) == 16, "the row layouts");
}  // namespace

struct kl_ctx {
    int G = 0, N = 0, M = 0, Q = 0;
    kt_laser laser{};
    kl_params params{};
    std::vector<KlGraph> graphs;
    std::vector<int> pool_offset;
    std::vector<char> dirty;  // per graph: edited since the last upload
    bool any_dirty = false;
    DeviceEditEpoch edit;  // device edits: which host copies are behind
    DeviceEditEpoch refresh;  // kl_refresh_device's refused rows (its words and call numbers only)
    RefreshOptions refresh_opt;
    int num_cus = 1;
    int2 *d_ends = nullptr;
    KlDev dev{};
    KlHdr *d_hdr = nullptr;
    int *d_adj_off = nullptr;
    int2 *d_adj = nullptr;
    kl_query *d_qin = nullptr;               // kl_search's host queries
    double *d_ranges = nullptr, *d_poses = nullptr;  // kl_set_scans' host arrays, grown on demand
    size_t stage_scans = 0;
    size_t lds = 0;
    StreamOrder order;
    DeviceBuffers mem;
    KernelTimer timer;
};

namespace {

#define KL_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, kl_err.fail, KL_EHIP, call.s, which, __VA_ARGS__)

int check_graph(const kl_ctx *c, int g)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (g < 0 || g >= c->G) return kl_err.fail(KL_EINVAL, "graph index out of range");
    return KL_OK;
}

// An edited graph: its header and adjacency.  The copies are synchronous and follow the previous device work.
int upload_graph(kl_ctx *c, int g)
{
    KlGraph &gr = c->graphs[g];
    gr.compile();
    const size_t N = (size_t)c->N, M = (size_t)c->M;
    const KlHdr h{gr.n_scans(), gr.n_edges(), c->pool_offset[g], 0};
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(c->d_hdr + g, &h, sizeof(h), hipMemcpyHostToDevice));
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(c->d_adj_off + g * (N + 1), gr.adj_off.data(), sizeof(int) * (gr.n_scans() + 1), hipMemcpyHostToDevice));
    if (!gr.ends.empty())
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(c->d_ends + g * M, gr.ends.data(), sizeof(int) * gr.ends.size(), hipMemcpyHostToDevice));
    if (!gr.adj.empty())
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(c->d_adj + g * 2 * M, gr.adj.data(), sizeof(int) * gr.adj.size(), hipMemcpyHostToDevice));
    c->dirty[g] = 0;
    return KL_OK;
}

int upload_dirty(kl_ctx *c)
{
    if (!c->any_dirty) return KL_OK;
    int rc = c->order.wait_last(kl_err);
    if (rc != KL_OK) return rc;
    for (int g = 0; g < c->G; ++g)
        if (c->dirty[g] && (rc = upload_graph(c, g)) != KL_OK) return rc;
    c->any_dirty = false;
    return KL_OK;
}

// The host copy of graph g, current again after device edits: waits, and copies the header and the edge list back.
int pull_graph(kl_ctx *c, int g)
{
    if (c->edit.current(g)) return KL_OK;
    int rc = c->order.wait_last(kl_err);
    if (rc != KL_OK) return rc;
    KlHdr h{};
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(&h, c->d_hdr + g, sizeof(h), hipMemcpyDeviceToHost));
    if (h.n_scans < 0 || h.n_scans > c->N || h.n_edges < 0 || h.n_edges > c->M)
        return kl_err.fail(KL_EHIP, "the device header of the graph is out of range");
    std::vector<int> ends((size_t)h.n_edges * 2);
    if (h.n_edges > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(ends.data(), c->d_ends + (size_t)g * c->M, sizeof(int) * ends.size(), hipMemcpyDeviceToHost));
    if (!kl_mirror_rebuild(c->graphs[g], h.n_scans, h.n_edges, ends.data()))
        return kl_err.fail(KL_EHIP, "the device edge list of the graph is not a graph's");
    c->edit.mark_current(g);
    return KL_OK;
}

KlEdit edit_args(kl_ctx *c)
{
    return KlEdit{c->d_hdr, c->d_adj_off, c->d_adj, c->d_ends, c->edit.d_info, c->N, c->M, c->G, c->edit.seq};
}

// before a device edit: pending host edits go up (the only wait); afterwards every host copy is behind
int begin_edit(kl_ctx *c, StreamCall &call)
{
    int rc = upload_dirty(c);
    if (rc != KL_OK) return rc;
    c->edit.bump();
    return call.begin();
}

void touch(kl_ctx *c, int g)
{
    c->dirty[g] = 1;
    c->any_dirty = true;
}

int run_reference(kl_ctx *c, int g, int first, int count, const double *d_ranges, const double *d_poses, StreamCall &call)
{
    int rc = call.begin();
    if (rc != KL_OK) return rc;
    KL_LAUNCH(L_REFERENCE, kl_reference_kernel, dim3((unsigned)count), dim3(KL_THREADS), 0, call.s, c->dev, g, first,
              d_ranges, d_poses);
    return call.done();
}

int run_search(kl_ctx *c, int count, const kl_query *d_queries, StreamCall &call)
{
    int rc = upload_dirty(c);
    if (rc != KL_OK) return rc;
    if ((rc = call.begin()) != KL_OK) return rc;
    KL_LAUNCH(L_SEARCH, kl_search_kernel, dim3((unsigned)count), dim3(KL_THREADS), c->lds, call.s, c->dev, d_queries, c->G);
    return call.done();
}

int check_scan_range(kl_ctx *c, int g, int first, int count)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    if (first < 0 || count < 0) return kl_err.fail(KL_EINVAL, "negative scan range");
    if (first > c->N - count) return kl_err.fail(KL_ERANGE, "scans beyond the context's max_scans");
    return KL_OK;
}

int check_slot(kl_ctx *c, int slot)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (slot < 0 || slot >= c->Q) return kl_err.fail(KL_EINVAL, "slot out of range");
    return KL_OK;
}

}  // namespace

extern "C" {

const char *kl_last_error(void) { return kl_err.c_str(); }
const char *kl_version(void) { return "slam2d-karto-loop 1 (gfx950)"; }

void kl_default_params(kl_params *p)
{
    if (!p) return;
    // Mapper::InitializeParameters (lesson6/lib/open_karto/src/Mapper.cpp:1462-1545)
    p->link_scan_maximum_distance = 10.0;
    p->loop_search_maximum_distance = 4.0;
    p->loop_match_minimum_chain_size = 10;
    p->use_scan_barycenter = 1;
}

void kl_node_params(kl_params *p)
{
    if (!p) return;
    // lesson6's mapper_params.yaml
    p->link_scan_maximum_distance = 1.5;
    p->loop_search_maximum_distance = 10.0;
    p->loop_match_minimum_chain_size = 5;
    p->use_scan_barycenter = 1;
}

int kl_destroy(kl_ctx *c)
{
    if (!c) return KL_OK;
    c->order.destroy();
    c->mem.free_all();
    c->timer.destroy();
    delete c;
    return KL_OK;
}

int kl_create(kl_ctx **out, const kt_laser *laser, const kl_params *params, int max_graphs, int max_scans, int max_edges,
              int max_queries)
{
    if (!out) return kl_err.fail(KL_EINVAL, "out is NULL");
    *out = nullptr;
    if (!laser) return kl_err.fail(KL_EINVAL, "laser is NULL");
    if (laser->n_readings < 1 || laser->n_readings > 4096) return kl_err.fail(KL_EINVAL, "need 1 <= n_readings <= 4096");
    if (max_graphs < 1 || max_graphs > KL_MAX_GRAPHS || max_scans < 1 || max_edges < 1 || max_edges > KL_MAX_EDGES ||
        max_queries < 1 || max_queries > KL_MAX_QUERIES)
        return kl_err.fail(KL_EINVAL, "need 1 <= max_graphs <= 2^16, max_scans >= 1, 1 <= max_edges <= 2^20, 1 <= max_queries <= 2^20");
    if (max_scans > KL_MAX_SCANS) return kl_err.fail(KL_ERANGE, "max_scans exceeds KL_MAX_SCANS (4096)");
    kl_params p;
    if (params) p = *params;
    else kl_default_params(&p);
    if (!(p.link_scan_maximum_distance >= 0) || !(p.loop_search_maximum_distance >= 0) ||
        !std::isfinite(p.link_scan_maximum_distance) || !std::isfinite(p.loop_search_maximum_distance))
        return kl_err.fail(KL_EINVAL, "the distances must be finite and >= 0");
    int poison = 0;
    if (const char *why = poison_from_env(poison)) return kl_err.fail(KL_EINVAL, why);
    RefreshOptions refresh_opt;
    if (const char *why = refresh_parse_options(refresh_opt, [](const char *knob) -> const char * { return getenv(knob); }))
        return kl_err.fail(KL_EINVAL, why);
    if (!device_present()) return kl_err.fail(KL_ENODEV, "no HIP device");
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return kl_err.fail(KL_ENODEV, "no HIP device");
    kl_ctx *c = new kl_ctx;
    c->refresh_opt = refresh_opt;
    c->num_cus = std::max(1, prop.multiProcessorCount);
    c->G = max_graphs;
    c->N = max_scans;
    c->M = max_edges;
    c->Q = max_queries;
    c->laser = *laser;
    c->params = p;
    c->graphs.resize((size_t)max_graphs);
    c->pool_offset.assign((size_t)max_graphs, 0);
    c->dirty.assign((size_t)max_graphs, 0);
    c->edit.synced.assign((size_t)max_graphs, 0);
    c->lds = kl_search_lds(max_scans);
    hipError_t e;
    if ((e = c->order.create()) != hipSuccess) {
        kl_destroy(c);
        return kl_err.fail(KL_EHIP, "hipStreamCreate", e);
    }
    KlDev &d = c->dev;
    d.max_scans = max_scans;
    d.max_edges = max_edges;
    d.max_queries = max_queries;
    d.chain_stride = max_scans / 2 + 1;
    d.minimum_angle = laser->minimum_angle;
    d.angular_resolution = laser->angular_resolution;
    d.minimum_range = laser->minimum_range;
    d.range_threshold = laser->range_threshold;
    d.n_readings = laser->n_readings;
    d.use_barycenter = p.use_scan_barycenter ? 1 : 0;
    d.min_chain = p.loop_match_minimum_chain_size;
    // math::Square(d) +- KT_TOLERANCE, once, in double (Mapper.cpp:1163, :1223, :1361; Mapper.h:623, :636)
    d.link_hi = p.link_scan_maximum_distance * p.link_scan_maximum_distance + KL_TOLERANCE;
    d.link_lo = p.link_scan_maximum_distance * p.link_scan_maximum_distance - KL_TOLERANCE;
    d.loop_hi = p.loop_search_maximum_distance * p.loop_search_maximum_distance + KL_TOLERANCE;
    d.loop_lo = p.loop_search_maximum_distance * p.loop_search_maximum_distance - KL_TOLERANCE;
    const size_t G = (size_t)max_graphs, N = (size_t)max_scans, M = (size_t)max_edges, Q = (size_t)max_queries;
    const size_t CS = (size_t)d.chain_stride;
    DeviceBuffers &m = c->mem;
    m.alloc(c->d_hdr, sizeof(KlHdr) * G);
    m.alloc(c->d_adj_off, sizeof(int) * G * (N + 1));
    m.alloc(c->d_adj, sizeof(int2) * G * 2 * M);
    m.alloc(c->d_ends, sizeof(int2) * G * M);
    m.alloc(c->edit.d_info, sizeof(unsigned long long) * 2);
    m.alloc(c->refresh.d_info, sizeof(unsigned long long) * 2);
    m.alloc(d.ref, sizeof(double2) * G * N);
    m.alloc(d.res, sizeof(kl_result) * Q);
    m.alloc(d.queries, sizeof(kl_query) * Q);
    m.alloc(d.d2, sizeof(double) * Q * N);
    m.alloc(d.near_link, sizeof(int) * Q * N);
    m.alloc(d.near_loop, sizeof(int) * Q * N);
    m.alloc(d.loop_chains, sizeof(kl_loop_chain) * Q * CS);
    m.alloc(d.near_chains, sizeof(kl_near_chain) * Q * CS);
    m.alloc(d.emit_off, sizeof(int2) * (Q + 1));
    m.alloc(d.emit_info, sizeof(int) * 2);
    m.alloc(c->d_qin, sizeof(kl_query) * Q);
    if ((e = m.error) != hipSuccess || (poison && (e = m.fill(0xA5, c->order.stream)) != hipSuccess)) {
        kl_destroy(c);
        return kl_err.fail(KL_ENOMEM, "hipMalloc", e);
    }
    d.hdr = c->d_hdr;
    d.adj_off = c->d_adj_off;
    d.adj = c->d_adj;
    // every graph starts empty and every slot without a result: a query on an empty graph is refused in its status
    std::vector<kl_result> r0(Q);
    for (auto &r : r0) {
        memset(&r, 0, sizeof(r));
        r.status = KL_EINVAL;
    }
    hipStream_t s = c->order.stream;
    if ((e = hipMemsetAsync(c->d_hdr, 0, sizeof(KlHdr) * G, s)) != hipSuccess ||
        (e = hipMemsetAsync(d.emit_info, 0, sizeof(int) * 2, s)) != hipSuccess ||
        (e = c->edit.reset_async(s)) != hipSuccess || (e = c->refresh.reset_async(s)) != hipSuccess ||
        (e = hipMemcpyAsync(d.res, r0.data(), sizeof(kl_result) * Q, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess || (e = hipEventRecord(c->order.ev_last, s)) != hipSuccess) {
        kl_destroy(c);
        return kl_err.fail(KL_EHIP, "initialising the context", e);
    }
    *out = c;
    return KL_OK;
}

int kl_add_vertex(kl_ctx *c, int g, int *state_id)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != KL_OK) return rc;
    if (c->graphs[g].n_scans() >= c->N) return kl_err.fail(KL_ERANGE, "the graph already has max_scans scans");
    const int id = c->graphs[g].add_vertex();
    if (state_id) *state_id = id;
    touch(c, g);
    return KL_OK;
}

int kl_add_edge(kl_ctx *c, int g, int source, int target, int *is_new)
{
    if (is_new) *is_new = 0;
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != KL_OK) return rc;
    KlGraph &gr = c->graphs[g];
    if (source < 0 || source >= gr.n_scans() || target < 0 || target >= gr.n_scans())
        return kl_err.fail(KL_EINVAL, "edge end is not a vertex of the graph");
    if (source == target) return kl_err.fail(KL_EINVAL, "an edge from a vertex to itself");
    if (gr.find_edge(source, target) >= 0) return KL_OK;  // rIsNewEdge = false
    if (gr.n_edges() >= c->M) return kl_err.fail(KL_ERANGE, "the graph already has max_edges edges");
    gr.append_edge(source, target);
    if (is_new) *is_new = 1;
    touch(c, g);
    return KL_OK;
}

int kl_set_graph(kl_ctx *c, int g, int n_scans, int n_edges, const int *ends)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    if (n_scans < 0 || n_edges < 0) return kl_err.fail(KL_EINVAL, "negative count");
    if (n_scans > c->N || n_edges > c->M) return kl_err.fail(KL_ERANGE, "more scans or edges than the context holds");
    if (n_edges > 0 && !ends) return kl_err.fail(KL_EINVAL, "ends is NULL");
    for (int e = 0; e < n_edges; ++e) {
        const int a = ends[2 * e], b = ends[2 * e + 1];
        if (a < 0 || a >= n_scans || b < 0 || b >= n_scans) return kl_err.fail(KL_EINVAL, "edge end out of range");
        if (a == b) return kl_err.fail(KL_EINVAL, "an edge from a vertex to itself");
    }
    std::lock_guard<std::mutex> lock(c->order.mu);
    KlGraph &gr = c->graphs[g];
    gr.clear();
    for (int k = 0; k < n_scans; ++k) gr.add_vertex();
    for (int e = 0; e < n_edges; ++e) gr.append_edge(ends[2 * e], ends[2 * e + 1]);
    c->edit.mark_current(g);
    touch(c, g);
    return KL_OK;
}

int kl_clear_graph(kl_ctx *c, int g)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    c->graphs[g].clear();
    c->edit.mark_current(g);
    touch(c, g);
    return KL_OK;
}

int kl_get_counts(kl_ctx *c, int g, int *n_scans, int *n_edges)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != KL_OK) return rc;
    if (n_scans) *n_scans = c->graphs[g].n_scans();
    if (n_edges) *n_edges = c->graphs[g].n_edges();
    return KL_OK;
}

int kl_set_pool_offset(kl_ctx *c, int g, int offset)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    if (offset < 0 || offset > INT_MAX - KL_MAX_SCANS) return kl_err.fail(KL_EINVAL, "pool offset out of range");
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != KL_OK) return rc;  // the upload that follows rewrites the whole graph
    c->pool_offset[g] = offset;
    touch(c, g);
    return KL_OK;
}

int kl_set_scans_device(kl_ctx *c, int g, int first, int count, const double *d_ranges, const double *d_poses,
                        void *hip_stream)
{
    int rc = check_scan_range(c, g, first, count);
    if (rc != KL_OK) return rc;
    if (!d_ranges || !d_poses) return kl_err.fail(KL_EINVAL, "NULL argument");
    if (count == 0) return KL_OK;
    StreamCall call(c->order, kl_err, hip_stream);
    return run_reference(c, g, first, count, d_ranges, d_poses, call);
}

int kl_set_scans(kl_ctx *c, int g, int first, int count, const double *ranges, const double *poses)
{
    int rc = check_scan_range(c, g, first, count);
    if (rc != KL_OK) return rc;
    if (!ranges || !poses) return kl_err.fail(KL_EINVAL, "NULL argument");
    if (count == 0) return KL_OK;
    StreamCall call(c->order, kl_err, nullptr);
    const size_t n = (size_t)c->laser.n_readings;
    if ((rc = c->order.wait_last(kl_err)) != KL_OK) return rc;  // the staging arrays may still be read
    if ((size_t)count > c->stage_scans) {
        c->mem.free(c->d_ranges);
        c->mem.free(c->d_poses);
        c->stage_scans = 0;
        c->mem.alloc(c->d_ranges, sizeof(double) * n * count);
        c->mem.alloc(c->d_poses, sizeof(double) * 3 * count);
        if (c->mem.error != hipSuccess) {
            const hipError_t e = c->mem.error;
            c->mem.error = hipSuccess;  // a smaller batch may still fit
            return kl_err.fail(KL_ENOMEM, "hipMalloc (scan staging)", e);
        }
        c->stage_scans = (size_t)count;
    }
    S2D_CHK(kl_err, KL_EHIP, hipMemcpyAsync(c->d_ranges, ranges, sizeof(double) * n * count, hipMemcpyHostToDevice, c->order.stream));
    S2D_CHK(kl_err, KL_EHIP, hipMemcpyAsync(c->d_poses, poses, sizeof(double) * 3 * count, hipMemcpyHostToDevice, c->order.stream));
    if ((rc = run_reference(c, g, first, count, c->d_ranges, c->d_poses, call)) != KL_OK) return rc;
    S2D_CHK(kl_err, KL_EHIP, hipStreamSynchronize(c->order.stream));
    return KL_OK;
}

int kl_get_reference(kl_ctx *c, int g, int first, int count, double *out)
{
    int rc = check_scan_range(c, g, first, count);
    if (rc != KL_OK) return rc;
    if (!out) return kl_err.fail(KL_EINVAL, "out is NULL");
    if (count == 0) return KL_OK;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = c->order.wait_last(kl_err)) != KL_OK) return rc;
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(out, c->dev.ref + (size_t)g * c->N + first, sizeof(double2) * count, hipMemcpyDeviceToHost));
    return KL_OK;
}

int kl_refresh_device(kl_ctx *c, int n_rows, const kl_refresh_row *d_rows, const double *d_pool_ranges,
                      const double *d_pool_poses, int pool_scans, kl_refresh_span *d_resolved_out, void *hip_stream)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (n_rows < 0 || pool_scans < 0) return kl_err.fail(KL_EINVAL, "negative count");
    if (n_rows > KL_REFRESH_MAX_ROWS) return kl_err.fail(KL_ERANGE, "more than KL_REFRESH_MAX_ROWS (4096) rows");
    if (n_rows == 0) return KL_OK;
    if (!d_rows || !d_pool_ranges || !d_pool_poses) return kl_err.fail(KL_EINVAL, "NULL argument");
    StreamCall call(c->order, kl_err, hip_stream);
    int rc = upload_dirty(c);  // an open row reads its graph's scan count from the device header
    if (rc != KL_OK) return rc;
    c->refresh.bump();
    if ((rc = call.begin()) != KL_OK) return rc;
    // the host knows no row, so the launch is sized by what the rows can name at most
    const int grid = refresh_grid(c->refresh_opt, c->num_cus, refresh_bound(n_rows, c->N));
    const KlRefresh r{d_rows, d_pool_ranges, d_pool_poses, (int2 *)d_resolved_out, c->refresh.d_info,
                      n_rows, pool_scans, c->G, c->refresh.seq};
    KL_LAUNCH(L_REFRESH, kl_refresh_kernel, dim3((unsigned)grid), dim3(KL_THREADS), 0, call.s, c->dev, r);
    return call.done();
}

int kl_get_refresh_info(kl_ctx *c, int *n_refused, int *first_status)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    const int rc = c->order.wait_last(kl_err);
    return rc != KL_OK ? rc : c->refresh.read_and_reset(kl_err, n_refused, first_status);
}

int kl_search_device(kl_ctx *c, int count, const kl_query *d_queries, void *hip_stream)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (count < 0 || count > c->Q) return kl_err.fail(KL_EINVAL, "count exceeds max_queries");
    if (count == 0) return KL_OK;
    if (!d_queries) return kl_err.fail(KL_EINVAL, "d_queries is NULL");
    StreamCall call(c->order, kl_err, hip_stream);
    return run_search(c, count, d_queries, call);
}

int kl_search(kl_ctx *c, int count, const kl_query *queries)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (count < 0 || count > c->Q) return kl_err.fail(KL_EINVAL, "count exceeds max_queries");
    if (count == 0) return KL_OK;
    if (!queries) return kl_err.fail(KL_EINVAL, "queries is NULL");
    StreamCall call(c->order, kl_err, nullptr);
    int rc = c->order.wait_last(kl_err);  // d_qin may still be read
    if (rc != KL_OK) return rc;
    S2D_CHK(kl_err, KL_EHIP, hipMemcpyAsync(c->d_qin, queries, sizeof(kl_query) * count, hipMemcpyHostToDevice, c->order.stream));
    if ((rc = run_search(c, count, c->d_qin, call)) != KL_OK) return rc;
    S2D_CHK(kl_err, KL_EHIP, hipStreamSynchronize(c->order.stream));
    return KL_OK;
}

int kl_get_result(kl_ctx *c, int slot, kl_result *result)
{
    int rc = check_slot(c, slot);
    if (rc != KL_OK) return rc;
    if (!result) return kl_err.fail(KL_EINVAL, "result is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = c->order.wait_last(kl_err)) != KL_OK) return rc;
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(result, c->dev.res + slot, sizeof(*result), hipMemcpyDeviceToHost));
    return KL_OK;
}

int kl_get_d2(kl_ctx *c, int slot, double *d2)
{
    kl_result r;
    int rc = kl_get_result(c, slot, &r);
    if (rc != KL_OK) return rc;
    if (d2 && r.status == KL_OK && r.n_scans > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(d2, c->dev.d2 + (size_t)slot * c->N, sizeof(double) * r.n_scans, hipMemcpyDeviceToHost));
    return KL_OK;
}

int kl_get_near(kl_ctx *c, int slot, int *near_link, int *near_loop)
{
    kl_result r;
    int rc = kl_get_result(c, slot, &r);
    if (rc != KL_OK) return rc;
    if (near_link && r.n_near_link > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(near_link, c->dev.near_link + (size_t)slot * c->N, sizeof(int) * r.n_near_link, hipMemcpyDeviceToHost));
    if (near_loop && r.n_near_loop > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(near_loop, c->dev.near_loop + (size_t)slot * c->N, sizeof(int) * r.n_near_loop, hipMemcpyDeviceToHost));
    return KL_OK;
}

int kl_get_chains(kl_ctx *c, int slot, kl_loop_chain *loop_chains, kl_near_chain *near_chains)
{
    kl_result r;
    int rc = kl_get_result(c, slot, &r);
    if (rc != KL_OK) return rc;
    const size_t cs = (size_t)c->dev.chain_stride;
    if (loop_chains && r.n_loop_chains > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(loop_chains, c->dev.loop_chains + slot * cs, sizeof(kl_loop_chain) * r.n_loop_chains, hipMemcpyDeviceToHost));
    if (near_chains && r.n_near_chains > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(near_chains, c->dev.near_chains + slot * cs, sizeof(kl_near_chain) * r.n_near_chains, hipMemcpyDeviceToHost));
    return KL_OK;
}

int kl_result_device(kl_ctx *c, const kl_result **d_results, const double **d_d2, const int **d_near_link,
                     const int **d_near_loop, const kl_loop_chain **d_loop_chains, const kl_near_chain **d_near_chains,
                     int *chain_stride)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (d_results) *d_results = c->dev.res;
    if (d_d2) *d_d2 = c->dev.d2;
    if (d_near_link) *d_near_link = c->dev.near_link;
    if (d_near_loop) *d_near_loop = c->dev.near_loop;
    if (d_loop_chains) *d_loop_chains = c->dev.loop_chains;
    if (d_near_chains) *d_near_chains = c->dev.near_chains;
    if (chain_stride) *chain_stride = c->dev.chain_stride;
    return KL_OK;
}

int kl_closest_device(kl_ctx *c, int count, const kl_closest_item *d_items, kl_closest *d_out, void *hip_stream)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (count < 0) return kl_err.fail(KL_EINVAL, "negative count");
    if (count == 0) return KL_OK;
    if (!d_items || !d_out) return kl_err.fail(KL_EINVAL, "NULL argument");
    StreamCall call(c->order, kl_err, hip_stream);
    int rc = upload_dirty(c);  // the kernel checks the items against the graphs' scan counts
    if (rc != KL_OK) return rc;
    if ((rc = call.begin()) != KL_OK) return rc;
    KL_LAUNCH(L_CLOSEST, kl_closest_kernel, dim3((unsigned)count), dim3(64), 0, call.s, c->dev, d_items, d_out, c->G);
    return call.done();
}

int kl_emit_batch_device(kl_ctx *c, int count, int which, int capacity, int *d_query_out, int *d_base_begin_out,
                         int *d_base_index_out, kl_source *d_source_out, int *d_n_matches, void *hip_stream)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (count < 0 || count > c->Q) return kl_err.fail(KL_EINVAL, "count exceeds max_queries");
    if (which != KL_LOOP_CHAINS && which != KL_NEAR_CHAINS) return kl_err.fail(KL_EINVAL, "which must be KL_LOOP_CHAINS or KL_NEAR_CHAINS");
    if (capacity < 0) return kl_err.fail(KL_EINVAL, "negative capacity");
    if (!d_base_begin_out || !d_n_matches || (capacity > 0 && (!d_query_out || !d_base_index_out || !d_source_out)))
        return kl_err.fail(KL_EINVAL, "NULL argument");
    StreamCall call(c->order, kl_err, hip_stream);
    int rc = upload_dirty(c);  // a pool offset set since the search
    if (rc != KL_OK) return rc;
    if ((rc = call.begin()) != KL_OK) return rc;
    KL_LAUNCH(L_EMIT_SCAN, kl_emit_scan_kernel, dim3(1), dim3(KL_THREADS), 0, call.s, c->dev, count, which, capacity,
              d_base_begin_out, d_n_matches);
    if (count > 0 && capacity > 0)
        KL_LAUNCH(L_EMIT_WRITE, kl_emit_write_kernel, dim3((unsigned)count), dim3(KL_THREADS), 0, call.s, c->dev, which,
                  capacity, d_query_out, d_base_begin_out, d_base_index_out, d_source_out);
    return call.done();
}

int kl_get_emit_info(kl_ctx *c, int *total_matches, int *status)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(kl_err);
    if (rc != KL_OK) return rc;
    int info[2] = {0, 0};
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(info, c->dev.emit_info, sizeof(info), hipMemcpyDeviceToHost));
    if (total_matches) *total_matches = info[0];
    if (status) *status = info[1];
    return KL_OK;
}

int kl_edit_vertices_device(kl_ctx *c, int count, const int *d_graph, const int *d_expect_id, int *d_id_out,
                            int *d_status_out, void *hip_stream)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (count < 0) return kl_err.fail(KL_EINVAL, "negative count");
    if (count == 0) return KL_OK;
    if (!d_graph) return kl_err.fail(KL_EINVAL, "d_graph is NULL");
    StreamCall call(c->order, kl_err, hip_stream);
    int rc = begin_edit(c, call);
    if (rc != KL_OK) return rc;
    KL_LAUNCH(L_EDIT_VERTICES, kl_edit_vertices_kernel, dim3((unsigned)count), dim3(GE_THREADS), 0, call.s, edit_args(c),
              count, d_graph, d_expect_id, d_id_out, d_status_out);
    return call.done();
}

int kl_edit_edges_device(kl_ctx *c, int count, const kl_edge_row *d_rows, int *d_is_new_out, int *d_status_out,
                         void *hip_stream)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    if (count < 0) return kl_err.fail(KL_EINVAL, "negative count");
    if (count == 0) return KL_OK;
    if (!d_rows) return kl_err.fail(KL_EINVAL, "d_rows is NULL");
    StreamCall call(c->order, kl_err, hip_stream);
    int rc = begin_edit(c, call);
    if (rc != KL_OK) return rc;
    const size_t lds = sizeof(int) * ((size_t)c->N + 1 + GE_THREADS + GE_WAVES + 1);
    KL_LAUNCH(L_EDIT_EDGES, kl_edit_edges_kernel, dim3((unsigned)count), dim3(GE_THREADS), lds, call.s, edit_args(c), count,
              d_rows, d_is_new_out, d_status_out);
    return call.done();
}

int kl_get_edit_info(kl_ctx *c, int *n_refused, int *first_status)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    const int rc = c->order.wait_last(kl_err);
    return rc != KL_OK ? rc : c->edit.read_and_reset(kl_err, n_refused, first_status);
}

int kl_download_graph(kl_ctx *c, int g, int *n_scans, int *n_edges, int *ends_out, int *adj_off_out, int *adj_out)
{
    int rc = check_graph(c, g);
    if (rc != KL_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = upload_dirty(c)) != KL_OK) return rc;
    if ((rc = c->order.wait_last(kl_err)) != KL_OK) return rc;
    KlHdr h{};
    S2D_CHK(kl_err, KL_EHIP, hipMemcpy(&h, c->d_hdr + g, sizeof(h), hipMemcpyDeviceToHost));
    if (h.n_scans < 0 || h.n_scans > c->N || h.n_edges < 0 || h.n_edges > c->M)
        return kl_err.fail(KL_EHIP, "the device header of the graph is out of range");
    if (n_scans) *n_scans = h.n_scans;
    if (n_edges) *n_edges = h.n_edges;
    const size_t N = (size_t)c->N, M = (size_t)c->M;
    if (ends_out && h.n_edges > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(ends_out, c->d_ends + g * M, sizeof(int2) * h.n_edges, hipMemcpyDeviceToHost));
    if (adj_off_out) {
        if (h.n_scans > 0) S2D_CHK(kl_err, KL_EHIP, hipMemcpy(adj_off_out, c->d_adj_off + g * (N + 1), sizeof(int) * (h.n_scans + 1), hipMemcpyDeviceToHost));
        else adj_off_out[0] = 0;  // a graph without scans has no list on the device
    }
    if (adj_out && h.n_edges > 0)
        S2D_CHK(kl_err, KL_EHIP, hipMemcpy(adj_out, c->d_adj + g * 2 * M, sizeof(int2) * 2 * h.n_edges, hipMemcpyDeviceToHost));
    return KL_OK;
}

int kl_set_timing(kl_ctx *c, int enable)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return set_timing(c->timer, enable);
}

int kl_num_kernels(void) { return L_NUM; }
const char *kl_kernel_name(int i) { return kernel_name(l_names, L_NUM, i); }

int kl_get_kernel_times(kl_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return kl_err.fail(KL_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return get_kernel_times(c->timer, kl_err, ms_out, launches_out, reset, L_NUM);
}

}  // extern "C"
