// karto_process_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_process.h) of the Karto
// scan-intake stage.  The decisions, the joining arrays and the running-scan buffer are computed in
// karto_process_kernels.hip; kp_commit_vertices turns the intake records into AddVertex / AddNode calls on the two
// host-mirrored graphs (karto_process_commit.h).  Without a usable HIP device kp_create fails with KP_ENODEV (no CPU
// fallback).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_process_commit.h"
#include "karto_process_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError kp_err;
S2D_ASSERT_STATUS_CODES(KP);

enum { P_INTAKE, P_COMPACT, P_STORE, P_APPLY, P_BIND_NEAR, P_ADVANCE, P_NUM };
const char *const p_names[P_NUM] = {"kp_intake_kernel", "kp_compact_kernel", "kp_store_kernel",
                                    "kp_apply_kernel", "kp_bind_near_kernel", "kp_advance_kernel"};
static_assert(P_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
}  // namespace

struct kp_ctx {
    int G = 0, n_readings = 0, max_scans = 0;
    kp_params params{};
    KpPlan plan;
    std::vector<int> pool_offset;
    int *d_pool_offset = nullptr;    // [G]
    kp_state *d_state = nullptr;     // [G]
    kp_intake *d_rec = nullptr;      // [G]: candidate i of the last intake
    kp_advanced *d_adv = nullptr;    // [G]
    KpPending *d_pending = nullptr;  // [G]
    int *d_counts = nullptr;         // [2]: jobs, seq matches of the last intake
    int g_first = 0, count = 0, pool_scans = 0;  // the last intake's
    StreamOrder order;
    DeviceBuffers mem;
    KernelTimer timer;
};

namespace {

#define KP_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, kp_err.fail, KP_EHIP, call.s, which, __VA_ARGS__)

kp_state empty_state()
{
    kp_state s;
    memset(&s, 0, sizeof(s));
    return s;
}

int put_state(kp_ctx *c, int g, const kp_state &s)
{
    int rc = c->order.wait_last(kp_err);
    if (rc != KP_OK) return rc;
    S2D_CHK(kp_err, KP_EHIP, hipMemcpy(c->d_state + g, &s, sizeof(s), hipMemcpyHostToDevice));
    return KP_OK;
}

}  // namespace

extern "C" {

const char *kp_last_error(void) { return kp_err.c_str(); }
const char *kp_version(void) { return "slam2d-karto-process 1 (gfx950)"; }

void kp_default_params(kp_params *p)
{
    if (!p) return;
    // Mapper::InitializeParameters (lesson6/lib/open_karto/src/Mapper.cpp:1468-1515)
    p->minimum_time_interval = 3600;
    p->minimum_travel_distance = 0.2;
    p->minimum_travel_heading = 10.0 * 0.017453292519943295;  // math::DegreesToRadians(10): degrees * KT_PI_180
    p->scan_buffer_maximum_scan_distance = 20;
    p->scan_buffer_size = 70;
    p->inverted = 0;
}

void kp_node_params(kp_params *p)
{
    if (!p) return;
    // lesson6's mapper_params.yaml
    p->minimum_time_interval = 3600;
    p->minimum_travel_distance = 0.2;
    p->minimum_travel_heading = 0.174;
    p->scan_buffer_maximum_scan_distance = 100;
    p->scan_buffer_size = 110;
    p->inverted = 0;
}

int kp_destroy(kp_ctx *c)
{
    if (!c) return KP_OK;
    c->order.destroy();
    c->mem.free_all();
    c->timer.destroy();
    delete c;
    return KP_OK;
}

int kp_create(kp_ctx **out, const kp_params *params, int n_graphs, int n_readings, int max_scans, const int *pool_offset)
{
    if (!out) return kp_err.fail(KP_EINVAL, "out is NULL");
    *out = nullptr;
    kp_params p;
    if (params) p = *params;
    else kp_default_params(&p);
    KpPlan plan;
    if (const char *why = kp_check_create(p, n_graphs, n_readings, max_scans, pool_offset, plan)) return kp_err.fail(KP_EINVAL, why);
    int poison = 0;
    if (const char *why = poison_from_env(poison)) return kp_err.fail(KP_EINVAL, why);
    if (!device_present()) return kp_err.fail(KP_ENODEV, "no HIP device");
    kp_ctx *c = new kp_ctx;
    c->G = n_graphs;
    c->n_readings = n_readings;
    c->max_scans = max_scans;
    c->params = p;
    c->plan = plan;
    c->pool_offset.resize((size_t)n_graphs);
    for (int g = 0; g < n_graphs; ++g) c->pool_offset[(size_t)g] = pool_offset ? pool_offset[g] : g * max_scans;
    hipError_t e;
    if ((e = c->order.create()) != hipSuccess) {
        kp_destroy(c);
        return kp_err.fail(KP_EHIP, "hipStreamCreate", e);
    }
    const size_t G = (size_t)n_graphs;
    c->mem.alloc(c->d_pool_offset, sizeof(int) * G);
    c->mem.alloc(c->d_state, sizeof(kp_state) * G);
    c->mem.alloc(c->d_rec, sizeof(kp_intake) * G);
    c->mem.alloc(c->d_adv, sizeof(kp_advanced) * G);
    c->mem.alloc(c->d_pending, sizeof(KpPending) * G);
    c->mem.alloc(c->d_counts, sizeof(int) * 2);
    if ((e = c->mem.error) != hipSuccess) {
        kp_destroy(c);
        return kp_err.fail(KP_ENOMEM, "hipMalloc", e);
    }
    const int fill = poison ? 0xA5 : 0;
    if ((e = hipMemcpyAsync(c->d_pool_offset, c->pool_offset.data(), sizeof(int) * G, hipMemcpyHostToDevice, c->order.stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_state, 0, sizeof(kp_state) * G, c->order.stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_rec, fill, sizeof(kp_intake) * G, c->order.stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_adv, fill, sizeof(kp_advanced) * G, c->order.stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_pending, 0, sizeof(KpPending) * G, c->order.stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_counts, 0, sizeof(int) * 2, c->order.stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->order.stream)) != hipSuccess || (e = hipEventRecord(c->order.ev_last, c->order.stream)) != hipSuccess) {
        kp_destroy(c);
        return kp_err.fail(KP_EHIP, "initialising the context", e);
    }
    *out = c;
    return KP_OK;
}

int kp_intake_device(kp_ctx *c, int g_first, int count, const kp_candidate *d_candidates, const float *d_ranges_f32,
                     int n_rows, double *d_pool_ranges, double *d_pool_poses, int pool_scans, int *d_query,
                     int *d_base_begin, int *d_base_index, int base_capacity, int *d_n_seq, ke_job *d_jobs,
                     kl_query *d_queries, int *d_n_jobs, kl_closest_item *d_closest_items, void *hip_stream)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (g_first < 0 || count < 0 || g_first > c->G - count) return kp_err.fail(KP_EINVAL, "graphs out of range");
    if (n_rows < 0 || pool_scans < 1 || base_capacity < 0) return kp_err.fail(KP_EINVAL, "negative size");
    if ((long long)base_capacity < (long long)count * c->plan.window_max)
        return kp_err.fail(KP_EINVAL, "base_capacity is below count * min(scan_buffer_size, max_scans)");
    if (count == 0) return KP_OK;
    if (!d_candidates || !d_pool_ranges || !d_pool_poses || !d_query || !d_base_begin || !d_base_index || !d_n_seq || !d_n_jobs ||
        (n_rows > 0 && !d_ranges_f32))
        return kp_err.fail(KP_EINVAL, "NULL argument");
    StreamCall call(c->order, kp_err, hip_stream);
    int rc = call.begin();
    if (rc != KP_OK) return rc;
    KpArgs a{};
    a.g_first = g_first;
    a.count = count;
    a.n_rows = n_rows;
    a.pool_scans = pool_scans;
    a.max_scans = c->max_scans;
    a.n_readings = c->n_readings;
    a.inverted = c->params.inverted;
    a.base_capacity = base_capacity;
    a.gate.min_time = c->params.minimum_time_interval;
    a.gate.min_heading = c->params.minimum_travel_heading;
    a.gate.thr_travel = c->plan.thr_travel;
    a.cand = d_candidates;
    a.ranges_f32 = d_ranges_f32;
    a.state = c->d_state;
    a.pool_offset = c->d_pool_offset;
    a.pool_ranges = d_pool_ranges;
    a.pool_poses = d_pool_poses;
    a.rec = c->d_rec;
    a.pending = c->d_pending;
    a.query = d_query;
    a.base_begin = d_base_begin;
    a.base_index = d_base_index;
    a.n_seq = d_n_seq;
    a.n_jobs = d_n_jobs;
    a.counts = c->d_counts;
    a.jobs = d_jobs;
    a.queries = d_queries;
    a.items = d_closest_items;
    c->g_first = g_first;
    c->count = count;
    c->pool_scans = pool_scans;
    const unsigned blocks = (unsigned)((count + KP_PER_BLOCK - 1) / KP_PER_BLOCK);
    KP_LAUNCH(P_INTAKE, kp_intake_kernel, dim3(blocks), dim3(KP_THREADS), 0, call.s, a);
    KP_LAUNCH(P_COMPACT, kp_compact_kernel, dim3(1), dim3(KP_THREADS), 0, call.s, a);
    KP_LAUNCH(P_STORE, kp_store_kernel, dim3((unsigned)count), dim3(KP_THREADS), 0, call.s, a);
    return call.done();
}

int kp_apply_match_device(kp_ctx *c, const kt_result *d_seq, int n_seq, double *d_pool_poses, int pool_scans, void *hip_stream)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (n_seq < 0) return kp_err.fail(KP_EINVAL, "negative size");
    if (c->count == 0) return KP_OK;
    if (pool_scans != c->pool_scans) return kp_err.fail(KP_EINVAL, "pool_scans differs from the last intake's");
    if (!d_pool_poses || (n_seq > 0 && !d_seq)) return kp_err.fail(KP_EINVAL, "NULL argument");
    StreamCall call(c->order, kp_err, hip_stream);
    int rc = call.begin();
    if (rc != KP_OK) return rc;
    KP_LAUNCH(P_APPLY, kp_apply_kernel, dim3((unsigned)((c->count + 63) / 64)), dim3(64), 0, call.s, c->g_first, c->count,
              n_seq, pool_scans, c->d_pool_offset, d_seq, c->d_rec, d_pool_poses);
    return call.done();
}

int kp_get_intake(kp_ctx *c, int first, int count, kp_intake *out, kp_advanced *advanced_out)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (first < 0 || count < 0 || first > c->G - count) return kp_err.fail(KP_EINVAL, "records out of range");
    if (count == 0) return KP_OK;
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(kp_err);
    if (rc != KP_OK) return rc;
    if (out)
        S2D_CHK(kp_err, KP_EHIP, hipMemcpy(out, c->d_rec + first, sizeof(kp_intake) * (size_t)count, hipMemcpyDeviceToHost));
    if (advanced_out)
        S2D_CHK(kp_err, KP_EHIP,
                hipMemcpy(advanced_out, c->d_adv + first, sizeof(kp_advanced) * (size_t)count, hipMemcpyDeviceToHost));
    return KP_OK;
}

int kp_commit_vertices(kp_ctx *c, kl_ctx *kl, spa_ctx *spa, int *n_added)
{
    if (n_added) *n_added = 0;
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (!kl) return kp_err.fail(KP_EINVAL, "kl is NULL");
    if (c->count == 0) return KP_OK;
    std::vector<kp_intake> recs((size_t)c->count);
    int rc = kp_get_intake(c, 0, c->count, recs.data(), nullptr);
    if (rc != KP_OK) return rc;
    std::string why;
    bool mismatch = false;
    const int n = kp_plan_vertices(
        recs.data(), c->count, c->g_first,
        [&](int g, int &id) {
            if (kl_add_vertex(kl, g, &id) != KL_OK) {
                why = std::string("kl_add_vertex: ") + kl_last_error();
                return false;
            }
            return true;
        },
        [&](int g, int scan, const double *pose) {
            if (spa && spa_add_node(spa, g, scan, pose) != SPA_OK) {
                why = std::string("spa_add_node: ") + spa_last_error();
                return false;
            }
            return true;
        },
        &mismatch);
    if (n_added) *n_added = n >= 0 ? n : -(n + 1);
    if (n < 0)
        return kp_err.fail(KP_EINVAL, mismatch ? "the graph's scan count differs from the intake's scan index" : why.c_str());
    return KP_OK;
}

int kp_bind_near_device(kp_ctx *c, ke_job *d_jobs, const kl_source *d_source, const int *d_n_matches, int max_matches, void *hip_stream)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (max_matches < 0) return kp_err.fail(KP_EINVAL, "negative size");
    if (c->count == 0) return KP_OK;
    if (!d_jobs || !d_n_matches || (max_matches > 0 && !d_source)) return kp_err.fail(KP_EINVAL, "NULL argument");
    StreamCall call(c->order, kp_err, hip_stream);
    int rc = call.begin();
    if (rc != KP_OK) return rc;
    KP_LAUNCH(P_BIND_NEAR, kp_bind_near_kernel, dim3((unsigned)((c->count + 63) / 64)), dim3(64), 0, call.s, c->d_counts,
              c->count, d_jobs, d_source, d_n_matches, max_matches);
    return call.done();
}

int kp_advance_device(kp_ctx *c, const double *d_pool_poses, int pool_scans, void *hip_stream)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (c->count == 0) return KP_OK;
    if (pool_scans != c->pool_scans) return kp_err.fail(KP_EINVAL, "pool_scans differs from the last intake's");
    if (!d_pool_poses) return kp_err.fail(KP_EINVAL, "NULL argument");
    StreamCall call(c->order, kp_err, hip_stream);
    int rc = call.begin();
    if (rc != KP_OK) return rc;
    KpAdvanceArgs a{};
    a.g_first = c->g_first;
    a.count = c->count;
    a.pool_scans = pool_scans;
    a.buffer_size = c->params.scan_buffer_size;
    a.thr_buffer = c->plan.thr_buffer;
    a.pool_offset = c->d_pool_offset;
    a.pool_poses = d_pool_poses;
    a.rec = c->d_rec;
    a.pending = c->d_pending;
    a.state = c->d_state;
    a.adv = c->d_adv;
    const unsigned blocks = (unsigned)((c->count + KP_PER_BLOCK - 1) / KP_PER_BLOCK);
    KP_LAUNCH(P_ADVANCE, kp_advance_kernel, dim3(blocks), dim3(KP_THREADS), 0, call.s, a);
    return call.done();
}

int kp_result_device(kp_ctx *c, const kp_intake **d_intake, const kp_advanced **d_advanced, const kp_state **d_state,
                     const int **d_counts)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (d_intake) *d_intake = c->d_rec;
    if (d_advanced) *d_advanced = c->d_adv;
    if (d_state) *d_state = c->d_state;
    if (d_counts) *d_counts = c->d_counts;
    return KP_OK;
}

int kp_get_state(kp_ctx *c, int g, kp_state *out)
{
    if (!c || !out) return kp_err.fail(KP_EINVAL, "NULL argument");
    if (g < 0 || g >= c->G) return kp_err.fail(KP_EINVAL, "graph out of range");
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(kp_err);
    if (rc != KP_OK) return rc;
    S2D_CHK(kp_err, KP_EHIP, hipMemcpy(out, c->d_state + g, sizeof(kp_state), hipMemcpyDeviceToHost));
    return KP_OK;
}

int kp_set_state(kp_ctx *c, int g, const kp_state *state)
{
    if (!c || !state) return kp_err.fail(KP_EINVAL, "NULL argument");
    if (g < 0 || g >= c->G) return kp_err.fail(KP_EINVAL, "graph out of range");
    if (!kp_state_valid(*state, c->max_scans, c->params.scan_buffer_size))
        return kp_err.fail(KP_EINVAL, "the running scans must be a tail of the scans, at most scan_buffer_size long");
    std::lock_guard<std::mutex> lock(c->order.mu);
    kp_state s = *state;
    s.pad_ = 0;
    return put_state(c, g, s);
}

int kp_clear_graph(kp_ctx *c, int g)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    if (g < 0 || g >= c->G) return kp_err.fail(KP_EINVAL, "graph out of range");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return put_state(c, g, empty_state());
}

int kp_set_timing(kp_ctx *c, int enable)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return set_timing(c->timer, enable);
}

int kp_num_kernels(void) { return P_NUM; }
const char *kp_kernel_name(int i) { return kernel_name(p_names, P_NUM, i); }

int kp_get_kernel_times(kp_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return kp_err.fail(KP_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return get_kernel_times(c->timer, kp_err, ms_out, launches_out, reset, P_NUM);
}

}  // extern "C"
