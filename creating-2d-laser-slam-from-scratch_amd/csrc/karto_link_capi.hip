// karto_link_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_link.h) of the Karto graph-linking
// stage.  The decisions, constraints and corrected poses are computed in karto_link_kernels.hip; ke_commit turns the
// link records into edits of the two host-mirrored graphs (karto_link_commit.h).  Without a usable HIP device
// ke_create fails with KE_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_link_commit.h"
#include "karto_link_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError ke_err;
S2D_ASSERT_STATUS_CODES(KE);

constexpr int KE_MAX_JOBS = 1 << 20;
constexpr int KE_MAX_MATCHES = 1 << 24;

enum { E_ADD_EDGES, E_COARSE_SCAN, E_COARSE_WRITE, E_FINE, E_CLOSE, E_NUM };
const char *const e_names[E_NUM] = {"ke_add_edges_kernel", "ke_coarse_scan_kernel", "ke_coarse_write_kernel",
                                    "ke_fine_kernel", "ke_close_kernel"};
static_assert(E_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
}  // namespace

struct ke_ctx {
    int J = 0, K = 0, M = 0, n_readings = 0;
    ke_params params{};
    double link_threshold = 0;
    ke_link *d_links = nullptr;     // [J][K]
    ke_job_out *d_out = nullptr;    // [J]
    int *d_info = nullptr;          // [2]: the last coarse call's accepted count and status
    StreamOrder order;
    DeviceBuffers mem;
    KernelTimer timer;
};

namespace {

#define KE_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, ke_err.fail, KE_EHIP, call.s, which, __VA_ARGS__)

int check_rows(ke_ctx *c, int first_job, int count)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    if (first_job < 0 || count < 0 || first_job > c->J - count) return ke_err.fail(KE_EINVAL, "job rows out of range");
    return KE_OK;
}

}  // namespace

extern "C" {

const char *ke_last_error(void) { return ke_err.c_str(); }
const char *ke_version(void) { return "slam2d-karto-link 1 (gfx950)"; }

void ke_default_params(ke_params *p)
{
    if (!p) return;
    // Mapper::InitializeParameters (lesson6/lib/open_karto/src/Mapper.cpp:1517-1564)
    p->link_match_minimum_response_fine = 0.8;
    p->loop_match_minimum_response_coarse = 0.8;
    p->loop_match_maximum_variance_coarse = 0.4 * 0.4;  // math::Square(0.4)
    p->loop_match_minimum_response_fine = 0.8;
}

void ke_node_params(ke_params *p)
{
    if (!p) return;
    // lesson6's mapper_params.yaml:37-44, the variance through setParamLoopMatchMaximumVarianceCoarse
    p->link_match_minimum_response_fine = 0.1;
    p->loop_match_minimum_response_coarse = 0.35;
    p->loop_match_maximum_variance_coarse = 3.0 * 3.0;
    p->loop_match_minimum_response_fine = 0.45;
}

int ke_destroy(ke_ctx *c)
{
    if (!c) return KE_OK;
    c->order.destroy();
    c->mem.free_all();
    c->timer.destroy();
    delete c;
    return KE_OK;
}

int ke_create(ke_ctx **out, const ke_params *params, int n_readings, int max_jobs, int max_links, int max_matches)
{
    if (!out) return ke_err.fail(KE_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_readings < 1 || n_readings > 4096) return ke_err.fail(KE_EINVAL, "need 1 <= n_readings <= 4096");
    if (max_jobs < 1 || max_jobs > KE_MAX_JOBS || max_matches < 1 || max_matches > KE_MAX_MATCHES)
        return ke_err.fail(KE_EINVAL, "need 1 <= max_jobs <= 2^20 and 1 <= max_matches <= 2^24");
    if (max_links < 1) return ke_err.fail(KE_EINVAL, "need max_links >= 1");
    if (max_links > KE_MAX_LINKS) return ke_err.fail(KE_ERANGE, "max_links exceeds KE_MAX_LINKS (64)");
    ke_params p;
    if (params) p = *params;
    else ke_default_params(&p);
    if (std::isnan(p.link_match_minimum_response_fine) || std::isnan(p.loop_match_minimum_response_coarse) ||
        std::isnan(p.loop_match_maximum_variance_coarse) || std::isnan(p.loop_match_minimum_response_fine))
        return ke_err.fail(KE_EINVAL, "a parameter is NaN");
    int poison = 0;
    if (const char *why = poison_from_env(poison)) return ke_err.fail(KE_EINVAL, why);
    if (!device_present()) return ke_err.fail(KE_ENODEV, "no HIP device");
    ke_ctx *c = new ke_ctx;
    c->J = max_jobs;
    c->K = max_links;
    c->M = max_matches;
    c->n_readings = n_readings;
    c->params = p;
    c->link_threshold = p.link_match_minimum_response_fine - KL_TOLERANCE;  // Mapper.cpp:1141
    hipError_t e;
    if ((e = c->order.create()) != hipSuccess) {
        ke_destroy(c);
        return ke_err.fail(KE_EHIP, "hipStreamCreate", e);
    }
    const size_t nl = sizeof(ke_link) * (size_t)max_jobs * max_links, no = sizeof(ke_job_out) * (size_t)max_jobs;
    c->mem.alloc(c->d_links, nl);
    c->mem.alloc(c->d_out, no);
    c->mem.alloc(c->d_info, sizeof(int) * 2);
    if ((e = c->mem.error) != hipSuccess) {
        ke_destroy(c);
        return ke_err.fail(KE_ENOMEM, "hipMalloc", e);
    }
    // no row holds a result yet: n_links 0, status KE_EINVAL
    std::vector<ke_job_out> o0((size_t)max_jobs);
    for (auto &o : o0) {
        memset(&o, 0, sizeof(o));
        o.status = KE_EINVAL;
    }
    if ((e = hipMemsetAsync(c->d_links, poison ? 0xA5 : 0, nl, c->order.stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_info, 0, sizeof(int) * 2, c->order.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->d_out, o0.data(), no, hipMemcpyHostToDevice, c->order.stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->order.stream)) != hipSuccess || (e = hipEventRecord(c->order.ev_last, c->order.stream)) != hipSuccess) {
        ke_destroy(c);
        return ke_err.fail(KE_EHIP, "initialising the context", e);
    }
    *out = c;
    return KE_OK;
}

int ke_add_edges_device(ke_ctx *c, int count, const ke_job *d_jobs, double *d_pool_poses, int pool_scans,
                        const kt_result *d_seq, int n_seq, const kl_closest *d_running, int n_running,
                        const kt_result *d_near, const kl_source *d_near_source, int n_near,
                        const kl_near_chain *d_near_chains, int chain_stride, int n_slots, int flags, void *hip_stream)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    if (count < 0 || count > c->J) return ke_err.fail(KE_EINVAL, "count exceeds max_jobs");
    if (pool_scans < 1 || n_seq < 0 || n_running < 0 || n_near < 0 || chain_stride < 0 || n_slots < 0)
        return ke_err.fail(KE_EINVAL, "negative size");
    if (flags & ~KE_WRITE_POSE) return ke_err.fail(KE_EINVAL, "unknown flag");
    if (count == 0) return KE_OK;
    if (!d_jobs || !d_pool_poses || (n_seq > 0 && !d_seq) || (n_running > 0 && !d_running) ||
        (n_near > 0 && (!d_near || !d_near_source || !d_near_chains)))
        return ke_err.fail(KE_EINVAL, "NULL argument");
    StreamCall call(c->order, ke_err, hip_stream);
    int rc = call.begin();
    if (rc != KE_OK) return rc;
    KeAddArgs a{};
    a.count = count;
    a.max_links = c->K;
    a.pool_scans = pool_scans;
    a.n_seq = n_seq;
    a.n_running = n_running;
    a.n_near = n_near;
    a.chain_stride = chain_stride;
    a.n_slots = n_slots;
    a.flags = flags;
    a.link_threshold = c->link_threshold;
    a.jobs = d_jobs;
    a.pool_poses = d_pool_poses;
    a.seq = d_seq;
    a.running = d_running;
    a.near = d_near;
    a.near_source = d_near_source;
    a.near_chains = d_near_chains;
    a.links = c->d_links;
    a.out = c->d_out;
    const unsigned blocks = (unsigned)((count + KE_JOBS_PER_BLOCK - 1) / KE_JOBS_PER_BLOCK);
    KE_LAUNCH(E_ADD_EDGES, ke_add_edges_kernel, dim3(blocks), dim3(KE_THREADS), 0, call.s, a);
    return call.done();
}

int ke_loop_coarse_device(ke_ctx *c, int max_matches, const int *d_n_matches, const kt_result *d_coarse,
                          const int *d_query, const int *d_base_begin, const int *d_base_index,
                          const double *d_pool_ranges, int pool_scans, int tmp_first, int capacity, int base_capacity,
                          int *d_fine_query, int *d_fine_base_begin, int *d_fine_base_index, int *d_fine_of, int *d_n_fine,
                          double *d_tmp_ranges, double *d_tmp_poses, void *hip_stream)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    if (max_matches < 0 || max_matches > c->M) return ke_err.fail(KE_EINVAL, "max_matches exceeds the context's");
    if (pool_scans < 1 || capacity < 0 || base_capacity < 0) return ke_err.fail(KE_EINVAL, "negative size");
    if (tmp_first < 0 || tmp_first > INT_MAX - capacity) return ke_err.fail(KE_EINVAL, "tmp_first out of range");
    if (!d_n_matches || !d_fine_base_begin || !d_n_fine) return ke_err.fail(KE_EINVAL, "NULL argument");
    if (max_matches > 0 && (!d_coarse || !d_query || !d_base_begin || !d_base_index || !d_pool_ranges))
        return ke_err.fail(KE_EINVAL, "NULL argument");
    if (capacity > 0 && (!d_fine_query || !d_fine_of || !d_tmp_ranges || !d_tmp_poses || (base_capacity > 0 && !d_fine_base_index)))
        return ke_err.fail(KE_EINVAL, "NULL argument");
    StreamCall call(c->order, ke_err, hip_stream);
    int rc = call.begin();
    if (rc != KE_OK) return rc;
    KeCoarseArgs a{};
    a.max_matches = max_matches;
    a.pool_scans = pool_scans;
    a.tmp_first = tmp_first;
    a.capacity = capacity;
    a.base_capacity = base_capacity;
    a.n_readings = c->n_readings;
    a.min_coarse = c->params.loop_match_minimum_response_coarse;
    a.max_var = c->params.loop_match_maximum_variance_coarse;
    a.n_matches = d_n_matches;
    a.coarse = d_coarse;
    a.query = d_query;
    a.base_begin = d_base_begin;
    a.base_index = d_base_index;
    a.pool_ranges = d_pool_ranges;
    a.fine_query = d_fine_query;
    a.fine_base_begin = d_fine_base_begin;
    a.fine_base_index = d_fine_base_index;
    a.fine_of = d_fine_of;
    a.n_fine = d_n_fine;
    a.tmp_ranges = d_tmp_ranges;
    a.tmp_poses = d_tmp_poses;
    a.info = c->d_info;
    KE_LAUNCH(E_COARSE_SCAN, ke_coarse_scan_kernel, dim3(1), dim3(KE_THREADS), 0, call.s, a);
    if (capacity > 0)
        KE_LAUNCH(E_COARSE_WRITE, ke_coarse_write_kernel, dim3((unsigned)capacity), dim3(KE_THREADS), 0, call.s, a);
    return call.done();
}

int ke_get_loop_info(ke_ctx *c, int *total_accepted, int *status)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(ke_err);
    if (rc != KE_OK) return rc;
    int info[2] = {0, 0};
    S2D_CHK(ke_err, KE_EHIP, hipMemcpy(info, c->d_info, sizeof(info), hipMemcpyDeviceToHost));
    if (total_accepted) *total_accepted = info[0];
    if (status) *status = info[1];
    return KE_OK;
}

int ke_loop_fine_device(ke_ctx *c, int count, int capacity, const int *d_n_fine, const kt_result *d_fine,
                        const int *d_fine_of, int max_matches, const kl_source *d_source, const int *d_query,
                        const kl_loop_chain *d_loop_chains, int chain_stride, ke_closure *d_closures,
                        double *d_pool_poses, int pool_scans, int flags, void *hip_stream)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    if (count < 0 || capacity < 0 || max_matches < 0 || chain_stride < 0 || pool_scans < 0)
        return ke_err.fail(KE_EINVAL, "negative size");
    if (max_matches > c->M) return ke_err.fail(KE_EINVAL, "max_matches exceeds the context's");
    if (flags & ~KE_WRITE_POSE) return ke_err.fail(KE_EINVAL, "unknown flag");
    if (count == 0) return KE_OK;
    if (!d_n_fine || !d_closures || (capacity > 0 && (!d_fine || !d_fine_of || !d_source || !d_loop_chains)))
        return ke_err.fail(KE_EINVAL, "NULL argument");
    if ((flags & KE_WRITE_POSE) && (!d_query || !d_pool_poses)) return ke_err.fail(KE_EINVAL, "KE_WRITE_POSE without d_query or d_pool_poses");
    StreamCall call(c->order, ke_err, hip_stream);
    int rc = call.begin();
    if (rc != KE_OK) return rc;
    KeFineArgs a{};
    a.count = count;
    a.capacity = capacity;
    a.max_matches = max_matches;
    a.chain_stride = chain_stride;
    a.pool_scans = pool_scans;
    a.flags = flags;
    a.min_fine = c->params.loop_match_minimum_response_fine;
    a.n_fine = d_n_fine;
    a.fine = d_fine;
    a.fine_of = d_fine_of;
    a.source = d_source;
    a.query = d_query;
    a.loop_chains = d_loop_chains;
    a.closures = d_closures;
    a.pool_poses = d_pool_poses;
    KE_LAUNCH(E_FINE, ke_fine_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, call.s, a);
    return call.done();
}

int ke_close_device(ke_ctx *c, int count, const ke_job *d_jobs, const ke_closure *d_closures, const kl_closest *d_closest,
                    const double *d_pool_poses, int pool_scans, void *hip_stream)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    if (count < 0 || count > c->J) return ke_err.fail(KE_EINVAL, "count exceeds max_jobs");
    if (pool_scans < 1) return ke_err.fail(KE_EINVAL, "negative size");
    if (count == 0) return KE_OK;
    if (!d_jobs || !d_closures || !d_closest || !d_pool_poses) return ke_err.fail(KE_EINVAL, "NULL argument");
    StreamCall call(c->order, ke_err, hip_stream);
    int rc = call.begin();
    if (rc != KE_OK) return rc;
    KE_LAUNCH(E_CLOSE, ke_close_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, call.s, count, c->K, pool_scans,
              d_jobs,
              d_closures, d_closest, d_pool_poses, c->d_links, c->d_out);
    return call.done();
}

int ke_get_links(ke_ctx *c, int first_job, int count, ke_link *links_out, ke_job_out *jobs_out)
{
    int rc = check_rows(c, first_job, count);
    if (rc != KE_OK) return rc;
    if (count == 0) return KE_OK;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = c->order.wait_last(ke_err)) != KE_OK) return rc;
    if (links_out)
        S2D_CHK(ke_err, KE_EHIP, hipMemcpy(links_out, c->d_links + (size_t)first_job * c->K, sizeof(ke_link) * (size_t)count * c->K, hipMemcpyDeviceToHost));
    if (jobs_out) S2D_CHK(ke_err, KE_EHIP, hipMemcpy(jobs_out, c->d_out + first_job, sizeof(ke_job_out) * (size_t)count, hipMemcpyDeviceToHost));
    return KE_OK;
}

int ke_result_device(ke_ctx *c, const ke_link **d_links, const ke_job_out **d_jobs_out, int *max_links)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    if (d_links) *d_links = c->d_links;
    if (d_jobs_out) *d_jobs_out = c->d_out;
    if (max_links) *max_links = c->K;
    return KE_OK;
}

int ke_commit(ke_ctx *c, kl_ctx *kl, spa_ctx *spa, int first_job, int count, int *n_new_edges)
{
    if (n_new_edges) *n_new_edges = 0;
    int rc = check_rows(c, first_job, count);
    if (rc != KE_OK) return rc;
    if (!kl) return ke_err.fail(KE_EINVAL, "kl is NULL");
    if (count == 0) return KE_OK;
    std::vector<ke_link> links((size_t)count * c->K);
    std::vector<ke_job_out> jobs((size_t)count);
    if ((rc = ke_get_links(c, first_job, count, links.data(), jobs.data())) != KE_OK) return rc;
    std::vector<KeAction> actions;
    std::string why;
    const bool ok = ke_plan_commit(jobs.data(), links.data(), count, c->K,
        [&](int g, int from, int to, bool &is_new) {
            int n = 0;
            if (kl_add_edge(kl, g, from, to, &n) != KL_OK) {
                why = std::string("kl_add_edge: ") + kl_last_error();
                return false;
            }
            is_new = n != 0;
            return true;
        },
        actions);
    int fresh = 0;
    for (const KeAction &a : actions) {
        if (!a.constraint) continue;
        ++fresh;
        if (!spa) continue;
        const ke_link &l = links[(size_t)a.job * c->K + a.record];
        if (spa_add_constraint(spa, a.graph, a.from, a.to, l.diff, l.precision, nullptr) != SPA_OK) {
            why = std::string("spa_add_constraint: ") + spa_last_error();
            if (n_new_edges) *n_new_edges = fresh;
            return ke_err.fail(KE_EINVAL, why.c_str());
        }
    }
    if (n_new_edges) *n_new_edges = fresh;
    return ok ? KE_OK : ke_err.fail(KE_EINVAL, why.c_str());
}

int ke_set_timing(ke_ctx *c, int enable)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return set_timing(c->timer, enable);
}

int ke_num_kernels(void) { return E_NUM; }
const char *ke_kernel_name(int i) { return kernel_name(e_names, E_NUM, i); }

int ke_get_kernel_times(ke_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return ke_err.fail(KE_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return get_kernel_times(c->timer, ke_err, ms_out, launches_out, reset, E_NUM);
}

}  // extern "C"
