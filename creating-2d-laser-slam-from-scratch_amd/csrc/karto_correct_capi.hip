// karto_correct_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_correct.h) of the Karto
// pose-correction stage: the scratch rows, the flatten launch of karto_correct_kernels.hip and, after it, the
// contexts' own row-indexed calls on the same stream.  Nothing here waits for the device but kc_get_info and
// kc_get_kernel_times.  Without a usable HIP device kc_create fails with KC_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_correct_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError kc_err;
S2D_ASSERT_STATUS_CODES(KC);
static_assert(KC_MAX_ROWS == KL_REFRESH_MAX_ROWS && KC_MAX_ROWS == KT_REFRESH_MAX_ROWS, "one call's rows fit both refreshes");

constexpr int KC_MAX_GRAPHS = 1 << 16;

enum { C_FLATTEN, C_NUM };
const char *const c_names[C_NUM] = {"kc_flatten_kernel"};
static_assert(C_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
}  // namespace

struct kc_ctx {
    int G = 0, N = 0, R = 0;
    int *d_pool_offset = nullptr;  // [G]
    kl_refresh_row *d_rows = nullptr;
    kl_refresh_span *d_spans = nullptr;
    int *d_graph = nullptr;
    int *d_info = nullptr;  // scans named, graphs corrected, records refused
    StreamOrder order;      // the scratch rows may still be read by the previous call's work on another stream
    DeviceBuffers mem;
    KernelTimer timer;
};

namespace {

#define KC_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, kc_err.fail, KC_EHIP, s, which, __VA_ARGS__)

// a driven context refused the call: its text behind the call's name
int refused(const std::string &why) { return kc_err.fail(KC_EINVAL, why.c_str()); }

int check_call(const kc_ctx *c, int count, const void *records, const double *d_pool_ranges, const double *d_pool_poses,
               int pool_scans)
{
    if (!c) return kc_err.fail(KC_EINVAL, "ctx is NULL");
    if (count < 0 || pool_scans < 0) return kc_err.fail(KC_EINVAL, "negative count");
    if (count > c->R) return kc_err.fail(KC_ERANGE, "more records than the context's max_rows");
    if (count > 0 && (!records || !d_pool_ranges || !d_pool_poses)) return kc_err.fail(KC_EINVAL, "NULL argument");
    return KC_OK;
}

int flatten(kc_ctx *c, hipStream_t s, KcFlatten f)
{
    f.pool_offset = c->d_pool_offset;
    f.rows = c->d_rows;
    f.spans = c->d_spans;
    f.graph = c->d_graph;
    f.info = c->d_info;
    f.n_graphs = c->G;
    f.max_scans = c->N;
    KC_LAUNCH(C_FLATTEN, kc_flatten_kernel, dim3((unsigned)((f.count + KC_THREADS - 1) / KC_THREADS)), dim3(KC_THREADS), 0, s, f);
    return KC_OK;
}

// the rows' scans in the loop-search context, then in each matcher with the rows that context resolved (without it:
// the flatten's own)
int refresh(kc_ctx *c, hipStream_t s, int count, kl_ctx *kl, kt_ctx *kt_seq, kt_ctx *kt_loop, const double *d_pool_ranges,
            const double *d_pool_poses, int pool_scans)
{
    if (kl && kl_refresh_device(kl, count, c->d_rows, d_pool_ranges, d_pool_poses, pool_scans, c->d_spans, s) != KL_OK)
        return refused(std::string("kl_refresh_device: ") + kl_last_error());
    for (kt_ctx *kt : {kt_seq, kt_loop})
        if (kt && kt_refresh_device(kt, count, c->d_spans, d_pool_ranges, d_pool_poses, pool_scans, s) != KT_OK)
            return refused(std::string("kt_refresh_device: ") + kt_last_error());
    return KC_OK;
}

}  // namespace

extern "C" {

const char *kc_last_error(void) { return kc_err.c_str(); }
const char *kc_version(void) { return "slam2d-karto-correct 1 (gfx950)"; }

int kc_destroy(kc_ctx *c)
{
    if (!c) return KC_OK;
    c->order.destroy();
    c->mem.free_all();
    c->timer.destroy();
    delete c;
    return KC_OK;
}

int kc_create(kc_ctx **out, int n_graphs, int max_scans, const int *pool_offset, int max_rows)
{
    if (!out) return kc_err.fail(KC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_graphs < 1 || n_graphs > KC_MAX_GRAPHS || max_scans < 1 || max_scans > KL_MAX_SCANS)
        return kc_err.fail(KC_EINVAL, "need 1 <= n_graphs <= 2^16 and 1 <= max_scans <= KL_MAX_SCANS");
    if (max_rows < 1 || max_rows > KC_MAX_ROWS) return kc_err.fail(KC_EINVAL, "need 1 <= max_rows <= KC_MAX_ROWS (4096)");
    std::vector<int> off((size_t)n_graphs);
    for (int g = 0; g < n_graphs; ++g) {
        const long long o = pool_offset ? pool_offset[g] : (long long)g * max_scans;
        if (o < 0 || o > INT_MAX - KL_MAX_SCANS) return kc_err.fail(KC_EINVAL, "pool offset out of range");
        off[g] = (int)o;
    }
    if (!device_present()) return kc_err.fail(KC_ENODEV, "no HIP device");
    kc_ctx *c = new kc_ctx;
    c->G = n_graphs;
    c->N = max_scans;
    c->R = max_rows;
    hipError_t e;
    if ((e = c->order.create()) != hipSuccess) {
        kc_destroy(c);
        return kc_err.fail(KC_EHIP, "hipStreamCreate", e);
    }
    c->mem.alloc(c->d_pool_offset, sizeof(int) * (size_t)n_graphs);
    c->mem.alloc(c->d_rows, sizeof(kl_refresh_row) * (size_t)max_rows);
    c->mem.alloc(c->d_spans, sizeof(kl_refresh_span) * (size_t)max_rows);
    c->mem.alloc(c->d_graph, sizeof(int) * (size_t)max_rows);
    c->mem.alloc(c->d_info, sizeof(int) * 3);
    if ((e = c->mem.error) != hipSuccess) {
        kc_destroy(c);
        return kc_err.fail(KC_ENOMEM, "hipMalloc", e);
    }
    hipStream_t s = c->order.stream;
    if ((e = hipMemsetAsync(c->d_info, 0, sizeof(int) * 3, s)) != hipSuccess ||
        (e = hipMemcpyAsync(c->d_pool_offset, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess || (e = hipEventRecord(c->order.ev_last, s)) != hipSuccess) {
        kc_destroy(c);
        return kc_err.fail(KC_EHIP, "initialising the context", e);
    }
    *out = c;
    return KC_OK;
}

int kc_refresh_intake_device(kc_ctx *c, const kp_intake *d_intake, int g_first, int count, kl_ctx *kl, kt_ctx *kt_seq,
                             kt_ctx *kt_loop, const double *d_pool_ranges, const double *d_pool_poses, int pool_scans,
                             void *hip_stream)
{
    int rc = check_call(c, count, d_intake, d_pool_ranges, d_pool_poses, pool_scans);
    if (rc != KC_OK) return rc;
    if (g_first < 0) return kc_err.fail(KC_EINVAL, "negative graph");
    if (count == 0) return KC_OK;
    StreamCall call(c->order, kc_err, hip_stream);
    if ((rc = call.begin()) != KC_OK) return rc;
    KcFlatten f{};
    f.intake = d_intake;
    f.mode = KC_INTAKE;
    f.g_first = g_first;
    f.count = count;
    if ((rc = flatten(c, call.s, f)) != KC_OK) return rc;
    if ((rc = refresh(c, call.s, count, kl, kt_seq, kt_loop, d_pool_ranges, d_pool_poses, pool_scans)) != KC_OK) return rc;
    return call.done();
}

int kc_refresh_jobs_device(kc_ctx *c, const ke_job *d_jobs, const ke_closure *d_closures, int count, kl_ctx *kl,
                           kt_ctx *kt_seq, kt_ctx *kt_loop, const double *d_pool_ranges, const double *d_pool_poses,
                           int pool_scans, void *hip_stream)
{
    int rc = check_call(c, count, d_jobs, d_pool_ranges, d_pool_poses, pool_scans);
    if (rc != KC_OK) return rc;
    if (count == 0) return KC_OK;
    StreamCall call(c->order, kc_err, hip_stream);
    if ((rc = call.begin()) != KC_OK) return rc;
    KcFlatten f{};
    f.jobs = d_jobs;
    f.closures = d_closures;
    f.mode = KC_JOBS;
    f.count = count;
    if ((rc = flatten(c, call.s, f)) != KC_OK) return rc;
    if ((rc = refresh(c, call.s, count, kl, kt_seq, kt_loop, d_pool_ranges, d_pool_poses, pool_scans)) != KC_OK) return rc;
    return call.done();
}

int kc_correct_poses_device(kc_ctx *c, const ke_job *d_jobs, const ke_closure *d_closures, int count, spa_ctx *spa,
                            const spa_params *params, kl_ctx *kl, kt_ctx *kt_seq, kt_ctx *kt_loop,
                            const double *d_pool_ranges, double *d_pool_poses, int pool_scans, void *hip_stream)
{
    int rc = check_call(c, count, d_jobs, d_pool_ranges, d_pool_poses, pool_scans);
    if (rc != KC_OK) return rc;
    if (!spa || !params) return kc_err.fail(KC_EINVAL, "spa or params is NULL");
    if (!d_closures && count > 0) return kc_err.fail(KC_EINVAL, "d_closures is NULL");
    if (!kl && (kt_seq || kt_loop)) return kc_err.fail(KC_EINVAL, "a matcher's refresh needs kl: it resolves the graphs' scan counts");
    if (count == 0) return KC_OK;
    StreamCall call(c->order, kc_err, hip_stream);
    if ((rc = call.begin()) != KC_OK) return rc;
    KcFlatten f{};
    f.jobs = d_jobs;
    f.closures = d_closures;
    f.mode = KC_CORRECT;
    f.count = count;
    if ((rc = flatten(c, call.s, f)) != KC_OK) return rc;
    if (spa_compute_rows_device(spa, count, c->d_graph, params, call.s) != SPA_OK)
        return refused(std::string("spa_compute_rows_device: ") + spa_last_error());
    if (spa_export_poses_device(spa, count, c->d_graph, c->d_pool_offset, d_pool_poses, pool_scans, call.s) != SPA_OK)
        return refused(std::string("spa_export_poses_device: ") + spa_last_error());
    if ((rc = refresh(c, call.s, count, kl, kt_seq, kt_loop, d_pool_ranges, d_pool_poses, pool_scans)) != KC_OK) return rc;
    return call.done();
}

int kc_get_info(kc_ctx *c, int *n_scans_refreshed, int *n_graphs_corrected, int *n_refused)
{
    if (!c) return kc_err.fail(KC_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(kc_err);
    if (rc != KC_OK) return rc;
    int info[3] = {0, 0, 0};
    S2D_CHK(kc_err, KC_EHIP, hipMemcpy(info, c->d_info, sizeof(info), hipMemcpyDeviceToHost));
    S2D_CHK(kc_err, KC_EHIP, hipMemset(c->d_info, 0, sizeof(info)));
    if (n_scans_refreshed) *n_scans_refreshed = info[0];
    if (n_graphs_corrected) *n_graphs_corrected = info[1];
    if (n_refused) *n_refused = info[2];
    return KC_OK;
}

int kc_set_timing(kc_ctx *c, int enable)
{
    if (!c) return kc_err.fail(KC_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return set_timing(c->timer, enable);
}

int kc_num_kernels(void) { return C_NUM; }
const char *kc_kernel_name(int i) { return kernel_name(c_names, C_NUM, i); }

int kc_get_kernel_times(kc_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return kc_err.fail(KC_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return get_kernel_times(c->timer, kc_err, ms_out, launches_out, reset, C_NUM);
}

}  // extern "C"
