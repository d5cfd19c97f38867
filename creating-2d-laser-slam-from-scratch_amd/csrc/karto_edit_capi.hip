// karto_edit_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_edit.h) of the Karto graph-edit
// stage: the scratch rows, the flatten / tally launches of karto_edit_kernels.hip and, between them, the graph
// contexts' own device-edit calls on the same stream.  Nothing here waits for the device but kd_get_info and
// kd_get_kernel_times.  Without a usable HIP device kd_create fails with KD_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include "stage_runtime.h"
#include "karto_edit_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError kd_err;
S2D_ASSERT_STATUS_CODES(KD);

constexpr int KD_MAX_ROWS = 1 << 24;

enum { D_FLATTEN_VERTICES, D_FLATTEN_EDGES, D_TALLY, D_NUM };
const char *const d_names[D_NUM] = {"kd_flatten_vertices_kernel", "kd_flatten_edges_kernel", "kd_tally_kernel"};
static_assert(D_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
}  // namespace

struct kd_ctx {
    int R = 0;
    int *d_graph = nullptr, *d_expect = nullptr, *d_val = nullptr, *d_mask = nullptr, *d_status = nullptr, *d_status2 = nullptr;
    int *d_info = nullptr;  // vertices, new edges, refused rows
    kl_edge_row *d_edges = nullptr;
    spa_node_row *d_nodes = nullptr;
    spa_con_row *d_cons = nullptr;
    StreamOrder order;  // the scratch rows may still be read by the previous call's work on another stream
    DeviceBuffers mem;
    KernelTimer timer;
};

namespace {

#define KD_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, kd_err.fail, KD_EHIP, s, which, __VA_ARGS__)

unsigned blocks_for(int n) { return (unsigned)((n + KD_THREADS - 1) / KD_THREADS); }

int tally(kd_ctx *c, hipStream_t s, int rows, const int *val, int which, const int *status, int *mask_out)
{
    KD_LAUNCH(D_TALLY, kd_tally_kernel, dim3(blocks_for(rows)), dim3(KD_THREADS), 0, s, rows, val, which, status, mask_out,
              c->d_info);
    return KD_OK;
}

// a graph context refused the call: its text behind the call's name
int refused(const std::string &why) { return kd_err.fail(KD_EINVAL, why.c_str()); }

}  // namespace

extern "C" {

const char *kd_last_error(void) { return kd_err.c_str(); }
const char *kd_version(void) { return "slam2d-karto-edit 1 (gfx950)"; }

int kd_destroy(kd_ctx *c)
{
    if (!c) return KD_OK;
    c->order.destroy();
    c->mem.free_all();
    c->timer.destroy();
    delete c;
    return KD_OK;
}

int kd_create(kd_ctx **out, int max_rows)
{
    if (!out) return kd_err.fail(KD_EINVAL, "out is NULL");
    *out = nullptr;
    if (max_rows < 1 || max_rows > KD_MAX_ROWS) return kd_err.fail(KD_EINVAL, "need 1 <= max_rows <= 2^24");
    if (!device_present()) return kd_err.fail(KD_ENODEV, "no HIP device");
    kd_ctx *c = new kd_ctx;
    c->R = max_rows;
    const size_t R = (size_t)max_rows;
    hipError_t e;
    if ((e = c->order.create()) != hipSuccess) {
        kd_destroy(c);
        return kd_err.fail(KD_EHIP, "hipStreamCreate", e);
    }
    for (int **rows : {&c->d_graph, &c->d_expect, &c->d_val, &c->d_mask, &c->d_status, &c->d_status2})
        c->mem.alloc(*rows, sizeof(int) * R);
    c->mem.alloc(c->d_info, sizeof(int) * 3);
    c->mem.alloc(c->d_edges, sizeof(kl_edge_row) * R);
    c->mem.alloc(c->d_nodes, sizeof(spa_node_row) * R);
    c->mem.alloc(c->d_cons, sizeof(spa_con_row) * R);
    if ((e = c->mem.error) != hipSuccess) {
        kd_destroy(c);
        return kd_err.fail(KD_ENOMEM, "hipMalloc", e);
    }
    hipStream_t s = c->order.stream;
    if ((e = hipMemsetAsync(c->d_info, 0, sizeof(int) * 3, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess || (e = hipEventRecord(c->order.ev_last, s)) != hipSuccess) {
        kd_destroy(c);
        return kd_err.fail(KD_EHIP, "initialising the context", e);
    }
    *out = c;
    return KD_OK;
}

int kd_commit_vertices_device(kd_ctx *c, const kp_intake *d_intake, int g_first, int count, kl_ctx *kl, spa_ctx *spa,
                              void *hip_stream)
{
    if (!c) return kd_err.fail(KD_EINVAL, "ctx is NULL");
    if (!kl) return kd_err.fail(KD_EINVAL, "kl is NULL");
    if (count < 0 || g_first < 0) return kd_err.fail(KD_EINVAL, "negative count or graph");
    if (count > c->R) return kd_err.fail(KD_ERANGE, "more records than the context's max_rows");
    if (count == 0) return KD_OK;
    if (!d_intake) return kd_err.fail(KD_EINVAL, "d_intake is NULL");
    StreamCall call(c->order, kd_err, hip_stream);
    const hipStream_t s = call.s;
    int rc = call.begin();
    if (rc != KD_OK) return rc;
    KD_LAUNCH(D_FLATTEN_VERTICES, kd_flatten_vertices_kernel, dim3(blocks_for(count)), dim3(KD_THREADS), 0, s, d_intake,
              g_first, count, c->d_graph, c->d_expect, c->d_nodes);
    if (kl_edit_vertices_device(kl, count, c->d_graph, c->d_expect, c->d_val, c->d_status, s) != KL_OK)
        return refused(std::string("kl_edit_vertices_device: ") + kl_last_error());
    if ((rc = tally(c, s, count, c->d_val, 0, c->d_status, c->d_mask)) != KD_OK) return rc;
    if (spa) {
        if (spa_edit_nodes_device(spa, count, c->d_nodes, c->d_mask, c->d_status2, s) != SPA_OK)
            return refused(std::string("spa_edit_nodes_device: ") + spa_last_error());
        if ((rc = tally(c, s, count, nullptr, 0, c->d_status2, nullptr)) != KD_OK) return rc;
    }
    return call.done();
}

int kd_commit_edges_device(kd_ctx *c, const ke_job_out *d_jobs_out, const ke_link *d_links, int max_links, int first_job,
                           int count, kl_ctx *kl, spa_ctx *spa, void *hip_stream)
{
    if (!c) return kd_err.fail(KD_EINVAL, "ctx is NULL");
    if (!kl) return kd_err.fail(KD_EINVAL, "kl is NULL");
    if (count < 0 || first_job < 0 || max_links < 1) return kd_err.fail(KD_EINVAL, "negative count or job, or max_links < 1");
    if ((long long)count * max_links > c->R) return kd_err.fail(KD_ERANGE, "more link records than the context's max_rows");
    if (count == 0) return KD_OK;
    if (!d_jobs_out || !d_links) return kd_err.fail(KD_EINVAL, "NULL argument");
    StreamCall call(c->order, kd_err, hip_stream);
    const hipStream_t s = call.s;
    const int rows = count * max_links;
    int rc = call.begin();
    if (rc != KD_OK) return rc;
    KD_LAUNCH(D_FLATTEN_EDGES, kd_flatten_edges_kernel, dim3(blocks_for(rows)), dim3(KD_THREADS), 0, s, d_jobs_out, d_links,
              max_links, first_job, count, c->d_edges, c->d_cons);
    if (kl_edit_edges_device(kl, rows, c->d_edges, c->d_val, c->d_status, s) != KL_OK)
        return refused(std::string("kl_edit_edges_device: ") + kl_last_error());
    if ((rc = tally(c, s, rows, c->d_val, 1, c->d_status, nullptr)) != KD_OK) return rc;
    if (spa) {
        if (spa_edit_constraints_device(spa, rows, c->d_cons, c->d_val, nullptr, c->d_status2, s) != SPA_OK)
            return refused(std::string("spa_edit_constraints_device: ") + spa_last_error());
        if ((rc = tally(c, s, rows, nullptr, 0, c->d_status2, nullptr)) != KD_OK) return rc;
    }
    return call.done();
}

int kd_get_info(kd_ctx *c, int *n_vertices, int *n_new_edges, int *n_refused)
{
    if (!c) return kd_err.fail(KD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(kd_err);
    if (rc != KD_OK) return rc;
    int info[3] = {0, 0, 0};
    S2D_CHK(kd_err, KD_EHIP, hipMemcpy(info, c->d_info, sizeof(info), hipMemcpyDeviceToHost));
    S2D_CHK(kd_err, KD_EHIP, hipMemset(c->d_info, 0, sizeof(info)));
    if (n_vertices) *n_vertices = info[0];
    if (n_new_edges) *n_new_edges = info[1];
    if (n_refused) *n_refused = info[2];
    return KD_OK;
}

int kd_set_timing(kd_ctx *c, int enable)
{
    if (!c) return kd_err.fail(KD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return set_timing(c->timer, enable);
}

int kd_num_kernels(void) { return D_NUM; }
const char *kd_kernel_name(int i) { return kernel_name(d_names, D_NUM, i); }

int kd_get_kernel_times(kd_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return kd_err.fail(KD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    return get_kernel_times(c->timer, kd_err, ms_out, launches_out, reset, D_NUM);
}

}  // extern "C"
