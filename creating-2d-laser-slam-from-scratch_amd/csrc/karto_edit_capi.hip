// karto_edit_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_edit.h) of the Karto graph-edit
// stage: the scratch rows, the flatten / tally launches of karto_edit_kernels.hip and, between them, the graph
// contexts' own device-edit calls on the same stream.  Nothing here waits for the device but kd_get_info and
// kd_get_kernel_times.  Without a usable HIP device kd_create fails with KD_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include "host_timing.h"
#include "karto_edit_kernels.hip"

using namespace s2d;

namespace {
thread_local std::string kd_err;

int dfail(int code, const char *what, hipError_t e = hipSuccess)
{
    kd_err = what;
    if (e != hipSuccess) {
        kd_err += ": ";
        kd_err += hipGetErrorString(e);
    }
    return code;
}

#define DCHK(expr)                                              \
    do {                                                        \
        hipError_t _e = (expr);                                 \
        if (_e != hipSuccess) return dfail(KD_EHIP, #expr, _e); \
    } while (0)

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
    hipStream_t stream = nullptr, last = nullptr;
    hipEvent_t ev_last = nullptr;
    KernelTimer timer;
    std::mutex mu;
};

namespace {

#define KD_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, dfail, KD_EHIP, s, which, __VA_ARGS__)

unsigned blocks_for(int n) { return (unsigned)((n + KD_THREADS - 1) / KD_THREADS); }

int wait_last(kd_ctx *c)
{
    if (c->last) DCHK(hipStreamSynchronize(c->last));
    return KD_OK;
}

// the scratch rows may still be read by the previous call's work on another stream
int begin_on(kd_ctx *c, hipStream_t s)
{
    DCHK(hipStreamWaitEvent(s, c->ev_last, 0));
    return KD_OK;
}

int end_on(kd_ctx *c, hipStream_t s)
{
    DCHK(hipEventRecord(c->ev_last, s));
    c->last = s;
    return KD_OK;
}

int tally(kd_ctx *c, hipStream_t s, int rows, const int *val, int which, const int *status, int *mask_out)
{
    KD_LAUNCH(D_TALLY, kd_tally_kernel, dim3(blocks_for(rows)), dim3(KD_THREADS), 0, s, rows, val, which, status, mask_out,
              c->d_info);
    return KD_OK;
}

}  // namespace

extern "C" {

const char *kd_last_error(void) { return kd_err.c_str(); }
const char *kd_version(void) { return "slam2d-karto-edit 1 (gfx950)"; }

int kd_destroy(kd_ctx *c)
{
    if (!c) return KD_OK;
    if (c->last) hipStreamSynchronize(c->last);
    if (c->stream) hipStreamSynchronize(c->stream);
    void *bufs[] = {c->d_graph, c->d_expect, c->d_val, c->d_mask, c->d_status, c->d_status2, c->d_info, c->d_edges,
                    c->d_nodes, c->d_cons};
    for (void *b : bufs)
        if (b) hipFree(b);
    c->timer.destroy();
    if (c->ev_last) hipEventDestroy(c->ev_last);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return KD_OK;
}

int kd_create(kd_ctx **out, int max_rows)
{
    if (!out) return dfail(KD_EINVAL, "out is NULL");
    *out = nullptr;
    if (max_rows < 1 || max_rows > KD_MAX_ROWS) return dfail(KD_EINVAL, "need 1 <= max_rows <= 2^24");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return dfail(KD_ENODEV, "no HIP device");
    kd_ctx *c = new kd_ctx;
    c->R = max_rows;
    const size_t R = (size_t)max_rows;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming)) != hipSuccess) {
        kd_destroy(c);
        return dfail(KD_EHIP, "hipStreamCreate", e);
    }
    if ((e = hipMalloc((void **)&c->d_graph, sizeof(int) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_expect, sizeof(int) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_val, sizeof(int) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_mask, sizeof(int) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_status, sizeof(int) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_status2, sizeof(int) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_info, sizeof(int) * 3)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_edges, sizeof(kl_edge_row) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_nodes, sizeof(spa_node_row) * R)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_cons, sizeof(spa_con_row) * R)) != hipSuccess) {
        kd_destroy(c);
        return dfail(KD_ENOMEM, "hipMalloc", e);
    }
    if ((e = hipMemsetAsync(c->d_info, 0, sizeof(int) * 3, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess || (e = hipEventRecord(c->ev_last, c->stream)) != hipSuccess) {
        kd_destroy(c);
        return dfail(KD_EHIP, "initialising the context", e);
    }
    *out = c;
    return KD_OK;
}

int kd_commit_vertices_device(kd_ctx *c, const kp_intake *d_intake, int g_first, int count, kl_ctx *kl, spa_ctx *spa,
                              void *hip_stream)
{
    if (!c) return dfail(KD_EINVAL, "ctx is NULL");
    if (!kl) return dfail(KD_EINVAL, "kl is NULL");
    if (count < 0 || g_first < 0) return dfail(KD_EINVAL, "negative count or graph");
    if (count > c->R) return dfail(KD_ERANGE, "more records than the context's max_rows");
    if (count == 0) return KD_OK;
    if (!d_intake) return dfail(KD_EINVAL, "d_intake is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    int rc = begin_on(c, s);
    if (rc != KD_OK) return rc;
    KD_LAUNCH(D_FLATTEN_VERTICES, kd_flatten_vertices_kernel, dim3(blocks_for(count)), dim3(KD_THREADS), 0, s, d_intake,
              g_first, count, c->d_graph, c->d_expect, c->d_nodes);
    if (kl_edit_vertices_device(kl, count, c->d_graph, c->d_expect, c->d_val, c->d_status, s) != KL_OK) {
        end_on(c, s);
        kd_err = std::string("kl_edit_vertices_device: ") + kl_last_error();
        return KD_EINVAL;
    }
    if ((rc = tally(c, s, count, c->d_val, 0, c->d_status, c->d_mask)) != KD_OK) return rc;
    if (spa) {
        if (spa_edit_nodes_device(spa, count, c->d_nodes, c->d_mask, c->d_status2, s) != SPA_OK) {
            end_on(c, s);
            kd_err = std::string("spa_edit_nodes_device: ") + spa_last_error();
            return KD_EINVAL;
        }
        if ((rc = tally(c, s, count, nullptr, 0, c->d_status2, nullptr)) != KD_OK) return rc;
    }
    return end_on(c, s);
}

int kd_commit_edges_device(kd_ctx *c, const ke_job_out *d_jobs_out, const ke_link *d_links, int max_links, int first_job,
                           int count, kl_ctx *kl, spa_ctx *spa, void *hip_stream)
{
    if (!c) return dfail(KD_EINVAL, "ctx is NULL");
    if (!kl) return dfail(KD_EINVAL, "kl is NULL");
    if (count < 0 || first_job < 0 || max_links < 1) return dfail(KD_EINVAL, "negative count or job, or max_links < 1");
    if ((long long)count * max_links > c->R) return dfail(KD_ERANGE, "more link records than the context's max_rows");
    if (count == 0) return KD_OK;
    if (!d_jobs_out || !d_links) return dfail(KD_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int rows = count * max_links;
    int rc = begin_on(c, s);
    if (rc != KD_OK) return rc;
    KD_LAUNCH(D_FLATTEN_EDGES, kd_flatten_edges_kernel, dim3(blocks_for(rows)), dim3(KD_THREADS), 0, s, d_jobs_out, d_links,
              max_links, first_job, count, c->d_edges, c->d_cons);
    if (kl_edit_edges_device(kl, rows, c->d_edges, c->d_val, c->d_status, s) != KL_OK) {
        end_on(c, s);
        kd_err = std::string("kl_edit_edges_device: ") + kl_last_error();
        return KD_EINVAL;
    }
    if ((rc = tally(c, s, rows, c->d_val, 1, c->d_status, nullptr)) != KD_OK) return rc;
    if (spa) {
        if (spa_edit_constraints_device(spa, rows, c->d_cons, c->d_val, nullptr, c->d_status2, s) != SPA_OK) {
            end_on(c, s);
            kd_err = std::string("spa_edit_constraints_device: ") + spa_last_error();
            return KD_EINVAL;
        }
        if ((rc = tally(c, s, rows, nullptr, 0, c->d_status2, nullptr)) != KD_OK) return rc;
    }
    return end_on(c, s);
}

int kd_get_info(kd_ctx *c, int *n_vertices, int *n_new_edges, int *n_refused)
{
    if (!c) return dfail(KD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    int rc = wait_last(c);
    if (rc != KD_OK) return rc;
    int info[3] = {0, 0, 0};
    DCHK(hipMemcpy(info, c->d_info, sizeof(info), hipMemcpyDeviceToHost));
    DCHK(hipMemset(c->d_info, 0, sizeof(info)));
    if (n_vertices) *n_vertices = info[0];
    if (n_new_edges) *n_new_edges = info[1];
    if (n_refused) *n_refused = info[2];
    return KD_OK;
}

int kd_set_timing(kd_ctx *c, int enable)
{
    if (!c) return dfail(KD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    c->timer.on = enable != 0;
    return KD_OK;
}

int kd_num_kernels(void) { return D_NUM; }
const char *kd_kernel_name(int i) { return (i >= 0 && i < D_NUM) ? d_names[i] : ""; }

int kd_get_kernel_times(kd_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return dfail(KD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    DCHK(hipDeviceSynchronize());
    DCHK(c->timer.collect(ms_out, launches_out, reset, D_NUM));
    return KD_OK;
}

}  // extern "C"
