// plicp_capi.hip -- host runtime + extern "C" boundary (include/slam2d/plicp.h) of the PL-ICP path.
// Every compute step is pl_icp_kernel (plicp_kernels.hip); without a usable HIP device pl_create fails
// with PL_ENODEV.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>
#include <vector>

#include "stage_runtime.h"
#include "plicp_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError pl_err;
S2D_ASSERT_COMMON_CODES(PL);

size_t pl_shmem(int n) { return (size_t)n * (sizeof(double2) + sizeof(unsigned long long) + 2 * sizeof(int16_t)); }
}  // namespace

struct pl_ctx {
    int max_pairs = 0, max_rays = 0;
    pl_params params{};
    double *d_ref = nullptr, *d_sens = nullptr, *d_guess = nullptr, *d_theta = nullptr;
    pl_result *d_res = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffers mem;
    KernelTimer timer;  // one index: pl_icp_kernel
};

extern "C" {

const char *pl_version(void) { return "slam2d-mi355x plicp 0.1 (gfx950)"; }
const char *pl_last_error(void) { return pl_err.c_str(); }

void pl_default_params(pl_params *p)
{
    if (!p) return;
    // ScanMatchPLICP::InitParams (lesson3/src/plicp_odometry.cc:74-186)
    p->max_angular_correction_deg = 45.0;
    p->max_linear_correction = 1.0;
    p->max_iterations = 10;
    p->epsilon_xy = 0.000001;
    p->epsilon_theta = 0.000001;
    p->max_correspondence_dist = 1.0;
    p->use_point_to_line_distance = 1;
    p->outliers_maxPerc = 0.90;
    p->outliers_adaptive_order = 0.7;
    p->outliers_adaptive_mult = 2.0;
    p->outliers_remove_doubles = 1;
    p->pad_ = 0;
}

int pl_create(pl_ctx **out, int max_pairs, int max_rays, const pl_params *params)
{
    if (!out) return pl_err.fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    if (max_pairs < 1 || max_rays < 2 || max_rays > PL_MAX_RAYS) return pl_err.fail(PL_EINVAL, "need 1 <= pairs, 2 <= rays <= 2048");
    if (params && (params->max_iterations < 1 || params->max_iterations > PL_MAX_IT))
        return pl_err.fail(PL_EINVAL, "max_iterations must be in [1, 64]");
    if (!device_present()) return pl_err.fail(PL_ENODEV, "no HIP device");
    pl_ctx *c = new pl_ctx;
    c->max_pairs = max_pairs;
    c->max_rays = max_rays;
    if (params) c->params = *params;
    else pl_default_params(&c->params);
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault)) != hipSuccess) {
        delete c;
        return pl_err.fail(PL_EHIP, "hipStreamCreate", e);
    }
    c->mem.alloc(c->d_ref, sizeof(double) * max_rays);
    c->mem.alloc(c->d_sens, sizeof(double) * max_rays);
    c->mem.alloc(c->d_guess, sizeof(double) * 3);
    c->mem.alloc(c->d_theta, sizeof(double) * max_rays);
    c->mem.alloc(c->d_res, sizeof(pl_result));
    if ((e = c->mem.error) != hipSuccess) {
        pl_destroy(c);
        return pl_err.fail(PL_ENOMEM, "hipMalloc", e);
    }
    *out = c;
    return PL_OK;
}

int pl_destroy(pl_ctx *c)
{
    if (!c) return PL_OK;
    if (c->stream) hipStreamSynchronize(c->stream);
    c->mem.free_all();
    c->timer.destroy();
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return PL_OK;
}

static int pl_launch(pl_ctx *c, int count, int n, double angle_min, double angle_inc, const double *d_ref,
                     const double *d_sens, const double *d_guess, pl_result *d_res, hipStream_t s,
                     const double *d_theta = nullptr)
{
    if (count < 0 || count > c->max_pairs) return pl_err.fail(PL_EINVAL, "count exceeds max_pairs");
    if (n < 2 || n > c->max_rays) return pl_err.fail(PL_EINVAL, "n out of range");
    if (!(angle_inc > 0.0)) return pl_err.fail(PL_EINVAL, "angle_increment must be > 0");
    if (count == 0) return PL_OK;
    const int rpt = (n + PL_THREADS - 1) / PL_THREADS;
    auto kern = rpt <= 2 ? pl_icp_kernel<2> : rpt <= 4 ? pl_icp_kernel<4> : rpt <= 5 ? pl_icp_kernel<5>
              : rpt <= 6 ? pl_icp_kernel<6> : pl_icp_kernel<PL_RPT_MAX>;
    S2D_TIMED_LAUNCH(c->timer, pl_err.fail, PL_EHIP, s, 0, kern, dim3(count), dim3(PL_THREADS), pl_shmem(n), s, c->params, n,
                     angle_min, angle_inc, d_theta, d_ref, d_sens, d_guess, d_res);
    return PL_OK;
}

int pl_icp(pl_ctx *c, int n, double angle_min, double angle_inc, const double *ref, const double *sens,
           const double first_guess[3], pl_result *result)
{
    if (!c || !ref || !sens || !result) return pl_err.fail(PL_EINVAL, "NULL argument");
    if (n < 2 || n > c->max_rays) return pl_err.fail(PL_EINVAL, "n out of range");
    const double zero[3] = {0.0, 0.0, 0.0};
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_ref, ref, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_sens, sens, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_guess, first_guess ? first_guess : zero, sizeof(double) * 3, hipMemcpyHostToDevice, c->stream));
    int rc = pl_launch(c, 1, n, angle_min, angle_inc, c->d_ref, c->d_sens, c->d_guess, c->d_res, c->stream);
    if (rc != PL_OK) return rc;
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(result, c->d_res, sizeof(pl_result), hipMemcpyDeviceToHost, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipStreamSynchronize(c->stream));
    return PL_OK;
}

int pl_set_params(pl_ctx *c, const pl_params *params)
{
    if (!c || !params) return pl_err.fail(PL_EINVAL, "NULL argument");
    if (params->max_iterations < 1 || params->max_iterations > PL_MAX_IT)
        return pl_err.fail(PL_EINVAL, "max_iterations must be in [1, 64]");
    c->params = *params;
    return PL_OK;
}

int pl_icp_ldp(pl_ctx *c, int n, const double *theta, const double *ref_readings, const int *ref_valid,
               const double *sens_readings, const int *sens_valid, const double first_guess[3], pl_result *result)
{
    if (!c || !theta || !ref_readings || !sens_readings || !result) return pl_err.fail(PL_EINVAL, "NULL argument");
    if (n < 2 || n > c->max_rays) return pl_err.fail(PL_EINVAL, "n out of range");
    // the correspondence search maps polar angles to rays with the mean increment; an LDP of a
    // LaserScan (angle_min + i * angle_increment, plicp_odometry.cc:306) is uniform to rounding
    const double inc = (theta[n - 1] - theta[0]) / (double)(n - 1);
    if (!(inc > 0.0)) return pl_err.fail(PL_EINVAL, "theta must increase");
    for (int i = 0; i < n; ++i)
        if (fabs(theta[i] - (theta[0] + i * inc)) > 1e-3 * inc)
            return pl_err.fail(PL_EINVAL, "theta[] is not a uniform LaserScan grid");
    // readings of invalid rays -> -1 (LaserScanToLDP, :297-301): valid[] decides, as ld_valid_ray does
    std::vector<double> rr(ref_readings, ref_readings + n), sr(sens_readings, sens_readings + n);
    for (int i = 0; i < n; ++i) {
        if (ref_valid && !ref_valid[i]) rr[i] = -1.0;
        if (sens_valid && !sens_valid[i]) sr[i] = -1.0;
        if (!(rr[i] > 0.0)) rr[i] = -1.0;
        if (!(sr[i] > 0.0)) sr[i] = -1.0;
    }
    const double zero[3] = {0.0, 0.0, 0.0};
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_ref, rr.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_sens, sr.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_theta, theta, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(c->d_guess, first_guess ? first_guess : zero, sizeof(double) * 3, hipMemcpyHostToDevice, c->stream));
    int rc = pl_launch(c, 1, n, theta[0], inc, c->d_ref, c->d_sens, c->d_guess, c->d_res, c->stream, c->d_theta);
    if (rc != PL_OK) return rc;
    S2D_CHK(pl_err, PL_EHIP, hipMemcpyAsync(result, c->d_res, sizeof(pl_result), hipMemcpyDeviceToHost, c->stream));
    S2D_CHK(pl_err, PL_EHIP, hipStreamSynchronize(c->stream));
    return PL_OK;
}

int pl_icp_batch_device(pl_ctx *c, int count, int n, double angle_min, double angle_inc, const double *d_ref,
                        const double *d_sens, const double *d_guess, pl_result *d_res, void *hip_stream)
{
    if (!c || !d_ref || !d_sens || !d_res) return pl_err.fail(PL_EINVAL, "NULL argument");
    return pl_launch(c, count, n, angle_min, angle_inc, d_ref, d_sens, d_guess, d_res,
                     hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int pl_set_timing(pl_ctx *c, int enable)
{
    if (!c) return pl_err.fail(PL_EINVAL, "ctx is NULL");
    return set_timing(c->timer, enable);
}

int pl_get_kernel_times(pl_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return pl_err.fail(PL_EINVAL, "ctx is NULL");
    return get_kernel_times(c->timer, pl_err, ms_out, launches_out, reset, 1);
}

}  // extern "C"
