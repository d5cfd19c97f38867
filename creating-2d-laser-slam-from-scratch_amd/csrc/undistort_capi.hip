// undistort_capi.hip -- host runtime + extern "C" boundary (include/slam2d/undistort.h) of the lesson5
// lidar undistortion path.  Every compute step is ud_correct_kernel (undistort_kernels.hip); without a
// usable HIP device ud_create fails with UD_ENODEV.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/slam2d/undistort.h"
#include "stage_runtime.h"
#include "undistort_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError ud_err;
S2D_ASSERT_COMMON_CODES(UD);
}  // namespace

struct ud_ctx {
    int B = 0, n = 0, max_imu = 0;
    UdGeom g{};
    bool has_geometry = false;
    double2 *d_cs = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;
    DeviceBuffers mem;
    // single-scan staging (ud_correct)
    float *d_ranges1 = nullptr, *d_cloud1 = nullptr, *d_xy1 = nullptr, *d_origo1 = nullptr;
    double *d_time1 = nullptr, *d_imu1 = nullptr, *d_odom1 = nullptr;
    int *d_int1 = nullptr;  // imu_n, n, status
};

namespace {
void set_rules(ud_ctx *c, const hs_laser *L, float scale)
{
    UdGeom &g = c->g;
    memcpy(g.tf, L->basis, sizeof(double) * 9);
    memcpy(g.tf + 9, L->origin, sizeof(double) * 3);
    g.sqr_min = L->sqr_laser_min_dist;
    g.sqr_max = L->sqr_laser_max_dist;
    g.use_max_sq = L->use_max_scan_range * L->use_max_scan_range;  // double product, hector_slam.cc:344
    g.z_min = L->laser_z_min_value;
    g.z_max = L->laser_z_max_value;
    g.scale = scale;
    g.origo = make_float2((float)L->origin[0] * scale, (float)L->origin[1] * scale);  // hector_slam.cc:329
}

int launch(ud_ctx *c, int count, const float *d_ranges, int range_stride, const double *d_scan_time,
           const double *d_imu, int imu_stride, const int *d_imu_n, const double *d_odom, float *d_cloud,
           int cloud_stride, float *d_xy, int xy_stride, int *d_n, float *d_origo, int *d_status, hipStream_t s)
{
    const size_t lds = c->g.use_imu ? sizeof(double) * 4 * (size_t)c->max_imu : 0;
    hipLaunchKernelGGL(ud_correct_kernel, dim3(count), dim3(256), lds, s, c->g, c->d_cs, d_ranges, range_stride,
                       d_scan_time, d_imu, imu_stride, d_imu_n, d_odom, d_cloud, cloud_stride, (float2 *)d_xy,
                       xy_stride, d_n, (float2 *)d_origo, d_status);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? UD_OK : ud_err.fail(UD_EHIP, "ud_correct_kernel launch", e);
}

int check_batch(ud_ctx *c, int count, const float *d_ranges, int range_stride, const double *d_scan_time,
                const double *d_imu, int imu_stride, const int *d_imu_n, const double *d_odom, float *d_cloud,
                int cloud_stride, float *d_xy, int xy_stride, int *d_n)
{
    if (!c->has_geometry) return ud_err.fail(UD_EINVAL, "ud_set_scan_geometry not called");
    if (count < 0 || count > c->B) return ud_err.fail(UD_EINVAL, "count must be in [0, num_streams]");
    if (count == 0) return UD_OK;
    if (!d_ranges || !d_scan_time) return ud_err.fail(UD_EINVAL, "d_ranges / d_scan_time is NULL");
    if (range_stride < c->n) return ud_err.fail(UD_EINVAL, "range_stride < n_beams");
    if (c->g.use_imu && (!d_imu || !d_imu_n || imu_stride < 1)) return ud_err.fail(UD_EINVAL, "use_imu needs d_imu, d_imu_n, imu_stride >= 1");
    if (c->g.use_odom && !d_odom) return ud_err.fail(UD_EINVAL, "use_odom needs d_odom");
    if (d_cloud && cloud_stride < c->n) return ud_err.fail(UD_EINVAL, "cloud_stride < n_beams");
    if (d_xy && (!d_n || xy_stride < c->n)) return ud_err.fail(UD_EINVAL, "d_xy needs d_n and xy_stride >= n_beams");
    return UD_OK;
}
}  // namespace

extern "C" {

const char *ud_version(void) { return "slam2d-mi355x undistort 0.1 (gfx950)"; }
const char *ud_last_error(void) { return ud_err.c_str(); }

void ud_default_laser(hs_laser *L, int n_beams, float angle_min, float angle_increment)
{
    if (!L) return;
    hs_default_laser(L, n_beams, angle_min, angle_increment);
    // CorrectLaserScan's current_point_z = 1.0 (lidar_undistortion.cc:343) puts the corrected cloud at z = 1;
    // Hector's (-1, 1) window (hector_slam.cc:157-161, strict at :353) would drop all of it
    L->laser_z_min_value = 0.0f;
    L->laser_z_max_value = 2.0f;
}

int ud_create(ud_ctx **out, int num_streams, int n_beams, int max_imu)
{
    if (!out) return ud_err.fail(UD_EINVAL, "out is NULL");
    *out = nullptr;
    if (num_streams < 1 || n_beams < 1) return ud_err.fail(UD_EINVAL, "need num_streams >= 1, n_beams >= 1");
    if (max_imu < 1 || max_imu > UD_MAX_IMU) return ud_err.fail(UD_EINVAL, "max_imu must be in [1, 2000] (queueLength)");
    if (!device_present()) return ud_err.fail(UD_ENODEV, "no HIP device");
    ud_ctx *c = new ud_ctx;
    c->B = num_streams;
    c->n = n_beams;
    c->max_imu = max_imu;
    c->g.n = n_beams;
    c->g.max_imu = max_imu;
    c->g.use_imu = 1;   // lidar_undistortion.cc:27-28
    c->g.use_odom = 1;
    hs_laser L;
    ud_default_laser(&L, n_beams, 0.0f, 0.0f);
    set_rules(c, &L, 20.0f);
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault)) != hipSuccess) {
        delete c;
        return ud_err.fail(UD_EHIP, "hipStreamCreate", e);
    }
    const size_t n = (size_t)n_beams;
    c->mem.alloc(c->d_cs, sizeof(double2) * n);
    c->mem.alloc(c->d_ranges1, sizeof(float) * n);
    c->mem.alloc(c->d_cloud1, sizeof(float) * 3 * n);
    c->mem.alloc(c->d_xy1, sizeof(float) * 2 * n);
    c->mem.alloc(c->d_origo1, sizeof(float) * 2);
    c->mem.alloc(c->d_time1, sizeof(double) * 2);
    c->mem.alloc(c->d_imu1, sizeof(double) * 4 * (size_t)max_imu);
    c->mem.alloc(c->d_odom1, sizeof(double) * 14);
    c->mem.alloc(c->d_int1, sizeof(int) * 3);
    if ((e = c->mem.error) != hipSuccess) {
        ud_destroy(c);
        return ud_err.fail(UD_ENOMEM, "hipMalloc", e);
    }
    *out = c;
    return UD_OK;
}

int ud_destroy(ud_ctx *c)
{
    if (!c) return UD_OK;
    if (c->stream) hipStreamSynchronize(c->stream);
    c->mem.free_all();
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return UD_OK;
}

int ud_set_scan_geometry(ud_ctx *c, float angle_min, float angle_increment, float range_min, float range_max,
                         const double *unit_vectors)
{
    if (!c) return ud_err.fail(UD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    std::vector<double> cs((size_t)2 * c->n);
    for (int i = 0; i < c->n; ++i) {
        if (unit_vectors) {
            cs[2 * i] = unit_vectors[2 * i];
            cs[2 * i + 1] = unit_vectors[2 * i + 1];
        } else {  // CreateAngleCache :168-173: float32 fields, so the sum is a float before it widens
            const float a = angle_min + (float)(unsigned)i * angle_increment;
            const double angle = (double)a;
            cs[2 * i] = cos(angle);
            cs[2 * i + 1] = sin(angle);
        }
    }
    S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(c->d_cs, cs.data(), sizeof(double) * cs.size(), hipMemcpyHostToDevice, c->stream));
    S2D_CHK(ud_err, UD_EHIP, hipStreamSynchronize(c->stream));
    c->g.range_min = range_min;
    c->g.range_max = range_max;
    c->has_geometry = true;
    return UD_OK;
}

int ud_set_container_rules(ud_ctx *c, const hs_laser *L, float scale_to_map)
{
    if (!c || !L) return ud_err.fail(UD_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    set_rules(c, L, scale_to_map);
    return UD_OK;
}

int ud_set_sources(ud_ctx *c, int use_imu, int use_odom)
{
    if (!c) return ud_err.fail(UD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    c->g.use_imu = use_imu != 0;
    c->g.use_odom = use_odom != 0;
    return UD_OK;
}

int ud_correct_batch_device(ud_ctx *c, int count, const float *d_ranges, int range_stride, const double *d_scan_time,
                            const double *d_imu, int imu_stride, const int *d_imu_n, const double *d_odom,
                            float *d_cloud, int cloud_stride, float *d_xy, int xy_stride, int *d_n, float *d_origo,
                            int *d_status, void *hip_stream)
{
    if (!c) return ud_err.fail(UD_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    int rc = check_batch(c, count, d_ranges, range_stride, d_scan_time, d_imu, imu_stride, d_imu_n, d_odom, d_cloud,
                         cloud_stride, d_xy, xy_stride, d_n);
    if (rc != UD_OK || count == 0) return rc;
    // without a DataContainer output the count and origo are still reported when asked for
    return launch(c, count, d_ranges, range_stride, d_scan_time, d_imu, imu_stride, d_imu_n, d_odom, d_cloud,
                  cloud_stride, d_xy, xy_stride, d_n, d_origo, d_status, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int ud_correct(ud_ctx *c, const float *ranges, double scan_time_start, double scan_time_increment, const double *imu,
               int imu_n, const double *odom, float *cloud_out, float *xy_out, int *n_out, float *origo_out,
               int *status_out)
{
    if (!c || !ranges) return ud_err.fail(UD_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    if (!c->has_geometry) return ud_err.fail(UD_EINVAL, "ud_set_scan_geometry not called");
    if (c->g.use_imu) {
        if (imu_n < 0 || imu_n > c->max_imu) return ud_err.fail(UD_EINVAL, "imu_n must be in [0, max_imu]");
        if (imu_n > 0 && !imu) return ud_err.fail(UD_EINVAL, "imu is NULL");
        for (int i = 1; i < imu_n; ++i)
            if (!(imu[4 * i] >= imu[4 * (i - 1)])) return ud_err.fail(UD_EINVAL, "IMU times must be non-decreasing");
    } else {
        imu_n = 0;
    }
    if (c->g.use_odom && !odom) return ud_err.fail(UD_EINVAL, "odom is NULL");
    hipStream_t s = c->stream;
    const double tm[2] = {scan_time_start, scan_time_increment};
    const int n = c->n;
    S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(c->d_ranges1, ranges, sizeof(float) * n, hipMemcpyHostToDevice, s));
    S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(c->d_time1, tm, sizeof(tm), hipMemcpyHostToDevice, s));
    if (imu_n > 0) S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(c->d_imu1, imu, sizeof(double) * 4 * imu_n, hipMemcpyHostToDevice, s));
    S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(c->d_int1, &imu_n, sizeof(int), hipMemcpyHostToDevice, s));
    if (c->g.use_odom) S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(c->d_odom1, odom, sizeof(double) * 14, hipMemcpyHostToDevice, s));
    S2D_CHK(ud_err, UD_EHIP, hipStreamSynchronize(s));  // the sources are pageable host memory of the caller
    int rc = launch(c, 1, c->d_ranges1, n, c->d_time1, c->d_imu1, c->max_imu, c->d_int1, c->d_odom1, c->d_cloud1, n,
                    c->d_xy1, n, c->d_int1 + 1, c->d_origo1, c->d_int1 + 2, s);
    if (rc != UD_OK) return rc;
    int res[3] = {0, 0, 0};
    S2D_CHK(ud_err, UD_EHIP, hipMemcpyAsync(res, c->d_int1, sizeof(res), hipMemcpyDeviceToHost, s));
    S2D_CHK(ud_err, UD_EHIP, hipStreamSynchronize(s));
    if (cloud_out) S2D_CHK(ud_err, UD_EHIP, hipMemcpy(cloud_out, c->d_cloud1, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    if (xy_out && res[1] > 0) S2D_CHK(ud_err, UD_EHIP, hipMemcpy(xy_out, c->d_xy1, sizeof(float) * 2 * res[1], hipMemcpyDeviceToHost));
    if (origo_out) S2D_CHK(ud_err, UD_EHIP, hipMemcpy(origo_out, c->d_origo1, sizeof(float) * 2, hipMemcpyDeviceToHost));
    if (n_out) *n_out = res[1];
    if (status_out) *status_out = res[2];
    return UD_OK;
}

int ud_rpy_from_quaternion(const double q[4], double rpy[3])
{
    if (!q || !rpy) return ud_err.fail(UD_EINVAL, "NULL argument");
    // tf::Matrix3x3::setRotation(q)
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double d = x * x + y * y + z * z + w * w;
    if (!(d != 0.0)) return ud_err.fail(UD_EINVAL, "zero quaternion");
    const double s = 2.0 / d;
    const double xs = x * s, ys = y * s, zs = z * s;
    const double wx = w * xs, wy = w * ys, wz = w * zs;
    const double xx = x * xs, xy = x * ys, xz = x * zs;
    const double yy = y * ys, yz = y * zs, zz = z * zs;
    const double m00 = 1.0 - (yy + zz), m01 = xy - wz, m02 = xz + wy;
    const double m10 = xy + wz;
    const double m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
    // tf::Matrix3x3::getRPY -> getEulerYPR, solution 1
    double roll, pitch, yaw;
    if (fabs(m20) >= 1.0) {  // pitch at a singularity: yaw = 0, roll from the difference-of-angles formula
        yaw = 0.0;
        if (m20 < 0.0) {
            pitch = M_PI / 2.0;
            roll = atan2(m01, m02);
        } else {
            pitch = -M_PI / 2.0;
            roll = atan2(-m01, -m02);
        }
    } else {
        pitch = -asin(m20);
        roll = atan2(m21 / cos(pitch), m22 / cos(pitch));
        yaw = atan2(m10 / cos(pitch), m00 / cos(pitch));
    }
    rpy[0] = roll;
    rpy[1] = pitch;
    rpy[2] = yaw;
    return UD_OK;
}

void *ud_get_stream(ud_ctx *c) { return c ? (void *)c->stream : nullptr; }

}  // extern "C"
