// undistort_kernels.hip -- the lesson5 lidar motion undistortion on the device (gfx950).
//
// LidarUndistortion::ScanCallback (lesson5/src/lidar_undistortion.cc:96-124) for a batch of scans, one
// 256-thread workgroup per scan, in the node's order: PruneImuDeque's integration loop (:202-246) and
// PruneOdomDeque's increment (:304-334) by one lane (serial chains: a parallel prefix sum would change the
// bits), then CorrectLaserScan (:339-395) beam by beam with ComputeRotation (:398-432) and ComputePosition
// (:435-447) reading the integrated window from LDS.  The corrected cloud is written as the node publishes it
// and, a second time, as Hector DataContainer points (rosPointCloudToDataContainer, lesson4/src/
// hector_mapping/hector_slam.cc:320-362) compacted in beam order.
//
// PCL / Eigen are not available to this build, so the float pieces are fixed here (DESIGN.md section 3,
// parity unpinned): pcl::getTransformation (PCL common/impl/eigen.hpp), Affine3f::inverse (3x3 cofactor
// inverse, translation -(L^-1 t)), the Affine3f product (L1 L2, L1 t2 + t1); every dot product left to right;
// float sin / cos = sdm_sinf / sdm_cosf (detmath.h).  Built with -ffp-contract=off: no expression below fuses.
#pragma once
#include <hip/hip_runtime.h>

#include <limits.h>

#include "detmath.h"

namespace s2d {

struct UdGeom {
    double tf[12];       // DataContainer rules: laserTransform basis rows, origin (hector_slam.cc:325, :348)
    double use_max_sq;   // p_use_max_scan_range_^2 (:344)
    float range_min, range_max;  // LaserScan range_min / range_max (lidar_undistortion.cc:351-352)
    float sqr_min, sqr_max, z_min, z_max, scale;
    float2 origo;        // laserPos.xy * scaleToMap (hector_slam.cc:329)
    int n;               // ranges per scan (scan_count_)
    int max_imu;         // LDS window capacity, samples
    int use_imu, use_odom;
};

struct UdAffine {  // Eigen::Affine3f, rows of [L | t]
    float m[12];
};

// pcl::getTransformation(x, y, z, roll, pitch, yaw)  (PCL common/impl/eigen.hpp, float instance)
__device__ __forceinline__ UdAffine ud_get_transformation(float x, float y, float z, float roll, float pitch, float yaw)
{
    const float A = sdm_cosf(yaw), B = sdm_sinf(yaw), C = sdm_cosf(pitch), D = sdm_sinf(pitch);
    const float E = sdm_cosf(roll), F = sdm_sinf(roll), DE = D * E, DF = D * F;
    UdAffine t;
    t.m[0] = A * C;  t.m[1] = A * DF - B * E;  t.m[2] = B * F + A * DE;   t.m[3] = x;
    t.m[4] = B * C;  t.m[5] = A * E + B * DF;  t.m[6] = B * DE - A * F;   t.m[7] = y;
    t.m[8] = -D;     t.m[9] = C * F;           t.m[10] = C * E;           t.m[11] = z;
    return t;
}

// Affine3f::inverse(): cofactor inverse of the linear part times 1/det, translation -(L^-1 t)
__device__ __forceinline__ UdAffine ud_inverse(const UdAffine &a)
{
#define UD_M(i, j) a.m[(i)*4 + (j)]
#define UD_COF(i, j) (UD_M(((i) + 1) % 3, ((j) + 1) % 3) * UD_M(((i) + 2) % 3, ((j) + 2) % 3) - \
                      UD_M(((i) + 1) % 3, ((j) + 2) % 3) * UD_M(((i) + 2) % 3, ((j) + 1) % 3))
    const float c00 = UD_COF(0, 0), c10 = UD_COF(1, 0), c20 = UD_COF(2, 0);
    const float det = c00 * UD_M(0, 0) + c10 * UD_M(1, 0) + c20 * UD_M(2, 0);
    const float invdet = __fdiv_rn(1.0f, det);
    UdAffine r;
    r.m[0] = c00 * invdet;           r.m[1] = c10 * invdet;           r.m[2] = c20 * invdet;
    r.m[4] = UD_COF(0, 1) * invdet;  r.m[5] = UD_COF(1, 1) * invdet;  r.m[6] = UD_COF(2, 1) * invdet;
    r.m[8] = UD_COF(0, 2) * invdet;  r.m[9] = UD_COF(1, 2) * invdet;  r.m[10] = UD_COF(2, 2) * invdet;
#undef UD_COF
#undef UD_M
    for (int i = 0; i < 3; ++i)
        r.m[i * 4 + 3] = -(r.m[i * 4] * a.m[3] + r.m[i * 4 + 1] * a.m[7] + r.m[i * 4 + 2] * a.m[11]);
    return r;
}

// Affine3f * Affine3f: L = L1 L2, t = L1 t2 + t1
__device__ __forceinline__ UdAffine ud_mul(const UdAffine &a, const UdAffine &b)
{
    UdAffine r;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            r.m[i * 4 + j] = a.m[i * 4] * b.m[j] + a.m[i * 4 + 1] * b.m[4 + j] + a.m[i * 4 + 2] * b.m[8 + j];
        r.m[i * 4 + 3] = a.m[i * 4] * b.m[3] + a.m[i * 4 + 1] * b.m[7] + a.m[i * 4 + 2] * b.m[11] + a.m[i * 4 + 3];
    }
    return r;
}

// the per-scan motion model the beams read (LDS): the integrated IMU window [k] = (imu_time_, imu_rot_x_,
// imu_rot_y_, imu_rot_z_)[k] for k <= cur, and the odometry increment with its two times
struct UdMotion {
    const double *win;
    int cur;             // current_imu_index_ after :246
    float inc[3];        // odom_incre_x_, _y_, _z_
    double t0, t1;       // start_odom_time_, end_odom_time_
};

// ComputeRotation (:398-432).  The reference walks imuPointerFront up from 0 while
// pointTime >= imu_time_[imuPointerFront]; for the non-decreasing times of a window the bisection below
// returns that same index: the first idx < cur with pointTime < t[idx], else cur.
__device__ __forceinline__ void ud_compute_rotation(const UdMotion &mo, double pointTime, float rot[3])
{
    int lo = 0, hi = mo.cur;                                                   // :405-411
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pointTime < mo.win[4 * mid]) hi = mid;
        else lo = mid + 1;
    }
    const int front = lo;
    const double tf = mo.win[4 * front];
    if (pointTime > tf || front == 0) {                                        // :414-419
        rot[0] = (float)mo.win[4 * front + 1];
        rot[1] = (float)mo.win[4 * front + 2];
        rot[2] = (float)mo.win[4 * front + 3];
    } else {
        const int back = front - 1;                                            // :422
        const double tb = mo.win[4 * back];
        const double ratioFront = (pointTime - tb) / (tf - tb);                // :425
        const double ratioBack = (tf - pointTime) / (tf - tb);                 // :426
        rot[0] = (float)(mo.win[4 * front + 1] * ratioFront + mo.win[4 * back + 1] * ratioBack);  // :428-430
        rot[1] = (float)(mo.win[4 * front + 2] * ratioFront + mo.win[4 * back + 2] * ratioBack);
        rot[2] = (float)(mo.win[4 * front + 3] * ratioFront + mo.win[4 * back + 3] * ratioBack);
    }
}

// ComputePosition (:435-447): float * double, rounded to float
__device__ __forceinline__ void ud_compute_position(const UdMotion &mo, double pointTime, float pos[3])
{
    const double ratioFront = (pointTime - mo.t0) / (mo.t1 - mo.t0);           // :442
    pos[0] = (float)((double)mo.inc[0] * ratioFront);                          // :444-446
    pos[1] = (float)((double)mo.inc[1] * ratioFront);
    pos[2] = (float)((double)mo.inc[2] * ratioFront);
}

// pcl::getTransformation(pos, rot) at a point time (:364-371, :383-384)
__device__ __forceinline__ UdAffine ud_pose_at(const UdGeom &g, const UdMotion &mo, double pointTime)
{
    float rot[3] = {0.0f, 0.0f, 0.0f}, pos[3] = {0.0f, 0.0f, 0.0f};            // :364-365
    if (g.use_imu) ud_compute_rotation(mo, pointTime, rot);                    // :368-369
    if (g.use_odom) ud_compute_position(mo, pointTime, pos);                   // :370-371
    return ud_get_transformation(pos[0], pos[1], pos[2], rot[0], rot[1], rot[2]);
}

// the validity test of CorrectLaserScan (:350-353)
__device__ __forceinline__ bool ud_beam_valid(const UdGeom &g, float r)
{
    return !(!isfinite(r) || r < g.range_min || r > g.range_max);
}

// rosPointCloudToDataContainer's loop body (hector_slam.cc:333-357) for one cloud point
__device__ __forceinline__ bool ud_container_point(const UdGeom &g, float x, float y, float z, float2 &p)
{
    const float d2 = x * x + y * y;                                            // :335
    bool keep = (d2 > g.sqr_min) && (d2 < g.sqr_max);                          // :336
    if ((x < 0.0f) && (d2 < 0.50f)) keep = false;                              // :338-341
    if ((double)d2 > g.use_max_sq) keep = false;                               // :344-345
    if (keep) {
        const double vx = (double)x, vy = (double)y, vz = (double)z;           // :348 tf dot products
        const double px = g.tf[0] * vx + g.tf[1] * vy + g.tf[2] * vz + g.tf[9];
        const double py = g.tf[3] * vx + g.tf[4] * vy + g.tf[5] * vz + g.tf[10];
        const double pz = g.tf[6] * vx + g.tf[7] * vy + g.tf[8] * vz + g.tf[11];
        const float zl = (float)(pz - g.tf[11]);                               // :351
        keep = zl > g.z_min && zl < g.z_max;                                   // :353
        p = make_float2((float)px * g.scale, (float)py * g.scale);             // :356
    }
    return keep;
}

// status: 0 corrected, 1 waiting for IMU, 2 waiting for odom (include/slam2d/undistort.h)
__global__ void __launch_bounds__(256)
ud_correct_kernel(UdGeom g, const double2 *__restrict__ cs, const float *__restrict__ ranges, int rstride,
                  const double *__restrict__ scan_time, const double *__restrict__ imu, int imu_stride,
                  const int *__restrict__ imu_n, const double *__restrict__ odom, float *__restrict__ cloud,
                  int cstride, float2 *__restrict__ xy, int xy_stride, int *__restrict__ n_out,
                  float2 *__restrict__ origo_out, int *__restrict__ status_out)
{
    extern __shared__ double s_win[];  // [max_imu][4]: (t, wx, wy, wz) staged, then (t, rot x, y, z) in place
    __shared__ double s_ot[2];
    __shared__ float s_inc[3];
    __shared__ float s_tsi[12];
    __shared__ int s_cur;
    __shared__ int s_first[4];
    __shared__ int s_w[4];

    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *r = ranges + (size_t)s * rstride;
    float *cl = cloud ? cloud + (size_t)s * cstride * 3 : nullptr;
    // CacheLaserScan :154-156 (scan_count_ is a double in the node)
    const double t_start = scan_time[2 * s], t_inc = scan_time[2 * s + 1];
    const double t_end = t_start + t_inc * ((double)g.n - 1);

    // ---- the early returns of ScanCallback (uniform over the workgroup) ----
    int status = 0, ni = 0;
    const double *w = nullptr;
    if (g.use_imu) {                                                           // :103-107
        ni = imu_n[s];
        w = imu + (size_t)s * imu_stride * 4;
        if (ni <= 0 || ni > g.max_imu || ni > imu_stride) {                    // :182 empty (or not a window)
            status = 1;
        } else {
            const double tf = w[0], tb = w[4 * (size_t)(ni - 1)];
            if (tf > t_start || tb < t_end) status = 1;                        // :183-184
            if (!(tf < t_start)) status = 1;  // :212-222 would leave index 0 unset, :237 then reads imu_time_[-1]
        }
    }
    if (status == 0 && g.use_odom) {                                           // :110-114, :257-263, :274-275
        const double *o = odom + (size_t)s * 14;
        if (o[0] != o[0] || o[7] != o[7]) status = 2;
    }
    if (status != 0) {  // the node returns before CorrectLaserScan: nothing is published
        if (cl)
            for (int i = tid; i < g.n * 3; i += 256) cl[i] = 0.0f;
        if (tid == 0) {
            if (n_out) n_out[s] = 0;
            if (origo_out) origo_out[s] = g.origo;
            if (status_out) status_out[s] = status;
        }
        return;
    }

    // ---- prologue: the window into LDS, then one lane integrates it ----
    for (int k = tid; k < ni * 4; k += 256) s_win[k] = w[k];
    __syncthreads();
    if (tid == 0) {
        int cur = 0;                                                           // :202
        if (g.use_imu) {
            for (int i = 0; i < ni; ++i) {                                     // :207
                const double t = s_win[4 * i];                                 // :210
                if (t < t_start) {                                             // :212
                    if (cur == 0) {                                            // :215-222
                        s_win[1] = 0.0;
                        s_win[2] = 0.0;
                        s_win[3] = 0.0;
                        s_win[0] = t;
                        ++cur;
                    }
                    continue;
                }
                if (t > t_end) break;                                          // :227-228
                const double ax = s_win[4 * i + 1], ay = s_win[4 * i + 2], az = s_win[4 * i + 3];  // :231-234
                // the integrated entry cur overwrites a staged sample already read (cur <= i)
                const double dt = t - s_win[4 * (cur - 1)];                    // :237
                s_win[4 * cur + 1] = s_win[4 * (cur - 1) + 1] + ax * dt;       // :238-240
                s_win[4 * cur + 2] = s_win[4 * (cur - 1) + 2] + ay * dt;
                s_win[4 * cur + 3] = s_win[4 * (cur - 1) + 3] + az * dt;
                s_win[4 * cur] = t;                                            // :241
                ++cur;                                                         // :242
            }
            --cur;                                                             // :246
        }
        s_cur = cur;
        float ix = 0.0f, iy = 0.0f, iz = 0.0f;                                 // :76-78
        double ot0 = 0.0, ot1 = 0.0;
        if (g.use_odom) {
            const double *o = odom + (size_t)s * 14;
            ot0 = o[0];                                                        // :301-302
            ot1 = o[7];
            const UdAffine tb = ud_get_transformation((float)o[1], (float)o[2], (float)o[3], (float)o[4], (float)o[5],
                                                      (float)o[6]);            // :311-315
            const UdAffine te = ud_get_transformation((float)o[8], (float)o[9], (float)o[10], (float)o[11],
                                                      (float)o[12], (float)o[13]);  // :321-325
            const UdAffine bt = ud_mul(ud_inverse(tb), te);                    // :328
            ix = bt.m[3];                                                      // :332-334: the translation; the Euler
            iy = bt.m[7];                                                      // increments are not used by the node
            iz = bt.m[11];
        }
        s_inc[0] = ix;
        s_inc[1] = iy;
        s_inc[2] = iz;
        s_ot[0] = ot0;
        s_ot[1] = ot1;
    }

    // ---- the first beam that passes :350-353 fixes transStartInverse (:374-380) ----
    int wfirst = INT_MAX;
    for (int b0 = 0; b0 < g.n; b0 += 256) {
        const int i = b0 + tid;
        const bool v = i < g.n && ud_beam_valid(g, r[i]);
        const unsigned long long m = __ballot(v);
        if (m != 0ull && wfirst == INT_MAX) wfirst = b0 + wv * 64 + __ffsll((long long)m) - 1;
    }
    if (lane == 0) s_first[wv] = wfirst;
    __syncthreads();  // s_first, and the prologue's s_win / s_cur / s_inc / s_ot
    UdMotion mo;
    mo.win = s_win;
    mo.cur = s_cur;
    mo.inc[0] = s_inc[0];
    mo.inc[1] = s_inc[1];
    mo.inc[2] = s_inc[2];
    mo.t0 = s_ot[0];
    mo.t1 = s_ot[1];
    const int first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
    if (tid == 0 && first < g.n) {
        const double pt = t_start + (double)first * t_inc;                     // :358
        const UdAffine tsi = ud_inverse(ud_pose_at(g, mo, pt));                // :376-378
        for (int k = 0; k < 12; ++k) s_tsi[k] = tsi.m[k];
    }
    __syncthreads();
    UdAffine tsi;
    for (int k = 0; k < 12; ++k) tsi.m[k] = s_tsi[k];  // (unset when no beam is valid: then never used)

    // ---- per beam (:347-394), then the DataContainer compaction in beam order ----
    float2 *out = xy ? xy + (size_t)s * xy_stride : nullptr;
    int base = 0;
    for (int b0 = 0; b0 < g.n; b0 += 256) {
        const int i = b0 + tid;
        float px = 0.0f, py = 0.0f, pz = 0.0f;  // an invalid beam keeps the resized cloud's zero point (:139)
        bool keep = false;
        float2 p = make_float2(0.0f, 0.0f);
        if (i < g.n) {
            const float ri = r[i];
            if (ud_beam_valid(g, ri)) {                                        // :350-353
                const double pt = t_start + (double)i * t_inc;                 // :358
                const double2 u = cs[i];
                const double x = (double)ri * u.x;                             // :361-362
                const double y = (double)ri * u.y;
                const double z = 1.0;                                          // :343
                const UdAffine tfin = ud_pose_at(g, mo, pt);                   // :383-384
                const UdAffine bt = ud_mul(tsi, tfin);                         // :387
                px = (float)((double)bt.m[0] * x + (double)bt.m[1] * y + (double)bt.m[2] * z + (double)bt.m[3]);    // :391
                py = (float)((double)bt.m[4] * x + (double)bt.m[5] * y + (double)bt.m[6] * z + (double)bt.m[7]);    // :392
                pz = (float)((double)bt.m[8] * x + (double)bt.m[9] * y + (double)bt.m[10] * z + (double)bt.m[11]);  // :393
                if (out) keep = ud_container_point(g, px, py, pz, p);
            } else if (out) {
                keep = ud_container_point(g, 0.0f, 0.0f, 0.0f, p);  // the cloud's zero points pass through the loop too
            }
            if (cl) {
                cl[3 * i] = px;
                cl[3 * i + 1] = py;
                cl[3 * i + 2] = pz;
            }
        }
        if (out) {  // (uniform) order-preserving compaction: wave ballots + a prefix over the 4 waves
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_w[wv] = __popcll(m);
            __syncthreads();
            int off = base;
            for (int k = 0; k < wv; ++k) off += s_w[k];
            if (keep) {
                const int k = off + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                out[k] = p;
            }
            base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (n_out) n_out[s] = base;
        if (origo_out) origo_out[s] = g.origo;                                 // hector_slam.cc:329
        if (status_out) status_out[s] = 0;
    }
}

}  // namespace s2d
