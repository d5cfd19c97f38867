/* tests/ref/undistort_ref.c -- CPU restatement of lesson5's LidarUndistortion (test infrastructure).
 *
 * lesson5/src/lidar_undistortion.cc:96-447 scalar by scalar, one scan per call, in a plain loop: the integration
 * loop of PruneImuDeque (:202-246), the increment of PruneOdomDeque (:304-334), CorrectLaserScan (:339-395) with
 * ComputeRotation (:398-432, the reference's linear search) and ComputePosition (:435-447); then
 * rosPointCloudToDataContainer (lesson4/src/hector_mapping/hector_slam.cc:320-362) over the corrected cloud.
 * The GPU kernel (csrc/undistort_kernels.hip) must equal this bit for bit.
 *
 * PCL / Eigen are absent, so the float pieces are fixed as DESIGN.md section 3 states them (parity unpinned):
 * pcl::getTransformation, Affine3f::inverse, the Affine3f product, dot products left to right, float sin / cos
 * from csrc/detmath.h.  Build: gcc -O2 -ffp-contract=off -shared -fPIC -I csrc.
 */
#include <math.h>
#include <string.h>

#include "detmath.h"

#define QUEUE_LENGTH 2000 /* :20 */

typedef struct {
    float m[3][4]; /* Eigen::Affine3f: [L | t] */
} affine;

/* pcl::getTransformation (PCL common/impl/eigen.hpp), float */
static affine get_transformation(float x, float y, float z, float roll, float pitch, float yaw)
{
    float A = sdm_cosf(yaw), B = sdm_sinf(yaw), C = sdm_cosf(pitch), D = sdm_sinf(pitch);
    float E = sdm_cosf(roll), F = sdm_sinf(roll), DE = D * E, DF = D * F;
    affine t;
    t.m[0][0] = A * C;
    t.m[0][1] = A * DF - B * E;
    t.m[0][2] = B * F + A * DE;
    t.m[0][3] = x;
    t.m[1][0] = B * C;
    t.m[1][1] = A * E + B * DF;
    t.m[1][2] = B * DE - A * F;
    t.m[1][3] = y;
    t.m[2][0] = -D;
    t.m[2][1] = C * F;
    t.m[2][2] = C * E;
    t.m[2][3] = z;
    return t;
}

static float cofactor(const affine *a, int i, int j)
{
    int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return a->m[i1][j1] * a->m[i2][j2] - a->m[i1][j2] * a->m[i2][j1];
}

/* Affine3f::inverse(): inverse(j, i) = cofactor(i, j) / det, translation -(L^-1 t) */
static affine inverse(const affine *a)
{
    float c00 = cofactor(a, 0, 0), c10 = cofactor(a, 1, 0), c20 = cofactor(a, 2, 0);
    float det = c00 * a->m[0][0] + c10 * a->m[1][0] + c20 * a->m[2][0];
    float invdet = 1.0f / det;
    affine r;
    int i, j;
    r.m[0][0] = c00 * invdet;
    r.m[0][1] = c10 * invdet;
    r.m[0][2] = c20 * invdet;
    for (j = 1; j < 3; ++j)
        for (i = 0; i < 3; ++i) r.m[j][i] = cofactor(a, i, j) * invdet;
    for (i = 0; i < 3; ++i)
        r.m[i][3] = -(r.m[i][0] * a->m[0][3] + r.m[i][1] * a->m[1][3] + r.m[i][2] * a->m[2][3]);
    return r;
}

/* Affine3f * Affine3f */
static affine mul(const affine *a, const affine *b)
{
    affine r;
    int i, j;
    for (i = 0; i < 3; ++i) {
        for (j = 0; j < 3; ++j) r.m[i][j] = a->m[i][0] * b->m[0][j] + a->m[i][1] * b->m[1][j] + a->m[i][2] * b->m[2][j];
        r.m[i][3] = a->m[i][0] * b->m[0][3] + a->m[i][1] * b->m[1][3] + a->m[i][2] * b->m[2][3] + a->m[i][3];
    }
    return r;
}

typedef struct {
    int current_imu_index_;
    double imu_time_[QUEUE_LENGTH], imu_rot_x_[QUEUE_LENGTH], imu_rot_y_[QUEUE_LENGTH], imu_rot_z_[QUEUE_LENGTH];
    double start_odom_time_, end_odom_time_;
    float odom_incre_x_, odom_incre_y_, odom_incre_z_;
} state;

/* ComputeRotation :398-432 */
static void compute_rotation(const state *st, double pointTime, float *rotXCur, float *rotYCur, float *rotZCur)
{
    int imuPointerFront = 0;
    *rotXCur = 0;
    *rotYCur = 0;
    *rotZCur = 0;
    while (imuPointerFront < st->current_imu_index_) { /* :406-411 */
        if (pointTime < st->imu_time_[imuPointerFront]) break;
        ++imuPointerFront;
    }
    if (pointTime > st->imu_time_[imuPointerFront] || imuPointerFront == 0) { /* :414-419 */
        *rotXCur = (float)st->imu_rot_x_[imuPointerFront];
        *rotYCur = (float)st->imu_rot_y_[imuPointerFront];
        *rotZCur = (float)st->imu_rot_z_[imuPointerFront];
    } else {
        int imuPointerBack = imuPointerFront - 1; /* :422 */
        double ratioFront = (pointTime - st->imu_time_[imuPointerBack]) /
                            (st->imu_time_[imuPointerFront] - st->imu_time_[imuPointerBack]); /* :425 */
        double ratioBack = (st->imu_time_[imuPointerFront] - pointTime) /
                           (st->imu_time_[imuPointerFront] - st->imu_time_[imuPointerBack]); /* :426 */
        *rotXCur = (float)(st->imu_rot_x_[imuPointerFront] * ratioFront + st->imu_rot_x_[imuPointerBack] * ratioBack);
        *rotYCur = (float)(st->imu_rot_y_[imuPointerFront] * ratioFront + st->imu_rot_y_[imuPointerBack] * ratioBack);
        *rotZCur = (float)(st->imu_rot_z_[imuPointerFront] * ratioFront + st->imu_rot_z_[imuPointerBack] * ratioBack);
    }
}

/* ComputePosition :435-447 */
static void compute_position(const state *st, double pointTime, float *posXCur, float *posYCur, float *posZCur)
{
    double ratioFront = (pointTime - st->start_odom_time_) / (st->end_odom_time_ - st->start_odom_time_); /* :442 */
    *posXCur = (float)(st->odom_incre_x_ * ratioFront); /* :444-446 */
    *posYCur = (float)(st->odom_incre_y_ * ratioFront);
    *posZCur = (float)(st->odom_incre_z_ * ratioFront);
}

/* CreateAngleCache :162-174: angle_min and angle_increment are float32 message fields, so the sum is a float */
void udr_unit_vectors(int n, float angle_min, float angle_increment, double *cs)
{
    unsigned int i;
    for (i = 0; i < (unsigned int)n; i++) {
        double angle = angle_min + i * angle_increment; /* :170 */
        cs[2 * i] = cos(angle);
        cs[2 * i + 1] = sin(angle);
    }
}

/* One ScanCallback.
 *   scan:   ranges[n], cs[2n] unit vectors, range_min / range_max, t_start, t_inc
 *   imu:    imu_n samples (t, wx, wy, wz), the queue after the node's trimming; odom: start / end records
 *           (t, x, y, z, roll, pitch, yaw), a NaN time = no covering pair
 *   rules:  tf[12] (basis rows, origin), use_max_scan_range; frules: sqr_min, sqr_max, z_min, z_max, scale
 *   out:    cloud[3n], xy[2n], *n_out, origo[2]; returns the status (0 corrected, 1 wait IMU, 2 wait odom) */
int udr_correct(int n, const float *ranges, const double *cs, float range_min, float range_max, double t_start,
                double t_inc, int use_imu, const double *imu, int imu_n, int use_odom, const double *odom,
                const double *rules, const float *frules, float *cloud, float *xy, int *n_out, float *origo)
{
    static state st; /* (the restatement is single-threaded test code) */
    const double *tf = rules;
    const double use_max = rules[12];
    const float sqr_min = frules[0], sqr_max = frules[1], z_min = frules[2], z_max = frules[3], scale = frules[4];
    double scan_count_ = n; /* a double in the node */
    double t_end = t_start + t_inc * (scan_count_ - 1); /* :156 */
    int i, count = 0, first_point_flag = 1;
    affine transStartInverse, transFinal, transBt;

    memset(cloud, 0, sizeof(float) * 3 * (size_t)n); /* :62, :139: cleared, then resized */
    *n_out = 0;
    origo[0] = (float)tf[9] * scale; /* hector_slam.cc:329 */
    origo[1] = (float)tf[10] * scale;
    memset(&st, 0, sizeof(st)); /* ResetParameters :60-79 */

    if (use_imu) { /* PruneImuDeque */
        if (imu_n <= 0 || imu_n > QUEUE_LENGTH || imu[0] > t_start || imu[4 * (imu_n - 1)] < t_end) return 1; /* :182-188 */
        if (!(imu[0] < t_start)) return 1; /* :237 would read imu_time_[-1] */
        st.current_imu_index_ = 0; /* :202 */
        for (i = 0; i < imu_n; i++) { /* :207 */
            double current_imu_time = imu[4 * i], time_diff;
            if (current_imu_time < t_start) { /* :212 */
                if (st.current_imu_index_ == 0) {
                    st.imu_rot_x_[0] = 0;
                    st.imu_rot_y_[0] = 0;
                    st.imu_rot_z_[0] = 0;
                    st.imu_time_[0] = current_imu_time;
                    ++st.current_imu_index_;
                }
                continue;
            }
            if (current_imu_time > t_end) break; /* :227 */
            time_diff = current_imu_time - st.imu_time_[st.current_imu_index_ - 1]; /* :237 */
            st.imu_rot_x_[st.current_imu_index_] = st.imu_rot_x_[st.current_imu_index_ - 1] + imu[4 * i + 1] * time_diff;
            st.imu_rot_y_[st.current_imu_index_] = st.imu_rot_y_[st.current_imu_index_ - 1] + imu[4 * i + 2] * time_diff;
            st.imu_rot_z_[st.current_imu_index_] = st.imu_rot_z_[st.current_imu_index_ - 1] + imu[4 * i + 3] * time_diff;
            st.imu_time_[st.current_imu_index_] = current_imu_time;
            ++st.current_imu_index_;
        }
        --st.current_imu_index_; /* :246 */
    }
    if (use_odom) { /* PruneOdomDeque */
        affine transBegin, transEnd, inv, bt;
        if (odom[0] != odom[0] || odom[7] != odom[7]) return 2; /* :257-263, :274-275 */
        st.start_odom_time_ = odom[0]; /* :301-302 */
        st.end_odom_time_ = odom[7];
        transBegin = get_transformation((float)odom[1], (float)odom[2], (float)odom[3], (float)odom[4], (float)odom[5],
                                        (float)odom[6]); /* :311-315 */
        transEnd = get_transformation((float)odom[8], (float)odom[9], (float)odom[10], (float)odom[11], (float)odom[12],
                                      (float)odom[13]); /* :321-325 */
        inv = inverse(&transBegin);
        bt = mul(&inv, &transEnd); /* :328 */
        st.odom_incre_x_ = bt.m[0][3]; /* :332-334 */
        st.odom_incre_y_ = bt.m[1][3];
        st.odom_incre_z_ = bt.m[2][3];
    }

    memset(&transStartInverse, 0, sizeof(transStartInverse));
    for (i = 0; i < n; i++) { /* CorrectLaserScan :347 */
        double current_point_time, current_point_x, current_point_y, current_point_z = 1.0;
        float rotXCur = 0, rotYCur = 0, rotZCur = 0, posXCur = 0, posYCur = 0, posZCur = 0;
        if (!isfinite(ranges[i]) || ranges[i] < range_min || ranges[i] > range_max) continue; /* :350-353 */
        current_point_time = t_start + i * t_inc; /* :358 */
        current_point_x = ranges[i] * cs[2 * i]; /* :361-362 */
        current_point_y = ranges[i] * cs[2 * i + 1];
        if (use_imu) compute_rotation(&st, current_point_time, &rotXCur, &rotYCur, &rotZCur);
        if (use_odom) compute_position(&st, current_point_time, &posXCur, &posYCur, &posZCur);
        if (first_point_flag) { /* :374-380 */
            affine t0 = get_transformation(posXCur, posYCur, posZCur, rotXCur, rotYCur, rotZCur);
            transStartInverse = inverse(&t0);
            first_point_flag = 0;
        }
        transFinal = get_transformation(posXCur, posYCur, posZCur, rotXCur, rotYCur, rotZCur); /* :383 */
        transBt = mul(&transStartInverse, &transFinal); /* :387 */
        cloud[3 * i] = (float)(transBt.m[0][0] * current_point_x + transBt.m[0][1] * current_point_y +
                               transBt.m[0][2] * current_point_z + transBt.m[0][3]); /* :391 */
        cloud[3 * i + 1] = (float)(transBt.m[1][0] * current_point_x + transBt.m[1][1] * current_point_y +
                                   transBt.m[1][2] * current_point_z + transBt.m[1][3]); /* :392 */
        cloud[3 * i + 2] = (float)(transBt.m[2][0] * current_point_x + transBt.m[2][1] * current_point_y +
                                   transBt.m[2][2] * current_point_z + transBt.m[2][3]); /* :393 */
    }

    for (i = 0; i < n; ++i) { /* rosPointCloudToDataContainer, hector_slam.cc:331-358 */
        float x = cloud[3 * i], y = cloud[3 * i + 1], z = cloud[3 * i + 2];
        float dist_sqr = x * x + y * y; /* :335 */
        if ((dist_sqr > sqr_min) && (dist_sqr < sqr_max)) {
            double bx, by, bz;
            float pointPosLaserFrameZ;
            if ((x < 0.0f) && (dist_sqr < 0.50f)) continue;
            if (dist_sqr > use_max * use_max) continue; /* :344 */
            bx = tf[0] * x + tf[1] * y + tf[2] * z + tf[9]; /* :348 */
            by = tf[3] * x + tf[4] * y + tf[5] * z + tf[10];
            bz = tf[6] * x + tf[7] * y + tf[8] * z + tf[11];
            pointPosLaserFrameZ = (float)(bz - tf[11]); /* :351 */
            if (pointPosLaserFrameZ > z_min && pointPosLaserFrameZ < z_max) {
                xy[2 * count] = (float)bx * scale; /* :356 */
                xy[2 * count + 1] = (float)by * scale;
                ++count;
            }
        }
    }
    *n_out = count;
    return 0;
}
