// karto_pose_math.h -- open_karto's Pose2 / Matrix3 arithmetic as the Karto graph-linking stage (karto_link_kernels.hip)
// and the scan-intake stage (karto_process_kernels.hip) share it: every operation written as the reference writes it,
// left to right, IEEE double with -ffp-contract=off and detmath.h's sin / cos (include/slam2d/karto_link.h, ARITHMETIC).
#pragma once
#include <math.h>
#include <stdint.h>

#include "detmath.h"

namespace s2d {

#define KE_FN __host__ __device__ static inline

constexpr double KE_PI = 3.14159265358979323846;   // KT_PI, Math.h:32
constexpr double KE_2PI = 6.28318530717958647692;  // KT_2PI, Math.h:33

// math::NormalizeAngle (Math.h:182-210).  Beyond 2^32 rad, or not finite: NaN (the reference does not terminate).
KE_FN double ke_normalize_angle(double angle)
{
    if (!(fabs(angle) < 4294967296.0)) return __builtin_nan("");
    while (angle < -KE_PI) {
        if (angle < -KE_2PI) angle += (double)(uint32_t)(angle / -KE_2PI) * KE_2PI;
        else angle += KE_2PI;
    }
    while (angle > KE_PI) {
        if (angle > KE_2PI) angle -= (double)(uint32_t)(angle / KE_2PI) * KE_2PI;
        else angle -= KE_2PI;
    }
    return angle;
}

// Matrix3::FromAxisAngle (Karto.h:2392-2421), every operation kept
KE_FN void ke_from_axis_angle(double x, double y, double z, double radians, double *m)
{
    const double cosRadians = sdm_cos(radians);
    const double sinRadians = sdm_sin(radians);
    const double oneMinusCos = 1.0 - cosRadians;
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xyMCos = x * y * oneMinusCos;
    const double xzMCos = x * z * oneMinusCos;
    const double yzMCos = y * z * oneMinusCos;
    const double xSin = x * sinRadians, ySin = y * sinRadians, zSin = z * sinRadians;
    m[0] = xx * oneMinusCos + cosRadians;
    m[1] = xyMCos - zSin;
    m[2] = xzMCos + ySin;
    m[3] = xyMCos + zSin;
    m[4] = yy * oneMinusCos + cosRadians;
    m[5] = yzMCos - xSin;
    m[6] = xzMCos - ySin;
    m[7] = yzMCos + xSin;
    m[8] = zz * oneMinusCos + cosRadians;
}

// Matrix3::operator* (Karto.h:2552-2567)
KE_FN void ke_mul(const double *a, const double *b, double *p)
{
    for (int row = 0; row < 3; ++row)
        for (int col = 0; col < 3; ++col)
            p[3 * row + col] = a[3 * row] * b[col] + a[3 * row + 1] * b[3 + col] + a[3 * row + 2] * b[6 + col];
}

// Matrix3 * Pose2 (Karto.h:2574-2583)
KE_FN void ke_mul_pose(const double *m, const double *p, double *out)
{
    out[0] = m[0] * p[0] + m[1] * p[1] + m[2] * p[2];
    out[1] = m[3] * p[0] + m[4] * p[1] + m[5] * p[2];
    out[2] = m[6] * p[0] + m[7] * p[1] + m[8] * p[2];
}

// Matrix3::Inverse through InverseFast(kInverse, 1e-14) (Karto.h:2445-2493); false where the reference asserts, and
// for a NaN determinant
KE_FN bool ke_inverse(const double *m, double *inv)
{
    inv[0] = m[4] * m[8] - m[5] * m[7];
    inv[1] = m[2] * m[7] - m[1] * m[8];
    inv[2] = m[1] * m[5] - m[2] * m[4];
    inv[3] = m[5] * m[6] - m[3] * m[8];
    inv[4] = m[0] * m[8] - m[2] * m[6];
    inv[5] = m[2] * m[3] - m[0] * m[5];
    inv[6] = m[3] * m[7] - m[4] * m[6];
    inv[7] = m[1] * m[6] - m[0] * m[7];
    inv[8] = m[0] * m[4] - m[1] * m[3];
    const double fDet = m[0] * inv[0] + m[1] * inv[3] + m[2] * inv[6];
    if (!(fabs(fDet) > 1e-14)) return false;
    const double fInvDet = 1.0 / fDet;
    for (int k = 0; k < 9; ++k) inv[k] *= fInvDet;
    return true;
}

}  // namespace s2d
