/* include/slam2d/undistort.h -- C-ABI of the MI355X lidar motion-undistortion path (lesson5).
 *
 * Reference: lesson5's LidarUndistortion (lesson5/src/lidar_undistortion.cc:96-447).  ScanCallback integrates
 * the IMU's angular velocity over the sweep (PruneImuDeque :177-249), takes the odometry increment between the
 * records around it (PruneOdomDeque :252-336) and moves every beam into the frame the scanner had at the
 * scan's first valid point (CorrectLaserScan :339-395).  Here that runs for a batch of scans in one kernel
 * launch (ud_correct_kernel, one workgroup per scan), and the corrected cloud can leave the kernel a second
 * time as Hector DataContainer points (rosPointCloudToDataContainer, lesson4/src/hector_mapping/
 * hector_slam.cc:320-362) in the layout hs_step_batch_device takes.
 *
 * PCL and Eigen are not part of this build: pcl::getTransformation, Affine3f::inverse and the Affine3f product
 * are evaluated in a fixed float operation order with the library's own sin / cos --
 * PARITY UNPINNED against a PCL build.
 *
 * What stays on the host: the message queues.  The caller trims its IMU queue as the node does (:191-197),
 * hands the remaining window over as (t, wx, wy, wz) doubles, and picks the start / end odometry records
 * (:280-296) as (t, x, y, z, roll, pitch, yaw) doubles (ud_rpy_from_quaternion gives the angles).
 * slam2d.undistort.LidarUndistortion is that host side in Python.
 *
 * Conventions as in hector.h: plain C types, int status (UD_OK / negative), ud_last_error(); *_device entry
 * points take device pointers and a hipStream_t (as void*, NULL = the context's own stream) and do not
 * synchronise.
 *
 * Per-scan status (d_status / status_out): the scans for which ScanCallback returns early.
 *   UD_SCAN_OK        0  corrected
 *   UD_SCAN_WAIT_IMU  1  use_imu and: the window is empty (:182), its first sample is later than the scan
 *                        start (:183), its last sample is earlier than the scan end (:184), or its first
 *                        sample is not strictly earlier than the scan start (the reference would then read
 *                        imu_time_[-1] at :237); also a device-side sample count outside [0, max_imu]
 *   UD_SCAN_WAIT_ODOM 2  use_odom and no covering odometry pair (:257-263, :274-275): the caller marks this
 *                        by a NaN time in the start or the end record
 * Such a scan gets a zeroed cloud and an empty DataContainer (n = 0).
 */
#ifndef SLAM2D_UNDISTORT_H
#define SLAM2D_UNDISTORT_H

#include <stddef.h>
#include <stdint.h>

#include "hector.h" /* hs_laser: the DataContainer rules */

#ifdef __cplusplus
extern "C" {
#endif

#define UD_OK 0
#define UD_EINVAL (-1)
#define UD_EHIP (-2)
#define UD_ENOMEM (-3)
#define UD_ENODEV (-4)

#define UD_SCAN_OK 0
#define UD_SCAN_WAIT_IMU 1
#define UD_SCAN_WAIT_ODOM 2

#define UD_MAX_IMU 2000 /* queueLength (lidar_undistortion.cc:20): the size of imu_time_ / imu_rot_*_ */

typedef struct ud_ctx ud_ctx;

const char *ud_version(void);
const char *ud_last_error(void);

/* LidarUndistortion ctor (:22-53) for num_streams scanners of n_beams ranges each; max_imu bounds the IMU
 * window of one scan (1 <= max_imu <= UD_MAX_IMU; more is UD_EINVAL).  Defaults: use_imu and use_odom on
 * (:27-28), no scan geometry (ud_set_scan_geometry must follow), ud_default_laser's container rules at
 * scale_to_map 20 (a 0.05 m map). */
int ud_create(ud_ctx **out, int num_streams, int n_beams, int max_imu);
int ud_destroy(ud_ctx *ctx);
/* The LaserScan fields the node reads (:170, :350-352) and CreateAngleCache (:162-174).  unit_vectors:
 * 2*n_beams doubles (cos_i, sin_i), or NULL to compute them here as the node does: host libm cos / sin of
 * the FLOAT sum angle_min + i * angle_increment (:170 adds two float32 fields). */
int ud_set_scan_geometry(ud_ctx *ctx, float angle_min, float angle_increment, float range_min, float range_max,
                         const double *unit_vectors);
/* hs_default_laser with the z window moved to (0, 2): CorrectLaserScan keeps current_point_z = 1.0 (:343), so
 * the corrected cloud sits at z = 1 (a quirk kept in the cloud), and Hector's default window (-1, 1)
 * (hector_slam.cc:157-161, strict comparisons at :353) would drop every point of it. */
void ud_default_laser(hs_laser *laser, int n_beams, float angle_min, float angle_increment);
/* The rules of the DataContainer output: basis, origin, sqr_laser_min/max_dist, use_max_scan_range and the
 * z window of `laser` (its n_beams, angles, range_min and range_cutoff are not used: the cloud is already
 * projected), and getScaleToMap of the Hector context the points go to. */
int ud_set_container_rules(ud_ctx *ctx, const hs_laser *laser, float scale_to_map);
/* The node's use_imu / use_odometry parameters (:27-28). */
int ud_set_sources(ud_ctx *ctx, int use_imu, int use_odom);

/* ScanCallback (:96-124) for `count` scans (count <= num_streams), one workgroup each:
 *   d_ranges    float[count][range_stride]    LaserScan ranges
 *   d_scan_time double[count][2]              current_scan_time_start_, current_scan_time_increment_ (:154-155)
 *   d_imu       double[count][imu_stride][4]  the trimmed IMU queue: t, angular velocity x, y, z
 *   d_imu_n     int[count]                    samples in each window
 *   d_odom      double[count][2][7]           start_odom_msg_, end_odom_msg_: t, x, y, z, roll, pitch, yaw
 *   d_cloud     float[count][cloud_stride][3] corrected_pointcloud_ (:391-393); invalid beams (0, 0, 0)
 *   d_xy, d_n, d_origo                        the DataContainer, as hs_step_batch_device takes it
 *   d_status    int[count]                    UD_SCAN_*
 * d_imu / d_imu_n may be NULL with use_imu off, d_odom with use_odom off.  Either output may be NULL:
 * d_cloud, or d_xy with d_n and d_origo; d_origo and d_status may be NULL by themselves. */
int ud_correct_batch_device(ud_ctx *ctx, int count, const float *d_ranges, int range_stride,
                            const double *d_scan_time, const double *d_imu, int imu_stride, const int *d_imu_n,
                            const double *d_odom, float *d_cloud, int cloud_stride, float *d_xy, int xy_stride,
                            int *d_n, float *d_origo, int *d_status, void *hip_stream);
/* ScanCallback for one scan from host memory (the ROS drop-in entry point; synchronises).  imu: imu_n
 * samples of 4 doubles, times non-decreasing (UD_EINVAL otherwise); odom: 2 records of 7 doubles.
 * cloud_out float[n_beams][3], xy_out float[n_beams][2], n_out, origo_out float[2], status_out: any may be NULL. */
int ud_correct(ud_ctx *ctx, const float *ranges, double scan_time_start, double scan_time_increment,
               const double *imu, int imu_n, const double *odom, float *cloud_out, float *xy_out, int *n_out,
               float *origo_out, int *status_out);
/* tf::Matrix3x3(q).getRPY(roll, pitch, yaw) (:308-309, :318-319) of q = (x, y, z, w), host libm. */
int ud_rpy_from_quaternion(const double q[4], double rpy[3]);
/* The context's own HIP stream (hipStream_t as void*). */
void *ud_get_stream(ud_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
