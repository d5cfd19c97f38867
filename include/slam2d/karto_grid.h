/* include/slam2d/karto_grid.h -- C-ABI of the MI355X Karto occupancy-grid rebuild (lesson6, config 5).
 *
 * Reference: karto::OccupancyGrid::CreateFromScans (lesson6/lib/open_karto/include/open_karto/Karto.h
 * :5659-5673), the one producer of SlamKarto::updateMap's /map (lesson6/src/karto_slam.cc:507-581): every
 * processed scan of the graph is re-traced at its (corrected) pose.
 *
 *   kg_build[_device]  ComputeDimensions (Karto.h:5804-5822) over the scans' bounding boxes
 *                      (LocalizedRangeScan::Update, :5362-5425), then per scan AddScan (:5852-5899) ->
 *                      RayTrace (:5910-5945) -> Grid::TraceLine (:4680-4745) into the pass / hit
 *                      counters, then Update / UpdateCell (:5953-5990)
 *   kg_get_map         the grid's cells (GridStates: 0 unknown, 100 occupied, 255 free), the
 *                      nav_msgs/OccupancyGrid bytes karto_slam.cc:546-569 makes of them (-1 / 100 / 0)
 *                      and both counter planes
 *
 * open_karto needs boost (Karto.h:37), absent from this image, so it is not built here: the CPU
 * restatement tests/ref/karto_grid_ref.c restates the sequence and parity is UNPINNED against the
 * library itself, as for the matcher (karto.h, DESIGN.md "Karto").  The GPU planes, dimensions and
 * offset equal the restatement's bit for bit: the counters are integers, so the sum is order-free.
 *
 * Conventions as in karto.h: plain C types, int status (KG_OK / negative), kg_last_error().  A scan is
 * n_readings doubles plus its sensor pose (x, y, heading); the laser offset is identity.  All four planes
 * are dense width x height, row-major (index y * width + x); the reference's 8-aligned row stride is
 * not part of the output.
 */
#ifndef SLAM2D_KARTO_GRID_H
#define SLAM2D_KARTO_GRID_H

#include <stddef.h>
#include <stdint.h>

#include "karto.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KG_OK 0
#define KG_EINVAL (-1)
#define KG_EHIP (-2)
#define KG_ENOMEM (-3)
#define KG_ENODEV (-4)
#define KG_ERANGE (-5) /* width * height exceeds the context's max_cells (kg_info still holds the dimensions) */

/* OccupancyGrid's parameters and the one LaserRangeFinder field kt_laser lacks. */
typedef struct kg_params {
    double resolution;          /* m per cell (karto_slam.cc resolution_, 0.05) */
    double maximum_range;       /* m: LaserRangeFinder::GetMaximumRange (scan->range_max, karto_slam.cc:389-395) */
    double occupancy_threshold; /* OccupancyThreshold 0.1: occupied if hits / pass > this */
    uint32_t min_pass_through;  /* MinPassThrough 2: a cell is classified if pass > this */
    int pad_;
} kg_params;

/* ComputeDimensions' results. */
typedef struct kg_info {
    int width, height;         /* cells */
    double offset_x, offset_y; /* world coordinates of cell (0, 0): the bounding box minimum */
    int status;                /* the build's return value */
    int pad_;
} kg_info;

typedef struct kg_ctx kg_ctx;

const char *kg_last_error(void);
/* resolution 0.05, occupancy_threshold 0.1, min_pass_through 2; maximum_range 0, which kg_create
 * rejects: the caller must set it. */
void kg_default_params(kg_params *params);

/* A builder for up to max_scans scans and maps of up to max_cells cells (<= 2^28).  KG_EINVAL for a
 * resolution or maximum_range that is not > 0 (the reference throws on resolution 0) and for
 * range_threshold / resolution above 2^20 cells. */
int kg_create(kg_ctx **out, const kt_laser *laser, const kg_params *params, int max_scans, size_t max_cells);
int kg_destroy(kg_ctx *ctx);

/* OccupancyGrid::CreateFromScans(scans, resolution): ranges double[count][n_readings], poses
 * double[count][3].  The bounding boxes are reduced on the device; their four doubles come back to the
 * host, which computes width, height and offset (math::Round) and sizes the launches: that copy is the
 * call's ONE synchronisation with the stream.  kg_build_device returns after enqueueing the rest
 * (d_ranges / d_poses must stay valid until the stream has run it); kg_build also waits for it.
 *   count == 0                      KG_EINVAL (the reference returns NULL: no grid)
 *   width * height > max_cells      KG_ERANGE, *info valid, the context's map empty: re-create larger
 *   width == 0 || height == 0       KG_OK, an empty map, nothing launched
 */
int kg_build(kg_ctx *ctx, int count, const double *ranges, const double *poses, kg_info *info);
int kg_build_device(kg_ctx *ctx, int count, const double *d_ranges, const double *d_poses, kg_info *info,
                    void *hip_stream);

/* The last build's planes into host arrays of width * height elements; any may be NULL.  Waits for the
 * build. */
int kg_get_map(kg_ctx *ctx, uint8_t *state, int8_t *ros, uint32_t *pass, uint32_t *hits);
/* Zero-copy readers: the context's device planes (valid after the build's stream work, until the next
 * build or kg_destroy); any may be NULL. */
int kg_device_planes(kg_ctx *ctx, const uint8_t **d_state, const int8_t **d_ros, const uint32_t **d_pass,
                     const uint32_t **d_hits);

int kg_set_timing(kg_ctx *ctx, int enable);
/* Accumulated device time per kernel: names kg_kernel_name(i), i < kg_num_kernels(). */
int kg_num_kernels(void);
const char *kg_kernel_name(int i);
int kg_get_kernel_times(kg_ctx *ctx, double *ms_out, int64_t *launches_out, int reset);

#ifdef __cplusplus
}
#endif

#endif
