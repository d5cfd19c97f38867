/* tests/ref/karto_grid_ref.c -- CPU restatement of karto::OccupancyGrid::CreateFromScans
 * (lesson6/lib/open_karto/include/open_karto/Karto.h:5659-5673) as SlamKarto::updateMap uses it
 * (lesson6/src/karto_slam.cc:507-581).  Test infrastructure: the sequence is restated statement by statement,
 * with the LITERAL TraceLine loop (Karto.h:4680-4745), not the closed form the kernels use.  open_karto needs
 * boost and is not built here, so parity with the library itself is unpinned; tests/test_karto_grid_cpu.py pins
 * this file to the reference text with hand-written cases.
 *
 * Built with gcc -O2 -ffp-contract=off; sin / cos are csrc/detmath.h's, as in the kernels.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "detmath.h"

#define KT_TOLERANCE 1e-06

typedef struct kgr_laser {
    double minimum_angle, angular_resolution, minimum_range, range_threshold, maximum_range;
    int n_readings, pad_;
} kgr_laser;

/* math::Round (Math.h:87-90) */
static double kgr_round(double value) { return value >= 0.0 ? floor(value + 0.5) : ceil(value - 0.5); }
/* math::InRange (Math.h:172) */
static int kgr_in_range(double value, double a, double b) { return value >= a && value <= b; }

typedef struct kgr_box {
    double min_x, min_y, max_x, max_y;
} kgr_box;

/* BoundingBox2() (Karto.h:2765) */
static void kgr_box_init(kgr_box *b)
{
    b->min_x = b->min_y = 999999999999999999.99999;
    b->max_x = b->max_y = -999999999999999999.99999;
}
/* BoundingBox2::Add (Karto.h:2815-2819): Vector2::MakeFloor / MakeCeil */
static void kgr_box_add(kgr_box *b, double x, double y)
{
    if (x < b->min_x) b->min_x = x;
    if (y < b->min_y) b->min_y = y;
    if (x > b->max_x) b->max_x = x;
    if (y > b->max_y) b->max_y = y;
}

/* the point of beam i (Karto.h:5384-5388 / :5394-5398) */
static void kgr_point(const kgr_laser *L, const double *pose, int i, double r, double *x, double *y)
{
    const double angle = pose[2] + L->minimum_angle + (double)(uint32_t)i * L->angular_resolution;
    *x = pose[0] + (r * sdm_cos(angle));
    *y = pose[1] + (r * sdm_sin(angle));
}

/* LocalizedRangeScan::Update's bounding box (Karto.h:5418-5424) */
static void kgr_scan_box(const kgr_laser *L, const double *ranges, const double *pose, kgr_box *b)
{
    kgr_box_init(b);
    kgr_box_add(b, pose[0], pose[1]);
    for (int i = 0; i < L->n_readings; i++) {
        const double r = ranges[i];
        double x, y;
        if (!kgr_in_range(r, L->minimum_range, L->range_threshold)) continue;
        kgr_point(L, pose, i, r, &x, &y);
        kgr_box_add(b, x, y);
    }
}

/* ComputeDimensions (Karto.h:5804-5822).  dims = width, height; offset = the box minimum.
 * Returns 0 for an empty scan list (CreateFromScans returns NULL, :5661). */
int kgr_dimensions(const kgr_laser *L, int count, const double *ranges, const double *poses, double resolution,
                   int *dims, double *offset)
{
    kgr_box box;
    if (count <= 0) return 0;
    kgr_box_init(&box);
    for (int s = 0; s < count; s++) {
        kgr_box b;
        kgr_scan_box(L, ranges + (size_t)s * L->n_readings, poses + 3 * (size_t)s, &b);
        kgr_box_add(&box, b.min_x, b.min_y);
        kgr_box_add(&box, b.max_x, b.max_y);
    }
    const double scale = 1.0 / resolution;
    dims[0] = (int32_t)kgr_round((box.max_x - box.min_x) * scale);
    dims[1] = (int32_t)kgr_round((box.max_y - box.min_y) * scale);
    offset[0] = box.min_x;
    offset[1] = box.min_y;
    return 1;
}

typedef struct kgr_grid {
    int width, height;
    double off_x, off_y, scale;
    uint32_t *pass, *hits;
} kgr_grid;

static int kgr_valid(const kgr_grid *g, int x, int y) { return x >= 0 && x < g->width && y >= 0 && y < g->height; }

/* Grid<T>::TraceLine (Karto.h:4680-4745), literal.  If cells != NULL every emitted point (valid or not) is
 * also appended there as (x, y); returns the number of emitted points. */
static int kgr_trace_line(const kgr_grid *g, int x0, int y0, int x1, int y1, int *cells)
{
    int emitted = 0;
    const int steep = abs(y1 - y0) > abs(x1 - x0);
    int t;
    if (steep) {
        t = x0, x0 = y0, y0 = t;
        t = x1, x1 = y1, y1 = t;
    }
    if (x0 > x1) {
        t = x0, x0 = x1, x1 = t;
        t = y0, y0 = y1, y1 = t;
    }
    const int deltaX = x1 - x0;
    const int deltaY = abs(y1 - y0);
    int error = 0;
    int ystep;
    int y = y0;
    if (y0 < y1)
        ystep = 1;
    else
        ystep = -1;
    int pointX, pointY;
    for (int x = x0; x <= x1; x++) {
        if (steep) {
            pointX = y;
            pointY = x;
        } else {
            pointX = x;
            pointY = y;
        }
        error += deltaY;
        if (2 * error >= deltaX) {
            y += ystep;
            error -= deltaX;
        }
        if (cells) {
            cells[2 * emitted] = pointX;
            cells[2 * emitted + 1] = pointY;
        }
        emitted++;
        if (g && kgr_valid(g, pointX, pointY)) g->pass[(size_t)pointY * g->width + pointX]++;
    }
    return emitted;
}

/* the literal line's points, for the closed-form comparison; cells holds max(|dx|, |dy|) + 1 pairs */
int kgr_line_cells(int x0, int y0, int x1, int y1, int *cells) { return kgr_trace_line(NULL, x0, y0, x1, y1, cells); }

/* CoordinateConverter::WorldToGrid (Karto.h:4237-4252) */
static void kgr_world_to_grid(const kgr_grid *g, double wx, double wy, int *gx, int *gy)
{
    const double gridX = (wx - g->off_x) * g->scale;
    const double gridY = (wy - g->off_y) * g->scale;
    *gx = (int32_t)kgr_round(gridX);
    *gy = (int32_t)kgr_round(gridY);
}

/* OccupancyGrid::RayTrace (Karto.h:5910-5945), doUpdate = false */
static void kgr_ray_trace(const kgr_grid *g, double fx, double fy, double tx, double ty, int is_end_point_valid)
{
    int x0, y0, x1, y1;
    kgr_world_to_grid(g, fx, fy, &x0, &y0);
    kgr_world_to_grid(g, tx, ty, &x1, &y1);
    kgr_trace_line(g, x0, y0, x1, y1, NULL);
    if (is_end_point_valid) {
        if (kgr_valid(g, x1, y1)) {
            const size_t index = (size_t)y1 * g->width + x1;
            g->pass[index]++;
            g->hits[index]++;
        }
    }
}

/* RayTrace on grid coordinates, for the hand-written cases: the ends are already cells */
void kgr_ray_trace_cells(int width, int height, int x0, int y0, int x1, int y1, int is_end_point_valid,
                         uint32_t *pass, uint32_t *hits)
{
    kgr_grid g = {width, height, 0.0, 0.0, 1.0, pass, hits};
    kgr_trace_line(&g, x0, y0, x1, y1, NULL);
    if (is_end_point_valid && kgr_valid(&g, x1, y1)) {
        pass[(size_t)y1 * width + x1]++;
        hits[(size_t)y1 * width + x1]++;
    }
}

/* OccupancyGrid::AddScan (Karto.h:5852-5899), doUpdate = false.  With cells != NULL nothing is traced: beam i's
 * RayTrace arguments after WorldToGrid go to cells[5 * i ..] as x0, y0, x1, y1, isEndPointValid (-1: ignored). */
static void kgr_add_scan(const kgr_grid *g, const kgr_laser *L, const double *ranges, const double *pose, int *cells)
{
    const double rangeThreshold = L->range_threshold;
    const double maxRange = L->maximum_range;
    const double minRange = L->minimum_range;
    /* GetPointReadings(false): one unfiltered point per beam, so pointIndex is the beam index */
    for (int pointIndex = 0; pointIndex < L->n_readings; pointIndex++) {
        const double rangeReading = ranges[pointIndex];
        const int isEndPointValid = rangeReading < (rangeThreshold - KT_TOLERANCE);
        double px, py;
        if (rangeReading <= minRange || rangeReading >= maxRange || isnan(rangeReading)) {
            if (cells) cells[5 * pointIndex + 4] = -1;
            continue;
        }
        kgr_point(L, pose, pointIndex, rangeReading, &px, &py);
        if (rangeReading >= rangeThreshold) {
            const double ratio = rangeThreshold / rangeReading;
            const double dx = px - pose[0];
            const double dy = py - pose[1];
            px = pose[0] + ratio * dx;
            py = pose[1] + ratio * dy;
        }
        if (cells) {
            int *o = cells + 5 * pointIndex;
            kgr_world_to_grid(g, pose[0], pose[1], &o[0], &o[1]);
            kgr_world_to_grid(g, px, py, &o[2], &o[3]);
            o[4] = isEndPointValid;
        } else {
            kgr_ray_trace(g, pose[0], pose[1], px, py, isEndPointValid);
        }
    }
}

/* what AddScan hands to TraceLine, per beam of every scan: cells holds count * n_readings * 5 ints (zeroed by the
 * caller), see kgr_add_scan */
void kgr_ray_cells(const kgr_laser *L, int count, const double *ranges, const double *poses, double resolution,
                   const double *offset, int *cells)
{
    kgr_grid g = {0, 0, offset[0], offset[1], 1.0 / resolution, NULL, NULL};
    for (int s = 0; s < count; s++)
        kgr_add_scan(&g, L, ranges + (size_t)s * L->n_readings, poses + 3 * (size_t)s,
                     cells + 5 * (size_t)s * L->n_readings);
}

/* UpdateCell (Karto.h:5953-5968) after Clear(): 0 unknown, 100 occupied, 255 free; and the byte
 * karto_slam.cc:553-567 makes of it */
void kgr_update(size_t cells, const uint32_t *pass, const uint32_t *hits, uint32_t min_pass_through,
                double occupancy_threshold, uint8_t *state, int8_t *ros)
{
    for (size_t i = 0; i < cells; i++) {
        uint8_t v = 0;
        if (pass[i] > min_pass_through) {
            const double hitRatio = (double)hits[i] / (double)pass[i];
            if (hitRatio > occupancy_threshold)
                v = 100;
            else
                v = 255;
        }
        state[i] = v;
        ros[i] = v == 0 ? -1 : (v == 100 ? 100 : 0);
    }
}

/* CreateFromScans on a grid of the dimensions kgr_dimensions gave: the planes are dense width x height */
void kgr_create_from_scans(const kgr_laser *L, int count, const double *ranges, const double *poses,
                           double resolution, int width, int height, const double *offset,
                           uint32_t min_pass_through, double occupancy_threshold, uint32_t *pass, uint32_t *hits,
                           uint8_t *state, int8_t *ros)
{
    kgr_grid g = {width, height, offset[0], offset[1], 1.0 / resolution, pass, hits};
    const size_t cells = (size_t)width * height;
    memset(pass, 0, sizeof(uint32_t) * cells);
    memset(hits, 0, sizeof(uint32_t) * cells);
    for (int s = 0; s < count; s++)
        kgr_add_scan(&g, L, ranges + (size_t)s * L->n_readings, poses + 3 * (size_t)s, NULL);
    kgr_update(cells, pass, hits, min_pass_through, occupancy_threshold, state, ros);
}
