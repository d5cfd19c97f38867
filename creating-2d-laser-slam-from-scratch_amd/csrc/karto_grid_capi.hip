// karto_grid_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto_grid.h) of the Karto
// occupancy-grid rebuild.  Every compute step runs in karto_grid_kernels.hip; without a usable HIP device
// kg_create fails with KG_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_grid_kernels.hip"
#include "karto_internal.h"  // kg_parse_options, kg_split_rule

using namespace s2d;

namespace {
thread_local StageError kg_err;
S2D_ASSERT_STATUS_CODES(KG);

double g_round(double v) { return v >= 0.0 ? std::floor(v + 0.5) : std::ceil(v - 0.5); }  // math::Round

constexpr size_t KG_MAX_CELLS = (size_t)1 << 28;
constexpr double KG_MAX_REACH = 1048576.0;  // range_threshold / resolution, cells

enum { G_BBOX, G_REDUCE, G_RAYS, G_TRACE, G_UPDATE, G_NUM };
const char *const g_names[G_NUM] = {"kg_bbox_kernel", "kg_bbox_reduce_kernel", "kg_rays_kernel", "kg_trace_kernel",
                                    "kg_update_kernel"};
static_assert(G_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
}  // namespace

struct kg_ctx {
    KgGeom g{};
    int max_scans = 0, num_cus = 0;
    int force_split = 0;  // SLAM2D_KG_SPLIT: workgroups per tile, overriding the rule (tests, A/B)
    size_t max_cells = 0;
    int width = 0, height = 0;  // the last build's map
    double *d_ranges = nullptr, *d_poses = nullptr;  // staging of kg_build
    double *d_boxes = nullptr, *d_box = nullptr, *h_box = nullptr;
    int2 *d_rays = nullptr;
    KgScan *d_scans = nullptr;
    uint32_t *d_pass = nullptr, *d_hits = nullptr;
    uint8_t *d_state = nullptr;
    int8_t *d_ros = nullptr;
    hipStream_t stream = nullptr, last = nullptr;
    std::mutex mu;
    DeviceBuffers mem;
    KernelTimer timer;
};

namespace {

#define KG_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, kg_err.fail, KG_EHIP, s, which, __VA_ARGS__)

int kg_run(kg_ctx *c, int count, const double *d_ranges, const double *d_poses, kg_info *info, hipStream_t s)
{
    KgGeom &g = c->g;
    c->width = c->height = 0;
    c->last = s;
    kg_info out{};
    KG_LAUNCH(G_BBOX, kg_bbox_kernel, dim3(count), dim3(KG_THREADS), 0, s, g, d_ranges, d_poses, c->d_boxes);
    KG_LAUNCH(G_REDUCE, kg_bbox_reduce_kernel, dim3(1), dim3(KG_THREADS), 0, s, count, c->d_boxes, c->d_box);
    S2D_CHK(kg_err, KG_EHIP, hipMemcpyAsync(c->h_box, c->d_box, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
    S2D_CHK(kg_err, KG_EHIP, hipStreamSynchronize(s));  // the call's one synchronisation: the launches below are sized by the box
    // ComputeDimensions (Karto.h:5816-5821)
    const double w = g_round((c->h_box[2] - c->h_box[0]) * g.scale);
    const double h = g_round((c->h_box[3] - c->h_box[1]) * g.scale);
    out.offset_x = c->h_box[0];
    out.offset_y = c->h_box[1];
    const bool fits = w >= 0 && h >= 0 && w <= 2147483647.0 && h <= 2147483647.0;  // false for NaN too
    out.width = fits ? (int)w : INT_MAX;
    out.height = fits ? (int)h : INT_MAX;
    if (!fits || (double)out.width * (double)out.height > (double)c->max_cells) {
        out.status = KG_ERANGE;
        if (info) *info = out;
        return kg_err.fail(KG_ERANGE, "the map has more cells than max_cells (kg_info holds its dimensions)");
    }
    out.status = KG_OK;
    if (info) *info = out;
    c->width = out.width;
    c->height = out.height;
    if (out.width == 0 || out.height == 0) return KG_OK;

    g.width = out.width;
    g.height = out.height;
    g.off_x = out.offset_x;
    g.off_y = out.offset_y;
    g.tiles_x = (g.width + KG_TILE - 1) / KG_TILE;
    g.tiles_y = (g.height + KG_TILE - 1) / KG_TILE;
    const int ntiles = g.tiles_x * g.tiles_y;
    g.split = kg_split_rule(c->force_split, c->num_cus, ntiles, count);
    const size_t cells = (size_t)g.width * g.height;

    KG_LAUNCH(G_RAYS, kg_rays_kernel, dim3(count), dim3(KG_THREADS), 0, s, g, d_ranges, d_poses, c->d_rays,
              c->d_scans);
    if (g.split > 1) {
        S2D_CHK(kg_err, KG_EHIP, hipMemsetAsync(c->d_pass, 0, sizeof(uint32_t) * cells, s));
        S2D_CHK(kg_err, KG_EHIP, hipMemsetAsync(c->d_hits, 0, sizeof(uint32_t) * cells, s));
    }
    KG_LAUNCH(G_TRACE, kg_trace_kernel, dim3((unsigned)(ntiles * g.split)), dim3(KG_THREADS), 0, s, g, count,
              c->d_rays, c->d_scans, c->d_pass, c->d_hits);
    const size_t groups = (cells + 15) / 16;
    KG_LAUNCH(G_UPDATE, kg_update_kernel, dim3((unsigned)((groups + KG_THREADS - 1) / KG_THREADS)), dim3(KG_THREADS),
              0, s, g, cells, c->d_pass, c->d_hits, c->d_state, c->d_ros);
    return KG_OK;
}

}  // namespace

extern "C" {

const char *kg_last_error(void) { return kg_err.c_str(); }

void kg_default_params(kg_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->resolution = 0.05;
    p->maximum_range = 0.0;  // the caller's scan->range_max
    p->occupancy_threshold = 0.1;
    p->min_pass_through = 2;
}

int kg_create(kg_ctx **out, const kt_laser *L, const kg_params *p, int max_scans, size_t max_cells)
{
    if (!out) return kg_err.fail(KG_EINVAL, "out is NULL");
    *out = nullptr;
    if (!L || !p) return kg_err.fail(KG_EINVAL, "NULL argument");
    if (!(p->resolution > 0) || !std::isfinite(p->resolution))
        return kg_err.fail(KG_EINVAL, "resolution must be > 0 (the reference throws on 0)");
    if (!(p->maximum_range > 0)) return kg_err.fail(KG_EINVAL, "maximum_range must be set (> 0): the scan's range_max");
    if (L->n_readings < 1 || L->n_readings > 4096) return kg_err.fail(KG_EINVAL, "n_readings must be in [1, 4096]");
    if (!(L->range_threshold > 0) || !(L->range_threshold / p->resolution <= KG_MAX_REACH))
        return kg_err.fail(KG_EINVAL, "range_threshold must be > 0 and at most 2^20 cells long");
    if (max_scans < 1 || max_cells < 1 || max_cells > KG_MAX_CELLS)
        return kg_err.fail(KG_EINVAL, "need max_scans >= 1 and 1 <= max_cells <= 2^28");
    int force_split = 0;
    if (const char *refused = kg_parse_options(force_split, [](const char *knob) -> const char * { return getenv(knob); }))
        return kg_err.fail(KG_EINVAL, refused);
    if (!device_present()) return kg_err.fail(KG_ENODEV, "no HIP device");
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return kg_err.fail(KG_ENODEV, "no HIP device");
    kg_ctx *c = new kg_ctx;
    c->max_scans = max_scans;
    c->max_cells = max_cells;
    c->num_cus = std::max(1, prop.multiProcessorCount);
    c->force_split = force_split;
    KgGeom &g = c->g;
    g.min_angle = L->minimum_angle;
    g.ang_res = L->angular_resolution;
    g.min_range = L->minimum_range;
    g.range_thr = L->range_threshold;
    g.max_range = p->maximum_range;
    g.scale = 1.0 / p->resolution;
    g.occ_thr = p->occupancy_threshold;
    g.min_pass = p->min_pass_through;
    g.n = L->n_readings;
    g.split = 1;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault)) != hipSuccess) {
        delete c;
        return kg_err.fail(KG_EHIP, "hipStreamCreate", e);
    }
    const size_t S = (size_t)max_scans, n = (size_t)g.n, cells = (max_cells + 15) & ~(size_t)15;
    DeviceBuffers &m = c->mem;
    m.alloc(c->d_ranges, sizeof(double) * S * n);
    m.alloc(c->d_poses, sizeof(double) * S * 3);
    m.alloc(c->d_boxes, sizeof(double) * S * 4);
    m.alloc(c->d_box, sizeof(double) * 4);
    m.alloc(c->d_rays, sizeof(int2) * S * n);
    m.alloc(c->d_scans, sizeof(KgScan) * S);
    m.alloc(c->d_pass, sizeof(uint32_t) * cells);
    m.alloc(c->d_hits, sizeof(uint32_t) * cells);
    m.alloc(c->d_state, cells);
    m.alloc(c->d_ros, cells);
    if ((e = m.error) != hipSuccess || (e = hipHostMalloc(&c->h_box, sizeof(double) * 4)) != hipSuccess) {
        kg_destroy(c);
        return kg_err.fail(KG_ENOMEM, "hipMalloc", e);
    }
    *out = c;
    return KG_OK;
}

int kg_destroy(kg_ctx *c)
{
    if (!c) return KG_OK;
    if (c->last) hipStreamSynchronize(c->last);
    if (c->stream) hipStreamSynchronize(c->stream);
    c->mem.free_all();
    if (c->h_box) hipHostFree(c->h_box);
    c->timer.destroy();
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return KG_OK;
}

int kg_build_device(kg_ctx *c, int count, const double *d_ranges, const double *d_poses, kg_info *info,
                    void *hip_stream)
{
    if (info) {
        memset(info, 0, sizeof(*info));
        info->status = KG_EINVAL;
    }
    if (!c) return kg_err.fail(KG_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    if (count == 0) return kg_err.fail(KG_EINVAL, "no scans: no grid (CreateFromScans returns NULL)");
    if (count < 0 || count > c->max_scans) return kg_err.fail(KG_EINVAL, "count exceeds max_scans");
    if (!d_ranges || !d_poses) return kg_err.fail(KG_EINVAL, "NULL argument");
    return kg_run(c, count, d_ranges, d_poses, info, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int kg_build(kg_ctx *c, int count, const double *ranges, const double *poses, kg_info *info)
{
    if (info) {
        memset(info, 0, sizeof(*info));
        info->status = KG_EINVAL;
    }
    if (!c) return kg_err.fail(KG_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    if (count == 0) return kg_err.fail(KG_EINVAL, "no scans: no grid (CreateFromScans returns NULL)");
    if (count < 0 || count > c->max_scans) return kg_err.fail(KG_EINVAL, "count exceeds max_scans");
    if (!ranges || !poses) return kg_err.fail(KG_EINVAL, "NULL argument");
    hipStream_t s = c->stream;
    S2D_CHK(kg_err, KG_EHIP, hipMemcpyAsync(c->d_ranges, ranges, sizeof(double) * (size_t)c->g.n * count, hipMemcpyHostToDevice, s));
    S2D_CHK(kg_err, KG_EHIP, hipMemcpyAsync(c->d_poses, poses, sizeof(double) * 3 * count, hipMemcpyHostToDevice, s));
    int rc = kg_run(c, count, c->d_ranges, c->d_poses, info, s);
    if (rc != KG_OK) return rc;
    S2D_CHK(kg_err, KG_EHIP, hipStreamSynchronize(s));
    return KG_OK;
}

int kg_get_map(kg_ctx *c, uint8_t *state, int8_t *ros, uint32_t *pass, uint32_t *hits)
{
    if (!c) return kg_err.fail(KG_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->last) S2D_CHK(kg_err, KG_EHIP, hipStreamSynchronize(c->last));
    const size_t cells = (size_t)c->width * c->height;
    if (cells == 0) return KG_OK;
    if (state) S2D_CHK(kg_err, KG_EHIP, hipMemcpy(state, c->d_state, cells, hipMemcpyDeviceToHost));
    if (ros) S2D_CHK(kg_err, KG_EHIP, hipMemcpy(ros, c->d_ros, cells, hipMemcpyDeviceToHost));
    if (pass) S2D_CHK(kg_err, KG_EHIP, hipMemcpy(pass, c->d_pass, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
    if (hits) S2D_CHK(kg_err, KG_EHIP, hipMemcpy(hits, c->d_hits, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
    return KG_OK;
}

int kg_device_planes(kg_ctx *c, const uint8_t **d_state, const int8_t **d_ros, const uint32_t **d_pass,
                     const uint32_t **d_hits)
{
    if (!c) return kg_err.fail(KG_EINVAL, "ctx is NULL");
    if (d_state) *d_state = c->d_state;
    if (d_ros) *d_ros = c->d_ros;
    if (d_pass) *d_pass = c->d_pass;
    if (d_hits) *d_hits = c->d_hits;
    return KG_OK;
}

int kg_set_timing(kg_ctx *c, int enable)
{
    if (!c) return kg_err.fail(KG_EINVAL, "ctx is NULL");
    return set_timing(c->timer, enable);
}

int kg_num_kernels(void) { return G_NUM; }
const char *kg_kernel_name(int i) { return kernel_name(g_names, G_NUM, i); }

int kg_get_kernel_times(kg_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return kg_err.fail(KG_EINVAL, "ctx is NULL");
    return get_kernel_times(c->timer, kg_err, ms_out, launches_out, reset, G_NUM);
}

}  // extern "C"
