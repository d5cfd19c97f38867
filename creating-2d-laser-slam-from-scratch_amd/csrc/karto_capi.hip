// karto_capi.hip -- host runtime + extern "C" boundary (include/slam2d/karto.h) of the Karto
// correlative scan-matcher path.  Every compute step runs in karto_kernels.hip; without a usable HIP
// device kt_create fails with KT_ENODEV (no CPU fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_graph_mirror.h"  // DeviceEditEpoch
#include "karto_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError kt_err;
S2D_ASSERT_STATUS_CODES(KT);

enum { K_PREPARE, K_BEGIN, K_BUILD, K_COARSE, K_SELECT, K_FINE, K_CLEAR, K_REFRESH, K_NUM };
const char *const k_names[K_NUM] = {"kt_prepare_kernel", "kt_begin_kernel", "kt_build_kernel", "kt_coarse_kernel",
                                    "kt_select_kernel",  "kt_fine_kernel",  "kt_build_kernel<1> (clear)",
                                    "kt_refresh_kernel"};
static_assert(K_NUM <= KernelTimer::MAX_KERNELS, "the timer's accumulators");
static_assert(KT_REFRESH_MAX_ROWS == REFRESH_MAX_ROWS, "the plan header's row limit");
}  // namespace

struct kt_ctx {
    kt_laser laser{};
    kt_params params{};
    KtGeom g{};
    int max_matches = 0, max_scans = 0, max_base = 0;
    KtOptions opt{};         // the environment's knobs, read once at kt_create
    RefreshOptions refresh_opt{};
    DeviceEditEpoch refresh;  // kt_refresh_device's refused rows (its words and call numbers only)
    int num_cus = 1;
    int slots = 0;           // match slots resident at once (kt_run_batch chunk)
    size_t prepare_lds = 0;  // kt_prepare_kernel's dynamic LDS
    int *d_scratch = nullptr, *d_dirty = nullptr, *d_dirty_cnt = nullptr;
    double *d_ranges = nullptr, *d_poses = nullptr;
    int *d_npts = nullptr;
    double2 *d_pts = nullptr, *d_loc = nullptr;
    unsigned char *d_bad = nullptr;
    int2 *d_evt = nullptr;
    unsigned char *d_grids = nullptr, *d_kernel = nullptr;
    KtState *d_state = nullptr;
    double *d_resp = nullptr;
    unsigned long long *d_posmax = nullptr;
    int *d_tie_idx = nullptr;
    double4 *d_tie_val = nullptr;
    int *d_query = nullptr, *d_bbeg = nullptr, *d_bidx = nullptr;
    kt_result *d_res = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffers mem;
    KernelTimer timer;

    KtPool pool() const { return KtPool{d_ranges, d_poses, d_npts, d_pts, d_loc, d_bad, d_evt}; }
};

namespace {

#define KT_LAUNCH(which, ...) S2D_TIMED_LAUNCH(c->timer, kt_err.fail, KT_EHIP, s, which, __VA_ARGS__)

int kt_prepare(kt_ctx *c, int first, int count, hipStream_t s)
{
    KT_LAUNCH(K_PREPARE, kt_prepare_kernel, dim3(count), dim3(KT_THREADS), c->prepare_lds, s, c->g, c->pool(), first);
    return KT_OK;
}

// MatchScan steps 1-5 for a chunk: centre the grids (kt_begin_kernel) and AddScans
int kt_chunk_build(kt_ctx *c, const KtChunkPlan &plan, int count, const int *d_query, const int *d_bbeg,
                   const int *d_bidx, hipStream_t s)
{
    const KtGeom &g = c->g;
    KT_LAUNCH(K_BEGIN, kt_begin_kernel, dim3(count), dim3(KT_THREADS), 0, s, g, c->pool(), d_query, c->d_state,
              c->d_posmax);
    switch (plan.add) {
    case KT_ADD_NONE: break;
    case KT_ADD_BINNED:
        KT_LAUNCH(K_BUILD, kt_addscans_kernel, dim3(plan.add_grid), dim3(plan.add_block), 0, s, g, c->pool(), c->d_state,
                  d_bbeg, d_bidx, c->d_kernel, c->d_grids, c->d_scratch, (size_t)c->max_base * g.n, c->d_dirty,
                  c->d_dirty_cnt);
        break;
    case KT_ADD_PER_MATCH:
        KT_LAUNCH(K_BUILD, (kt_build_kernel<0, 8>), dim3(plan.add_grid), dim3(plan.add_block), 0, s, g, c->pool(),
                  c->d_state, d_bbeg, d_bidx, c->d_kernel, c->d_grids, count, c->max_base);
        break;
    case KT_ADD_PER_BASE:
        KT_LAUNCH(K_BUILD, (kt_build_kernel<0, 4>), dim3(plan.add_grid), dim3(plan.add_block), 0, s, g, c->pool(),
                  c->d_state, d_bbeg, d_bidx, c->d_kernel, c->d_grids, count, c->max_base);
        break;
    }
    return KT_OK;
}

int kt_chunk_coarse(kt_ctx *c, int count, int pass, int penalize, int shard, int nshards, hipStream_t s)
{
    const KtGeom &g = c->g;
    const KtCoarsePlan plan = kt_plan_coarse(c->opt, g, count, pass);
    if (plan.refused) return kt_err.fail(KT_EINVAL, plan.refused);
    KT_LAUNCH(K_COARSE, kt_coarse_kernel, dim3((unsigned)plan.blocks), dim3(KT_THREADS), (size_t)g.n * sizeof(int), s,
              g, c->pool(), c->d_state, c->d_grids, c->d_resp, c->d_posmax, count, pass, penalize, shard, nshards,
              plan.angle_group);
    return KT_OK;
}

// the fine match (MatchScan step 7) and the grids' footprint clear
int kt_chunk_finish(kt_ctx *c, const KtChunkPlan &plan, int count, const int *d_bbeg, const int *d_bidx, int penalize,
                    int refine, kt_result *d_res, hipStream_t s)
{
    const KtGeom &g = c->g;
    if (refine)
        KT_LAUNCH(K_FINE, kt_fine_kernel, dim3(plan.fine_grid), dim3(plan.fine_block), 0, s, g, c->pool(), c->d_state,
                  c->d_grids, penalize, d_res);
    if (plan.clear == KT_CLEAR_TILES)
        KT_LAUNCH(K_CLEAR, kt_clear_tiles_kernel, dim3(plan.clear_grid_x, plan.clear_grid_y), dim3(KT_THREADS), 0, s, g,
                  c->d_grids, c->d_dirty, c->d_dirty_cnt);
    else if (plan.clear == KT_CLEAR_FOOTPRINT)
        KT_LAUNCH(K_CLEAR, (kt_build_kernel<1, 4>), dim3(plan.clear_grid_x), dim3(KT_THREADS), 0, s, g, c->pool(),
                  c->d_state, d_bbeg, d_bidx, c->d_kernel, c->d_grids, count, c->max_base);
    return KT_OK;
}

// the one select launch (below kt_chunk_finish: the kernel instances are emitted in the order of their first use)
int kt_chunk_select(kt_ctx *c, const KtChunkPlan &plan, int count, int pass, int refine, kt_result *d_res, hipStream_t s)
{
    const auto kernel = plan.select_threads == 1024 ? kt_select_kernel<1024> : kt_select_kernel<KT_THREADS>;
    KT_LAUNCH(K_SELECT, kernel, dim3(count), dim3(plan.select_threads), 0, s, c->g, c->d_state, c->d_resp, c->d_posmax,
              c->d_tie_idx, c->d_tie_val, pass, refine, d_res);
    return KT_OK;
}

int kt_run_chunk(kt_ctx *c, int count, const int *d_query, const int *d_bbeg, const int *d_bidx, int penalize,
                 int refine, kt_result *d_res, hipStream_t s)
{
    const KtChunkPlan plan = kt_plan_chunk(c->opt, c->g, c->max_base, count);
    int rc = kt_chunk_build(c, plan, count, d_query, d_bbeg, d_bidx, s);
    if (rc != KT_OK) return rc;
    for (int pass = 0; pass < c->g.npass; ++pass) {
        if ((rc = kt_chunk_coarse(c, count, pass, penalize, 0, 1, s)) != KT_OK) return rc;
        if ((rc = kt_chunk_select(c, plan, count, pass, refine, d_res, s)) != KT_OK) return rc;
    }
    return kt_chunk_finish(c, plan, count, d_bbeg, d_bidx, penalize, refine, d_res, s);
}

// The batch runs in chunks of `slots` matches (kt_slots).
int kt_run_batch(kt_ctx *c, int count, const int *d_query, const int *d_bbeg, const int *d_bidx, int penalize,
                 int refine, kt_result *d_res, hipStream_t s)
{
    for (int c0 = 0; c0 < count; c0 += c->slots) {
        const int cnt = std::min(c->slots, count - c0);
        const int rc = kt_run_chunk(c, cnt, d_query + c0, d_bbeg + c0, d_bidx, penalize, refine, d_res + c0, s);
        if (rc != KT_OK) return rc;
    }
    return KT_OK;
}

}  // namespace

extern "C" {

const char *kt_version(void) { return "slam2d-mi355x karto 0.1 (gfx950)"; }
const char *kt_last_error(void) { return kt_err.c_str(); }

void kt_default_params(kt_params *p)
{
    if (!p) return;
    // Mapper::InitializeParameters (lesson6/lib/open_karto/src/Mapper.cpp:1569-1660)
    p->search_size = 0.3;
    p->resolution = 0.01;
    p->smear_deviation = 0.03;
    p->distance_variance_penalty = 0.3 * 0.3;
    const double d20 = 20 * 0.01745329251994329577;
    p->angle_variance_penalty = d20 * d20;
    p->fine_search_angle_offset = 0.2 * 0.01745329251994329577;
    p->coarse_search_angle_offset = d20;
    p->coarse_angle_resolution = 2 * 0.01745329251994329577;
    p->minimum_angle_penalty = 0.9;
    p->minimum_distance_penalty = 0.5;
    p->use_response_expansion = 0;
    p->pad_ = 0;
}

void kt_default_loop_params(kt_params *p)
{
    if (!p) return;
    kt_default_params(p);
    p->search_size = 8.0;  // LoopSearchSpaceDimension
    p->resolution = 0.05;  // LoopSearchSpaceResolution
    p->smear_deviation = 0.03;
}

int kt_destroy(kt_ctx *c)
{
    if (!c) return KT_OK;
    if (c->stream) hipStreamSynchronize(c->stream);
    c->mem.free_all();
    c->timer.destroy();
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return KT_OK;
}

int kt_create(kt_ctx **out, const kt_laser *laser, const kt_params *params, int max_matches, int max_scans,
              int max_base_per_match)
{
    if (!out) return kt_err.fail(KT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!laser) return kt_err.fail(KT_EINVAL, "laser is NULL");
    if (max_matches < 1 || max_matches > 65535 || max_scans < 1 || max_base_per_match < 0)
        return kt_err.fail(KT_EINVAL, "need 1 <= max_matches <= 65535, max_scans >= 1, max_base_per_match >= 0");
    kt_params p;
    if (params) p = *params;
    else kt_default_params(&p);
    KtOptions opt;
    const char *refused = kt_parse_options(opt, [](const char *knob) -> const char * { return getenv(knob); });
    if (refused) return kt_err.fail(KT_EINVAL, refused);
    RefreshOptions refresh_opt;
    if ((refused = refresh_parse_options(refresh_opt, [](const char *knob) -> const char * { return getenv(knob); })))
        return kt_err.fail(KT_EINVAL, refused);
    KtGeom g;
    std::vector<unsigned char> kernel;
    const int rc = kt_geometry(*laser, p, opt, g, kernel, refused);
    if (rc != KT_OK) return kt_err.fail(rc, refused);
    if (!device_present()) return kt_err.fail(KT_ENODEV, "no HIP device");
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return kt_err.fail(KT_ENODEV, "no HIP device");
    kt_ctx *c = new kt_ctx;
    c->refresh_opt = refresh_opt;
    c->num_cus = std::max(1, prop.multiProcessorCount);
    c->laser = *laser;
    c->params = p;
    c->g = g;
    c->max_matches = max_matches;
    c->max_scans = max_scans;
    c->max_base = max_base_per_match;
    c->opt = opt;
    c->slots = kt_slots(opt, max_matches);
    const KtChunkPlan plan = kt_plan_chunk(opt, g, max_base_per_match, 1);
    c->prepare_lds = plan.prepare_lds;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault)) != hipSuccess) {
        delete c;
        return kt_err.fail(KT_EHIP, "hipStreamCreate", e);
    }
    const size_t S = (size_t)max_scans, n = (size_t)g.n, M = (size_t)c->slots;
    const size_t mp = (size_t)g.max_poses, npos = (size_t)g.nxy * g.nxy;
    DeviceBuffers &m = c->mem;
    m.alloc(c->d_ranges, sizeof(double) * S * n);
    m.alloc(c->d_poses, sizeof(double) * S * 3);
    m.alloc(c->d_npts, sizeof(int) * S);
    m.alloc(c->d_pts, sizeof(double2) * S * n);
    m.alloc(c->d_loc, sizeof(double2) * S * n);
    m.alloc(c->d_bad, S * n);
    m.alloc(c->d_evt, sizeof(int2) * S * n);
    m.alloc(c->d_grids, g.grid_stride * M);
    m.alloc(c->d_kernel, kernel.size());
    m.alloc(c->d_state, sizeof(KtState) * M);
    m.alloc(c->d_resp, sizeof(double) * mp * M);
    m.alloc(c->d_posmax, sizeof(unsigned long long) * npos * M);
    m.alloc(c->d_tie_idx, sizeof(int) * mp * M);
    m.alloc(c->d_tie_val, sizeof(double4) * std::max(mp, npos) * M);
    m.alloc(c->d_query, sizeof(int));
    m.alloc(c->d_bbeg, sizeof(int) * 2);
    m.alloc(c->d_bidx, sizeof(int) * std::max<size_t>(1, (size_t)max_base_per_match));
    m.alloc(c->d_res, sizeof(kt_result));
    m.alloc(c->refresh.d_info, sizeof(unsigned long long) * 2);
    if (kt_binned_eligible(opt, g, max_base_per_match)) {
        m.alloc(c->d_scratch, sizeof(int) * M * std::max<size_t>(1, (size_t)max_base_per_match) * n);
        m.alloc(c->d_dirty, sizeof(int) * M * (size_t)g.ntiles);
        m.alloc(c->d_dirty_cnt, sizeof(int) * M);
    }
    if ((e = m.error) != hipSuccess || (opt.poison && (e = m.fill(0xA5, c->stream)) != hipSuccess)) {
        kt_destroy(c);
        return kt_err.fail(KT_ENOMEM, "hipMalloc", e);
    }
    if (plan.prepare_attr &&
        (e = hipFuncSetAttribute((const void *)kt_prepare_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)plan.prepare_lds)) != hipSuccess) {
        kt_destroy(c);
        return kt_err.fail(KT_EHIP, "hipFuncSetAttribute(kt_prepare_kernel)", e);
    }
    // kt_refresh_kernel keeps the rows' prefix sum (at most 16 KB) behind the same arrays
    if (kt_refresh_lds(plan.prepare_lds, REFRESH_MAX_ROWS) + 64 > 65536 &&
        (e = hipFuncSetAttribute((const void *)kt_refresh_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kt_refresh_lds(plan.prepare_lds, REFRESH_MAX_ROWS))) != hipSuccess) {
        kt_destroy(c);
        return kt_err.fail(KT_EHIP, "hipFuncSetAttribute(kt_refresh_kernel)", e);
    }
    if ((e = hipMemsetAsync(c->d_grids, 0, g.grid_stride * M, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->d_npts, 0, sizeof(int) * S, c->stream)) != hipSuccess ||
        (e = c->refresh.reset_async(c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->d_kernel, kernel.data(), kernel.size(), hipMemcpyHostToDevice, c->stream)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        kt_destroy(c);
        return kt_err.fail(KT_EHIP, "initialising the context", e);
    }
    *out = c;
    return KT_OK;
}

int kt_get_grid_info(kt_ctx *c, int *out)
{
    if (!c || !out) return kt_err.fail(KT_EINVAL, "NULL argument");
    kt_grid_info_words(c->g, out);
    return KT_OK;
}

int kt_set_scans_device(kt_ctx *c, int first, int count, const double *d_ranges, const double *d_poses,
                        void *hip_stream)
{
    if (!c || !d_ranges || !d_poses) return kt_err.fail(KT_EINVAL, "NULL argument");
    if (first < 0 || count < 0 || first + count > c->max_scans) return kt_err.fail(KT_EINVAL, "scan slots out of range");
    if (count == 0) return KT_OK;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const size_t n = (size_t)c->g.n;
    if (d_ranges != c->d_ranges + (size_t)first * n)
        S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_ranges + (size_t)first * n, d_ranges, sizeof(double) * n * count,
                            hipMemcpyDeviceToDevice, s));
    if (d_poses != c->d_poses + (size_t)first * 3)
        S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_poses + (size_t)first * 3, d_poses, sizeof(double) * 3 * count,
                            hipMemcpyDeviceToDevice, s));
    return kt_prepare(c, first, count, s);
}

int kt_set_scans(kt_ctx *c, int first, int count, const double *ranges, const double *poses)
{
    if (!c || !ranges || !poses) return kt_err.fail(KT_EINVAL, "NULL argument");
    if (first < 0 || count < 0 || first + count > c->max_scans) return kt_err.fail(KT_EINVAL, "scan slots out of range");
    if (count == 0) return KT_OK;
    const size_t n = (size_t)c->g.n;
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_ranges + (size_t)first * n, ranges, sizeof(double) * n * count, hipMemcpyHostToDevice,
                        c->stream));
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_poses + (size_t)first * 3, poses, sizeof(double) * 3 * count, hipMemcpyHostToDevice,
                        c->stream));
    int rc = kt_prepare(c, first, count, c->stream);
    if (rc != KT_OK) return rc;
    S2D_CHK(kt_err, KT_EHIP, hipStreamSynchronize(c->stream));
    return KT_OK;
}

int kt_pool_device(kt_ctx *c, const double **d_ranges, const double **d_poses, int *max_scans)
{
    if (!c) return kt_err.fail(KT_EINVAL, "ctx is NULL");
    if (d_ranges) *d_ranges = c->d_ranges;
    if (d_poses) *d_poses = c->d_poses;
    if (max_scans) *max_scans = c->max_scans;
    return KT_OK;
}

int kt_refresh_device(kt_ctx *c, int n_rows, const void *d_rows, const double *d_pool_ranges, const double *d_pool_poses,
                      int pool_scans, void *hip_stream)
{
    if (!c) return kt_err.fail(KT_EINVAL, "ctx is NULL");
    if (n_rows < 0 || pool_scans < 0) return kt_err.fail(KT_EINVAL, "negative count");
    if (n_rows > KT_REFRESH_MAX_ROWS) return kt_err.fail(KT_ERANGE, "more than KT_REFRESH_MAX_ROWS (4096) rows");
    if (n_rows == 0) return KT_OK;
    if (!d_rows || !d_pool_ranges || !d_pool_poses) return kt_err.fail(KT_EINVAL, "NULL argument");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int limit = std::min(c->max_scans, pool_scans);
    if (limit == 0) return KT_OK;  // no row can name a slot: nothing to launch (and nothing to refuse into)
    c->refresh.bump();
    // the host knows no row, so the launch is sized by what the rows can name at most
    const int grid = refresh_grid(c->refresh_opt, c->num_cus, refresh_bound(n_rows, limit));
    const KtRefresh r{(const int2 *)d_rows, d_pool_ranges, d_pool_poses, c->d_ranges, c->d_poses, c->refresh.d_info, n_rows,
                      limit, (d_pool_ranges != c->d_ranges ? 1 : 0) | (d_pool_poses != c->d_poses ? 2 : 0), c->refresh.seq,
                      (int)kt_refresh_prefix_offset(c->prepare_lds)};
    KT_LAUNCH(K_REFRESH, kt_refresh_kernel, dim3((unsigned)grid), dim3(KT_THREADS), kt_refresh_lds(c->prepare_lds, n_rows), s,
              c->g, c->pool(), r);
    return KT_OK;
}

int kt_get_refresh_info(kt_ctx *c, int *n_refused, int *first_status)
{
    if (!c) return kt_err.fail(KT_EINVAL, "ctx is NULL");
    S2D_CHK(kt_err, KT_EHIP, hipDeviceSynchronize());
    return c->refresh.read_and_reset(kt_err, n_refused, first_status);
}

int kt_get_prepared(kt_ctx *c, int slot, int *npts, double *pts, double *loc, unsigned char *bad, int *evt)
{
    if (!c) return kt_err.fail(KT_EINVAL, "ctx is NULL");
    if (slot < 0 || slot >= c->max_scans) return kt_err.fail(KT_EINVAL, "scan slot out of range");
    S2D_CHK(kt_err, KT_EHIP, hipDeviceSynchronize());
    int k = 0;
    S2D_CHK(kt_err, KT_EHIP, hipMemcpy(&k, c->d_npts + slot, sizeof(int), hipMemcpyDeviceToHost));
    if (k < 0 || k > c->g.n) return kt_err.fail(KT_EHIP, "the slot's point count is out of range");
    if (npts) *npts = k;
    const size_t at = (size_t)slot * c->g.n;
    if (k > 0 && pts) S2D_CHK(kt_err, KT_EHIP, hipMemcpy(pts, c->d_pts + at, sizeof(double2) * k, hipMemcpyDeviceToHost));
    if (k > 0 && loc) S2D_CHK(kt_err, KT_EHIP, hipMemcpy(loc, c->d_loc + at, sizeof(double2) * k, hipMemcpyDeviceToHost));
    if (k > 0 && bad) S2D_CHK(kt_err, KT_EHIP, hipMemcpy(bad, c->d_bad + at, (size_t)k, hipMemcpyDeviceToHost));
    if (k > 0 && evt) S2D_CHK(kt_err, KT_EHIP, hipMemcpy(evt, c->d_evt + at, sizeof(int2) * k, hipMemcpyDeviceToHost));
    return KT_OK;
}

int kt_match_batch_device(kt_ctx *c, int count, const int *d_query, const int *d_bbeg, const int *d_bidx,
                          int do_penalize, int do_refine, kt_result *d_res, void *hip_stream)
{
    if (!c || !d_query || !d_bbeg || !d_res) return kt_err.fail(KT_EINVAL, "NULL argument");
    if (count < 0 || count > c->max_matches) return kt_err.fail(KT_EINVAL, "count exceeds max_matches");
    if (count == 0) return KT_OK;
    if (c->max_base > 0 && !d_bidx) return kt_err.fail(KT_EINVAL, "d_base_index is NULL");
    return kt_run_batch(c, count, d_query, d_bbeg, d_bidx, do_penalize ? 1 : 0, do_refine ? 1 : 0, d_res,
                        hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int kt_match_scan(kt_ctx *c, const double *q_ranges, const double q_pose[3], int n_base, const double *b_ranges,
                  const double *b_poses, int do_penalize, int do_refine, kt_result *result)
{
    if (!c || !q_ranges || !q_pose || !result || (n_base > 0 && (!b_ranges || !b_poses)))
        return kt_err.fail(KT_EINVAL, "NULL argument");
    if (n_base < 0 || n_base > c->max_base || n_base + 1 > c->max_scans)
        return kt_err.fail(KT_EINVAL, "n_base exceeds max_base_per_match or the scan pool");
    const size_t n = (size_t)c->g.n;
    hipStream_t s = c->stream;
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_ranges, q_ranges, sizeof(double) * n, hipMemcpyHostToDevice, s));
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_poses, q_pose, sizeof(double) * 3, hipMemcpyHostToDevice, s));
    if (n_base > 0) {
        S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_ranges + n, b_ranges, sizeof(double) * n * n_base, hipMemcpyHostToDevice, s));
        S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_poses + 3, b_poses, sizeof(double) * 3 * n_base, hipMemcpyHostToDevice, s));
    }
    int rc = kt_prepare(c, 0, 1 + n_base, s);
    if (rc != KT_OK) return rc;
    std::vector<int> idx((size_t)std::max(1, n_base));
    for (int i = 0; i < n_base; ++i) idx[i] = 1 + i;
    const int q0 = 0, beg[2] = {0, n_base};
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_query, &q0, sizeof(int), hipMemcpyHostToDevice, s));
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_bbeg, beg, sizeof(int) * 2, hipMemcpyHostToDevice, s));
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(c->d_bidx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice, s));
    rc = kt_run_batch(c, 1, c->d_query, c->d_bbeg, c->d_bidx, do_penalize ? 1 : 0, do_refine ? 1 : 0, c->d_res, s);
    if (rc != KT_OK) return rc;
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(result, c->d_res, sizeof(kt_result), hipMemcpyDeviceToHost, s));
    S2D_CHK(kt_err, KT_EHIP, hipStreamSynchronize(s));
    return KT_OK;
}

size_t kt_window_exchange_words(kt_ctx *c)
{
    if (!c) return 0;
    const size_t nxy2 = (size_t)c->g.nxy * c->g.nxy;
    return 2 + nxy2 + nxy2 * (size_t)c->g.nang[0];
}

int kt_match_sharded_begin_device(kt_ctx *c, int count, const int *d_query, const int *d_bbeg, const int *d_bidx,
                                  int do_penalize, int shard, int nshards, int64_t *d_exchange, void *hip_stream)
{
    if (!c || !d_query || !d_bbeg || !d_exchange) return kt_err.fail(KT_EINVAL, "NULL argument");
    if (count < 1 || count > c->slots) return kt_err.fail(KT_EINVAL, "sharded batch must hold 1 .. slots matches");
    if (nshards < 1 || shard < 0 || shard >= nshards) return kt_err.fail(KT_EINVAL, "need 0 <= shard < nshards");
    if (c->g.npass != 1) return kt_err.fail(KT_EINVAL, "a sharded window does not support response expansion");
    if (c->max_base > 0 && !d_bidx) return kt_err.fail(KT_EINVAL, "d_base_index is NULL");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    int rc = kt_chunk_build(c, kt_plan_chunk(c->opt, c->g, c->max_base, count), count, d_query, d_bbeg, d_bidx, s);
    if (rc != KT_OK) return rc;
    if ((rc = kt_chunk_coarse(c, count, 0, do_penalize ? 1 : 0, shard, nshards, s)) != KT_OK) return rc;
    hipLaunchKernelGGL(kt_exchange_kernel, dim3(count), dim3(KT_THREADS), 0, s, c->g, c->d_state, c->d_resp,
                       c->d_posmax, (long long *)d_exchange, 0);
    S2D_CHK(kt_err, KT_EHIP, hipGetLastError());
    return KT_OK;
}

int kt_match_sharded_end_device(kt_ctx *c, int count, const int *d_bbeg, const int *d_bidx, int do_penalize,
                                int do_refine, const int64_t *d_exchange, kt_result *d_res, void *hip_stream)
{
    if (!c || !d_bbeg || !d_exchange || !d_res) return kt_err.fail(KT_EINVAL, "NULL argument");
    if (count < 1 || count > c->slots) return kt_err.fail(KT_EINVAL, "sharded batch must hold 1 .. slots matches");
    if (c->max_base > 0 && !d_bidx) return kt_err.fail(KT_EINVAL, "d_base_index is NULL");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    hipLaunchKernelGGL(kt_exchange_kernel, dim3(count), dim3(KT_THREADS), 0, s, c->g, c->d_state, c->d_resp,
                       c->d_posmax, (long long *)d_exchange, 1);
    S2D_CHK(kt_err, KT_EHIP, hipGetLastError());
    // the same plan as the begin call's: it depends on the context and `count` alone
    const KtChunkPlan plan = kt_plan_chunk(c->opt, c->g, c->max_base, count);
    const int rc = kt_chunk_select(c, plan, count, 0, do_refine ? 1 : 0, d_res, s);
    if (rc != KT_OK) return rc;
    return kt_chunk_finish(c, plan, count, d_bbeg, d_bidx, do_penalize ? 1 : 0, do_refine ? 1 : 0, d_res, s);
}

int kt_copy_grid_device(kt_ctx *c, int slot, unsigned char *d_out, void *hip_stream)
{
    if (!c || !d_out) return kt_err.fail(KT_EINVAL, "NULL argument");
    if (slot < 0 || slot >= c->slots) return kt_err.fail(KT_EINVAL, "slot out of range");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyAsync(d_out, c->d_grids + (size_t)slot * c->g.grid_stride, (size_t)c->g.data_size,
                        hipMemcpyDeviceToDevice, s));
    return KT_OK;
}

int kt_set_timing(kt_ctx *c, int enable)
{
    if (!c) return kt_err.fail(KT_EINVAL, "ctx is NULL");
    return set_timing(c->timer, enable);
}

#if defined(KT_DIAG_STAMPS)
// diagnostic builds only: per-workgroup s_memtime stamps of kt_addscans_kernel (8 per block)
int kt_diag_stamps(unsigned long long *out, int blocks)
{
    S2D_CHK(kt_err, KT_EHIP, hipDeviceSynchronize());
    S2D_CHK(kt_err, KT_EHIP, hipMemcpyFromSymbol(out, HIP_SYMBOL(kt_diag), sizeof(unsigned long long) * 8 * blocks));
    return KT_OK;
}
#endif

int kt_num_kernels(void) { return K_NUM; }
const char *kt_kernel_name(int i) { return kernel_name(k_names, K_NUM, i); }

int kt_get_kernel_times(kt_ctx *c, double *ms_out, int64_t *launches_out, int reset)
{
    if (!c) return kt_err.fail(KT_EINVAL, "ctx is NULL");
    return get_kernel_times(c->timer, kt_err, ms_out, launches_out, reset, K_NUM);
}

}  // extern "C"
