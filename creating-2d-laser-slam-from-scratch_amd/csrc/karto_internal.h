// karto_internal.h -- what the Karto kernels and their host runtimes share (KtGeom, the kernel sizes), and the hosts'
// policy: the options read from the environment at kt_create / kg_create (the knob table is in DESIGN.md, "Karto host
// knobs"), the matcher's geometry and what a chunk of matches launches.  No HIP type, no context, no global: it
// compiles as plain C++17 too (tests/cpp/karto_launch_check.cpp, tests/test_karto_launch_cpu.py).
#pragma once
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/slam2d/karto.h"
#include "knob_int.h"  // parse_knob_int

namespace s2d {

constexpr int KT_THREADS = 256;
constexpr int KT_MAX_READINGS = 4096;
constexpr int KT_FINE_MAX_ANG = 64;
constexpr int KT_MAX_NXY = 1024;  // coarse positions per axis
constexpr int KT_OCC = 100;
// kt_addscans_kernel (karto_kernels.hip explains them)
constexpr int KT_AS_WAVES = 8;
constexpr int KT_AS_MAX_TILES = 2048;  // tiles per grid (e.g. 2896 x 2896 cells)
constexpr int KT_AS_MAX_BASE = 1024;
constexpr int KT_FINE_THREADS = KT_THREADS;  // 1024 threads (4 waves per SIMD) measured slower

// Host-computed geometry of one ScanMatcher (ScanMatcher::Create + CorrelateScan's search spaces).
struct KtGeom {
    double scale, res;                 // 1 / resolution, GetResolution() = 1 / scale
    int grid_size, border, width, height, ws, data_size;
    int side, probs_ws, half, ksize;
    int n;                             // readings per scan
    int nxy;                           // coarse positions per axis
    int ctx, cty, clw;                 // coarse position tiles along x / y; log2 of gather lanes per tile row
    int npass;                         // 1, or 4 with response expansion
    int nang[4];
    double aoff[4];                    // coarse angle offset per pass
    double coff, cres;                 // coarse search offset / resolution
    double foff;                       // fine search offset (resolution = res)
    int fn, fnang;                     // fine positions per axis, fine angles
    double faoff, fares;               // fine angle offset / resolution
    double min_angle, ang_res, min_range, range_thr;
    double dvp, avp, mdp, map_;        // penalties
    double cares;                      // coarse angle resolution
    int use_expansion;
    int max_poses;
    size_t grid_stride;                // bytes per match slot grid
    int tiles_x, tiles_y, ntiles;      // 64 x 64-cell tiles of the grid (kt_addscans_kernel)
};

// ================================================== host policy ==================================================
enum KtBuild : int { KT_BUILD_DEFAULT, KT_BUILD_CAS, KT_BUILD_PER_BASE };  // SLAM2D_KT_BUILD unset / cas / per_base

struct KtOptions {
    int tile_w = 16;      // SLAM2D_KT_TW: coarse tile of 16 x 16, 32 x 8 or 64 x 4 positions (kt_geometry)
    int angle_group = 1;  // SLAM2D_KT_AG: angles per kt_coarse_kernel workgroup, clamped to the pass's at plan time
    int slots = 0;        // SLAM2D_KT_SLOTS: > 0 caps the match slots resident at once (kt_slots)
    KtBuild build = KT_BUILD_DEFAULT;  // the CAS AddScans kernels instead of the binned one (kt_plan_chunk)
    // SLAM2D_POISON != 0 (test hook): fill every buffer with 0xA5 bytes first, so that a kernel reading memory the
    // context never initialised fails its parity test instead of passing on fresh zero pages
    bool poison = false;
};

// Every matcher knob, through get (the library: getenv).  Returns NULL, or the message of the refusal: a number
// that is not one (kt_create then fails with KT_EINVAL).
inline const char *kt_parse_options(KtOptions &o, const char *(*get)(const char *))
{
    o = KtOptions{};
    int poison = 0;
    if (const char *v = get("SLAM2D_KT_TW"))
        if (!parse_knob_int(v, o.tile_w) || (o.tile_w != 16 && o.tile_w != 32 && o.tile_w != 64))
            return "SLAM2D_KT_TW must be 16, 32 or 64";
    if (const char *v = get("SLAM2D_KT_AG"))
        if (!parse_knob_int(v, o.angle_group)) return "SLAM2D_KT_AG must be an integer";
    if (const char *v = get("SLAM2D_KT_SLOTS"))
        if (!parse_knob_int(v, o.slots)) return "SLAM2D_KT_SLOTS must be an integer";
    if (const char *v = get("SLAM2D_POISON"))
        if (!parse_knob_int(v, poison)) return "SLAM2D_POISON must be an integer";
    o.poison = poison != 0;
    if (const char *v = get("SLAM2D_KT_BUILD"))
        o.build = !strcmp(v, "cas") ? KT_BUILD_CAS : !strcmp(v, "per_base") ? KT_BUILD_PER_BASE : KT_BUILD_DEFAULT;
    return nullptr;
}

inline double kt_h_round(double v) { return v >= 0.0 ? floor(v + 0.5) : ceil(v - 0.5); }  // math::Round
inline int kt_align8(int v) { return (v + 7) & ~7; }
inline size_t kt_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ScanMatcher::Create + CorrelationGrid::CreateGrid / CalculateKernel + CorrelateScan's search spaces,
// evaluated exactly as oracle/karto_oracle.c (ko_geom_init) does.  KT_OK, or KT_EINVAL with `refused` set.
inline int kt_geometry(const kt_laser &L, const kt_params &p, const KtOptions &o, KtGeom &g,
                       std::vector<unsigned char> &kernel, const char *&refused)
{
    const auto no = [&](const char *what) {
        refused = what;
        return KT_EINVAL;
    };
    g = KtGeom{};
    if (!(p.resolution > 0) || !(p.search_size > 0) || p.smear_deviation < 0 || !(L.range_threshold > 0))
        return no("ScanMatcher::Create rejects these parameters (resolution, searchSize, smear, rangeThreshold)");
    if (L.n_readings < 1 || L.n_readings > KT_MAX_READINGS) return no("n_readings must be in [1, 4096]");
    if (!(p.coarse_angle_resolution > 0) || !(p.fine_search_angle_offset > 0) || !(p.coarse_search_angle_offset > 0))
        return no("angle offsets / resolutions must be > 0");
    g.side = (int)(uint32_t)(kt_h_round(p.search_size / p.resolution) + 1);
    const int margin = (int)(uint32_t)ceil(L.range_threshold / p.resolution);
    g.grid_size = g.side + 2 * margin;
    g.border = (int)kt_h_round(2.0 * p.smear_deviation / p.resolution) + 1;
    g.width = g.grid_size + 2 * g.border;
    g.height = g.width;
    g.ws = kt_align8(g.width);
    if ((double)g.ws * g.height > 2.0e9) return no("correlation grid larger than 2^31 cells");
    g.data_size = g.ws * g.height;
    g.probs_ws = kt_align8(g.side);
    g.scale = 1.0 / p.resolution;
    g.res = 1.0 / g.scale;
    if (!(p.smear_deviation >= 0.5 * g.res && p.smear_deviation <= 10 * g.res))
        return no("smear deviation must be between 0.5 and 10 resolutions (CalculateKernel)");
    g.half = (int)kt_h_round(2.0 * p.smear_deviation / g.res);
    g.ksize = 2 * g.half + 1;
    if (g.ksize > 41) return no("smear kernel wider than 41 cells");
    kernel.assign((size_t)g.ksize * g.ksize, 0);
    for (int i = -g.half; i <= g.half; i++)
        for (int j = -g.half; j <= g.half; j++) {
            const double d = hypot(i * g.res, j * g.res);
            const double z = exp(-0.5 * pow(d / p.smear_deviation, 2));
            const uint32_t kv = (uint32_t)kt_h_round(z * KT_OCC);
            kernel[(i + g.half) + g.ksize * (j + g.half)] = (unsigned char)kv;
            if ((i != 0 || j != 0) && kv >= (uint32_t)KT_OCC)
                return no("smear kernel has an off-centre value of 100 (smear_deviation too close to "
                          "10 * resolution): AddScan would become order-dependent; not supported");
        }
    g.n = L.n_readings;
    g.coff = 0.5 * ((double)g.side - 1) * g.res;
    g.cres = 2 * g.res;
    g.nxy = (int)(uint32_t)(kt_h_round(g.coff * 2.0 / g.cres) + 1);
    {
        // coarse tile shape: 16 x 16 positions.  SLAM2D_KT_TW = 32 / 64 makes it 32 x 8 / 64 x 4 (a wave's
        // gather then touches 8 / 4 grid rows of 64 / 128 bytes instead of 16 rows of 32 bytes): measured
        // slower (loop window 22.3 k -> 20.1 k / 20.8 k matches/s, sequential batch 321 k -> 269 k), so the
        // coarse kernel is not bound by L2 line requests per gather instruction
        int tw = o.tile_w;
        g.clw = tw >= 64 ? 4 : (tw >= 32 ? 3 : 2);
        tw = 4 << g.clw;
        g.ctx = (g.nxy + tw - 1) / tw;
        g.cty = (g.nxy + (256 / tw) - 1) / (256 / tw);
    }
    if (g.nxy > KT_MAX_NXY) return no("coarse search wider than 1024 positions");
    g.use_expansion = p.use_response_expansion ? 1 : 0;
    g.npass = g.use_expansion ? 4 : 1;
    g.cares = p.coarse_angle_resolution;
    double aoff = p.coarse_search_angle_offset;
    for (int i = 0; i < 4; ++i) {
        if (i > 0) aoff += 20 * 0.01745329251994329577;  // DegreesToRadians(20)
        g.aoff[i] = aoff;
        g.nang[i] = (int)(uint32_t)(kt_h_round(aoff * 2.0 / g.cares) + 1);
    }
    g.foff = g.cres * 0.5;
    g.fn = (int)(uint32_t)(kt_h_round(g.foff * 2.0 / g.res) + 1);
    g.faoff = 0.5 * p.coarse_angle_resolution;
    g.fares = p.fine_search_angle_offset;
    g.fnang = (int)(uint32_t)(kt_h_round(g.faoff * 2.0 / g.fares) + 1);
    if (g.fn != 3) return no("fine search must be 3x3 positions");
    if (g.fnang > KT_FINE_MAX_ANG) return no("fine search has more than 64 angles");
    if (g.nang[g.npass - 1] > 4096) return no("coarse search has more than 4096 angles");
    g.min_angle = L.minimum_angle;
    g.ang_res = L.angular_resolution;
    g.min_range = L.minimum_range;
    g.range_thr = L.range_threshold;
    g.dvp = p.distance_variance_penalty;
    g.avp = p.angle_variance_penalty;
    g.mdp = p.minimum_distance_penalty;
    g.map_ = p.minimum_angle_penalty;
    const double mp = (double)g.nxy * g.nxy * g.nang[g.npass - 1];
    if (mp > 2.0e8) return no("coarse search window larger than 2e8 poses");
    g.max_poses = (int)mp;
    g.grid_stride = kt_align256((size_t)g.data_size + 64);
    g.tiles_x = (g.ws + 63) / 64;
    g.tiles_y = (g.height + 63) / 64;
    g.ntiles = g.tiles_x * g.tiles_y;
    return KT_OK;
}

// kt_get_grid_info's ten words
inline void kt_grid_info_words(const KtGeom &g, int out[10])
{
    const int v[10] = {g.grid_size, g.border, g.width, g.ws, g.data_size, g.side, g.probs_ws, g.half, g.ksize,
                       g.max_poses};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}

// Match slots resident at once: a batch runs in chunks of this many matches (default: all of them).  Smaller chunks
// keep a chunk's grids cache-resident but were measured slower (the per-match select / fine workgroups are latency
// bound and need the whole batch to fill the GPU); SLAM2D_KT_SLOTS caps the slot memory.
inline int kt_slots(const KtOptions &o, int max_matches)
{
    const int want = o.slots > 0 && o.slots < max_matches ? o.slots : max_matches;
    return want < 1 ? 1 : want;
}

// AddScans by kt_addscans_kernel (tile-binned, plain stores) is possible: its LDS tables hold the grid's tiles and
// a match's base scans, and no CAS kernel was asked for.  (The context then has the kernel's scratch and dirty lists.)
inline bool kt_binned_eligible(const KtOptions &o, const KtGeom &g, int max_base)
{
    return g.ntiles <= KT_AS_MAX_TILES && max_base <= KT_AS_MAX_BASE && o.build == KT_BUILD_DEFAULT;
}

// kt_addscans_kernel | kt_build_kernel<0, 8>, one workgroup per match | kt_build_kernel<0, 4>, one per (match, base scan)
enum KtAddScans : int { KT_ADD_NONE, KT_ADD_BINNED, KT_ADD_PER_MATCH, KT_ADD_PER_BASE };
// kt_clear_tiles_kernel (the binned kernel's dirty tiles) | kt_build_kernel<1, 4> (the footprints again)
enum KtClear : int { KT_CLEAR_NONE, KT_CLEAR_TILES, KT_CLEAR_FOOTPRINT };
struct KtChunkPlan {
    KtAddScans add;
    int add_grid, add_block;
    KtClear clear;
    int clear_grid_x, clear_grid_y;  // block: KT_THREADS
    int select_threads;              // kt_select_kernel<256> or <1024>, one workgroup per match
    int fine_grid, fine_block;       // kt_fine_kernel (launched when the call refines)
    size_t prepare_lds;              // kt_prepare_kernel's dynamic LDS: a scan's points (double2) and two int arrays
    bool prepare_attr;               // ... above 64 KB: hipFuncSetAttribute(MaxDynamicSharedMemorySize) at kt_create
};

// What a chunk of `count` matches launches on a context of at most max_base base scans per match.
inline KtChunkPlan kt_plan_chunk(const KtOptions &o, const KtGeom &g, int max_base, int count)
{
    KtChunkPlan p{};
    const int per_base = (count + 7) / 8 * 8 * max_base;
    if (max_base > 0) {
        // the binned AddScans runs one workgroup per match: small batches use the per-(match, base scan) kernel
        const bool large = count >= 128;
        p.add = large && kt_binned_eligible(o, g, max_base) ? KT_ADD_BINNED
                : large && o.build != KT_BUILD_PER_BASE     ? KT_ADD_PER_MATCH
                                                            : KT_ADD_PER_BASE;
        p.add_grid = p.add == KT_ADD_PER_BASE ? per_base : count;
        p.add_block = p.add == KT_ADD_BINNED ? KT_AS_WAVES * 64 : p.add == KT_ADD_PER_MATCH ? 512 : KT_THREADS;
        p.clear = p.add == KT_ADD_BINNED ? KT_CLEAR_TILES : KT_CLEAR_FOOTPRINT;
        p.clear_grid_x = p.clear == KT_CLEAR_TILES ? count : per_base;
        p.clear_grid_y = p.clear == KT_CLEAR_TILES ? 4 : 1;
    }
    p.select_threads = g.nxy * g.nxy > 512 ? 1024 : KT_THREADS;
    p.fine_grid = count;
    p.fine_block = KT_FINE_THREADS;
    p.prepare_lds = (size_t)g.n * (2 * sizeof(double) + 2 * sizeof(int));
    p.prepare_attr = p.prepare_lds > 65536;
    return p;
}

struct KtCoarsePlan {
    int angle_group;      // angles per workgroup
    long long blocks;     // 8-match groups x position tiles x angle groups
    const char *refused;  // NULL, or why the launch is refused (KT_EINVAL)
};

// kt_coarse_kernel of pass `pass`.  Angles per workgroup: 1 (r02 A/B, loop window / sequential batch: 7 angles 5 % /
// 3 angles 5 % slower, 21 angles 29 % slower -- fewer workgroups left in flight for the gathers); SLAM2D_KT_AG
// overrides.
inline KtCoarsePlan kt_plan_coarse(const KtOptions &o, const KtGeom &g, int count, int pass)
{
    const long long per_angle = (long long)((count + 7) / 8) * 8 * g.ctx * g.cty;
    const int nA = g.nang[pass];
    const int ag = o.angle_group < 1 ? 1 : (o.angle_group > nA ? nA : o.angle_group);
    KtCoarsePlan p{ag, per_angle * ((nA + ag - 1) / ag), nullptr};
    if (p.blocks > 0x7fffffffLL) p.refused = "coarse launch too large: lower the batch size";
    return p;
}

// ---- the occupancy-grid rebuild (karto_grid_capi.hip) ----
constexpr int KG_MAX_SPLIT = 32;

// SLAM2D_KG_SPLIT: workgroups per tile, overriding kg_split_rule (tests, A/B); <= 0 or unset: the rule
inline const char *kg_parse_options(int &force_split, const char *(*get)(const char *))
{
    force_split = 0;
    if (const char *v = get("SLAM2D_KG_SPLIT"))
        if (!parse_knob_int(v, force_split)) return "SLAM2D_KG_SPLIT must be an integer";
    return nullptr;
}

// Workgroups per tile.  One owner per tile (plain stores, no memset) as soon as the tiles alone fill every
// CU's four resident workgroups (the tile's 33 KB of LDS); below that the tiles' scan lists are split so that
// about 4 * CUs workgroups run, never finer than 32 scans per workgroup.  The split is rounded up to 1, 2, 4 or
// a multiple of 8: workgroups go to the 8 XCDs round-robin and the part is blockIdx % split, so each XCD's L2
// then serves the rays of split / 8 parts only -- the supposed cause of what was measured, 15 parts 2.58 ms and
// 16 parts 1.73 ms per rebuild (profiles/r07/karto_grid.md).
inline int kg_split_rule(int force_split, int num_cus, int ntiles, int count)
{
    if (force_split > 0) return force_split < KG_MAX_SPLIT ? force_split : KG_MAX_SPLIT;
    const int want = 4 * num_cus;
    if (ntiles >= want) return 1;
    int split = (want + ntiles - 1) / ntiles;
    const int by_scans = (count + 31) / 32;
    split = split < by_scans ? split : by_scans;
    if (split < 1) split = 1;
    if (split > 4) split = (split + 7) & ~7;
    else if (split == 3) split = 4;
    return split < KG_MAX_SPLIT ? split : KG_MAX_SPLIT;
}

}  // namespace s2d
