// karto_grid_kernels.hip -- device side of the Karto occupancy-grid rebuild
// (karto::OccupancyGrid::CreateFromScans, lesson6/lib/open_karto/include/open_karto/Karto.h:5659-5673).
//
//   kg_bbox_kernel     one workgroup per scan: LocalizedRangeScan::Update's bounding box (Karto.h:5418-5424),
//                      the sensor position plus the readings InRange(r, minimumRange, rangeThreshold).
//   kg_bbox_reduce_kernel  one workgroup: ComputeDimensions' union of the scan boxes (Karto.h:5810-5814).
//                      Minimum / maximum of doubles do not depend on the order, so both steps are exact.
//   kg_rays_kernel     one workgroup per scan, after the host has fixed the offset: AddScan's reading rules
//                      (Karto.h:5869-5887) and RayTrace's WorldToGrid of both ends (:5917-5918, :4237-4252);
//                      per beam the end cell + the valid-end flag (8 bytes), per scan the start cell and the
//                      integer box of everything its rays can touch.
//   kg_trace_kernel    the hot path.  A workgroup owns one 64 x 64-cell tile of the grid with both u32
//                      counter planes in LDS (32 KB + the scan list: four workgroups, 16 waves, per CU's
//                      160 KB; a 128 x 64 tile would leave two, 32 x 32 quadruples the ray culls): it visits the scans
//                      whose box meets the tile, culls their rays by the end points' box, clips each
//                      survivor to the tile in closed form (karto_grid_line.h), adds with LDS atomics, and
//                      writes the tile with plain row-contiguous stores -- no global atomic and no memset.
//                      When the map has too few tiles to fill the chip, `split` workgroups share a tile's
//                      scan list and merge with row-contiguous integer atomicAdds into zeroed planes.
//   kg_update_kernel   OccupancyGrid::Update / UpdateCell (Karto.h:5953-5990) and karto_slam.cc:546-569's
//                      bytes: 16 cells per lane, both byte planes with 16-byte stores.
// Doubles throughout, -ffp-contract=off and detmath.h's sin / cos as in kt_prepare_kernel;
// tests/ref/karto_grid_ref.c evaluates the same sequence with the literal TraceLine loop.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/slam2d/karto_grid.h"
#include "detmath.h"
#include "karto_grid_line.h"

namespace s2d {

constexpr int KG_THREADS = 256;
constexpr int KG_TILE = 64;
constexpr int KG_SKIP = INT_MIN;  // a beam AddScan ignores
constexpr double KG_TOL = 1e-06;  // KT_TOLERANCE
constexpr double KG_BOX_INIT = 999999999999999999.99999;  // BoundingBox2() (Karto.h:2765)

struct KgGeom {
    double min_angle, ang_res, min_range, range_thr, max_range;
    double scale;          // 1 / resolution
    double off_x, off_y;   // the grid's offset (the bounding box minimum)
    double occ_thr;
    uint32_t min_pass;
    int n;                 // readings per scan
    int width, height;
    int tiles_x, tiles_y;
    int split;             // workgroups per tile
};

// per scan: start cell and the box of its rays' end cells and start cell (empty: bx0 > bx1)
struct KgScan {
    int ox, oy, bx0, by0, bx1, by1, pad0, pad1;
};

__device__ __forceinline__ double kg_round(double v) { return v >= 0.0 ? floor(v + 0.5) : ceil(v - 0.5); }

__device__ __forceinline__ double kg_wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ double kg_wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int kg_wave_imin(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int kg_wave_imax(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// box[4] = min x, min y, max x, max y over the block
__device__ __forceinline__ void kg_block_box(double x0, double y0, double x1, double y1, double *out)
{
    __shared__ double sb[KG_THREADS / 64][4];
    x0 = kg_wave_min(x0);
    y0 = kg_wave_min(y0);
    x1 = kg_wave_max(x1);
    y1 = kg_wave_max(y1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sb[w][0] = x0, sb[w][1] = y0, sb[w][2] = x1, sb[w][3] = y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < KG_THREADS / 64; ++k) {
            x0 = sb[k][0] < x0 ? sb[k][0] : x0;
            y0 = sb[k][1] < y0 ? sb[k][1] : y0;
            x1 = sb[k][2] > x1 ? sb[k][2] : x1;
            y1 = sb[k][3] > y1 ? sb[k][3] : y1;
        }
        out[0] = x0, out[1] = y0, out[2] = x1, out[3] = y1;
    }
}

__global__ void __launch_bounds__(KG_THREADS)
kg_bbox_kernel(KgGeom g, const double *__restrict__ ranges, const double *__restrict__ poses,
               double *__restrict__ boxes)
{
    const int s = blockIdx.x;
    const double *raw = ranges + (size_t)s * g.n;
    const double px = poses[3 * s], py = poses[3 * s + 1], ph = poses[3 * s + 2];
    double x0 = KG_BOX_INIT, y0 = KG_BOX_INIT, x1 = -KG_BOX_INIT, y1 = -KG_BOX_INIT;
    // m_BoundingBox.Add(scanPose.GetPosition())
    x0 = px < x0 ? px : x0, y0 = py < y0 ? py : y0;
    x1 = px > x1 ? px : x1, y1 = py > y1 ? py : y1;
    for (int i = threadIdx.x; i < g.n; i += KG_THREADS) {
        const double r = raw[i];
        if (!(r >= g.min_range && r <= g.range_thr)) continue;
        const double angle = ph + g.min_angle + (double)(uint32_t)i * g.ang_res;
        const double x = px + (r * sdm_cos(angle));
        const double y = py + (r * sdm_sin(angle));
        x0 = x < x0 ? x : x0, y0 = y < y0 ? y : y0;
        x1 = x > x1 ? x : x1, y1 = y > y1 ? y : y1;
    }
    kg_block_box(x0, y0, x1, y1, boxes + 4 * (size_t)s);
}

__global__ void __launch_bounds__(KG_THREADS)
kg_bbox_reduce_kernel(int count, const double *__restrict__ boxes, double *__restrict__ out)
{
    double x0 = KG_BOX_INIT, y0 = KG_BOX_INIT, x1 = -KG_BOX_INIT, y1 = -KG_BOX_INIT;
    for (int s = threadIdx.x; s < count; s += KG_THREADS) {
        const double *b = boxes + 4 * (size_t)s;
        x0 = b[0] < x0 ? b[0] : x0, y0 = b[1] < y0 ? b[1] : y0;
        x1 = b[2] > x1 ? b[2] : x1, y1 = b[3] > y1 ? b[3] : y1;
    }
    kg_block_box(x0, y0, x1, y1, out);
}

// ray word: .x = end cell x (KG_SKIP: ignored beam), .y = end cell y * 2 + isEndPointValid
__global__ void __launch_bounds__(KG_THREADS)
kg_rays_kernel(KgGeom g, const double *__restrict__ ranges, const double *__restrict__ poses,
               int2 *__restrict__ rays, KgScan *__restrict__ scans)
{
    __shared__ int sb[KG_THREADS / 64][4];
    const int s = blockIdx.x;
    const double *raw = ranges + (size_t)s * g.n;
    const double px = poses[3 * s], py = poses[3 * s + 1], ph = poses[3 * s + 2];
    const int ox = (int)kg_round((px - g.off_x) * g.scale);
    const int oy = (int)kg_round((py - g.off_y) * g.scale);
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
    for (int i = threadIdx.x; i < g.n; i += KG_THREADS) {
        const double r = raw[i];
        int2 w = make_int2(KG_SKIP, 0);
        if (!(r <= g.min_range || r >= g.max_range || isnan(r))) {
            const double angle = ph + g.min_angle + (double)(uint32_t)i * g.ang_res;
            double x = px + (r * sdm_cos(angle));
            double y = py + (r * sdm_sin(angle));
            const int valid = r < (g.range_thr - KG_TOL) ? 1 : 0;
            if (r >= g.range_thr) {
                const double ratio = g.range_thr / r;
                const double dx = x - px;
                const double dy = y - py;
                x = px + ratio * dx;
                y = py + ratio * dy;
            }
            const int gx = (int)kg_round((x - g.off_x) * g.scale);
            const int gy = (int)kg_round((y - g.off_y) * g.scale);
            w = make_int2(gx, gy * 2 + valid);
            bx0 = min(bx0, gx), by0 = min(by0, gy);
            bx1 = max(bx1, gx), by1 = max(by1, gy);
        }
        rays[(size_t)s * g.n + i] = w;
    }
    bx0 = kg_wave_imin(bx0), by0 = kg_wave_imin(by0);
    bx1 = kg_wave_imax(bx1), by1 = kg_wave_imax(by1);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sb[wv][0] = bx0, sb[wv][1] = by0, sb[wv][2] = bx1, sb[wv][3] = by1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < KG_THREADS / 64; ++k) {
            bx0 = min(bx0, sb[k][0]), by0 = min(by0, sb[k][1]);
            bx1 = max(bx1, sb[k][2]), by1 = max(by1, sb[k][3]);
        }
        if (bx0 <= bx1) {  // some beam is traced: its line starts at the scan's cell
            bx0 = min(bx0, ox), by0 = min(by0, oy);
            bx1 = max(bx1, ox), by1 = max(by1, oy);
        }
        KgScan o;
        o.ox = ox, o.oy = oy, o.bx0 = bx0, o.by0 = by0, o.bx1 = bx1, o.by1 = by1, o.pad0 = 0, o.pad1 = 0;
        scans[s] = o;
    }
}

// one ray's share of the tile [tx0, tx1] x [ty0, ty1] into the tile's LDS planes
__device__ __forceinline__ void kg_trace_ray(int2 w, const KgScan &sc, int tx0, int ty0, int tx1, int ty1,
                                             uint32_t *s_pass, uint32_t *s_hits)
{
    if (w.x == KG_SKIP) return;
    const int ex = w.x, ey = w.y >> 1;
    // the line stays in the box of its two ends
    if (min(sc.ox, ex) > tx1 || max(sc.ox, ex) < tx0 || min(sc.oy, ey) > ty1 || max(sc.oy, ey) < ty0) return;
    const kgl_line L = kgl_setup(sc.ox, sc.oy, ex, ey);
    int ia, ib;
    if (kgl_clip(&L, tx0, ty0, tx1, ty1, &ia, &ib)) {
        int c = kgl_carry(&L, ia);
        int err = kgl_error(&L, ia, c);
        for (int k = ia; k <= ib; ++k) {
            const int a = L.x0 + k, b = L.y0 + L.ystep * c;
            const int lx = (L.steep ? b : a) - tx0, ly = (L.steep ? a : b) - ty0;
            // the clip guarantees the tile; the test keeps a corrupt input (NaN pose) off other memory
            if ((unsigned)lx < (unsigned)KG_TILE && (unsigned)ly < (unsigned)KG_TILE)
                atomicAdd(&s_pass[ly * KG_TILE + lx], 1u);
            err += L.dy;
            if (2 * err >= L.dx) {
                ++c;
                err -= L.dx;
            }
        }
    }
    // RayTrace's end point (Karto.h:5924-5942) belongs to the tile that holds the end cell
    if ((w.y & 1) && ex >= tx0 && ex <= tx1 && ey >= ty0 && ey <= ty1) {
        const int k = (ey - ty0) * KG_TILE + (ex - tx0);
        atomicAdd(&s_pass[k], 1u);
        atomicAdd(&s_hits[k], 1u);
    }
}

// grid = tiles_x * tiles_y * split workgroups
__global__ void __launch_bounds__(KG_THREADS)
kg_trace_kernel(KgGeom g, int count, const int2 *__restrict__ rays, const KgScan *__restrict__ scans,
                uint32_t *__restrict__ pass, uint32_t *__restrict__ hits)
{
    __shared__ uint32_t s_pass[KG_TILE * KG_TILE];
    __shared__ uint32_t s_hits[KG_TILE * KG_TILE];
    __shared__ int s_list[KG_THREADS];
    __shared__ int s_cnt;

    const int tid = threadIdx.x;
    const int tile = blockIdx.x / g.split, part = blockIdx.x % g.split;
    const int tx0 = (tile % g.tiles_x) * KG_TILE, ty0 = (tile / g.tiles_x) * KG_TILE;
    const int tx1 = min(tx0 + KG_TILE, g.width) - 1, ty1 = min(ty0 + KG_TILE, g.height) - 1;  // inclusive, in the grid

    for (int k = tid; k < KG_TILE * KG_TILE; k += KG_THREADS) {
        s_pass[k] = 0;
        s_hits[k] = 0;
    }
    __syncthreads();
    // this workgroup's share of the scans
    const int per = (count + g.split - 1) / g.split;
    const int sa = part * per, sb = min(sa + per, count);

    for (int base = sa; base < sb; base += KG_THREADS) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const int s = base + tid;
        if (s < sb) {
            const KgScan sc = scans[s];
            if (sc.bx0 <= tx1 && sc.bx1 >= tx0 && sc.by0 <= ty1 && sc.by1 >= ty0) s_list[atomicAdd(&s_cnt, 1)] = s;
        }
        __syncthreads();
        const int cnt = s_cnt;
        // a wave per listed scan; each lane fetches four of its rays before it walks any, so the walk of one
        // hides the L2 latency of the others (one dependent load per ray left the kernel latency-bound)
        for (int j = tid >> 6; j < cnt; j += KG_THREADS / 64) {
            const int sj = s_list[j];
            const KgScan sc = scans[sj];
            const int2 *rj = rays + (size_t)sj * g.n;
            for (int i0 = tid & 63; i0 < g.n; i0 += 4 * 64) {
                int2 w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + 64 * q;
                    w[q] = i < g.n ? rj[i] : make_int2(KG_SKIP, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) kg_trace_ray(w[q], sc, tx0, ty0, tx1, ty1, s_pass, s_hits);
            }
        }
        __syncthreads();  // every lane has read s_cnt and s_list before the next round resets them
    }
    // the tile's rows: 64 consecutive lanes write (or add) 256 contiguous bytes
    for (int k = tid; k < KG_TILE * KG_TILE; k += KG_THREADS) {
        const int lx = k & (KG_TILE - 1), ly = k >> 6;
        const int x = tx0 + lx, y = ty0 + ly;
        if (x > tx1 || y > ty1) continue;
        const size_t idx = (size_t)y * g.width + x;
        const uint32_t p = s_pass[k], h = s_hits[k];
        if (g.split == 1) {
            pass[idx] = p;
            hits[idx] = h;
        } else {
            if (p) atomicAdd(&pass[idx], p);
            if (h) atomicAdd(&hits[idx], h);
        }
    }
}

__device__ __forceinline__ void kg_update_cell(uint32_t p, uint32_t h, const KgGeom &g, uint32_t &st, uint32_t &ro)
{
    st = 0;     // GridStates_Unknown
    ro = 0xFF;  // -1
    if (p > g.min_pass) {
        const double ratio = (double)h / (double)p;
        if (ratio > g.occ_thr) {
            st = 100, ro = 100;  // GridStates_Occupied
        } else {
            st = 255, ro = 0;    // GridStates_Free
        }
    }
}

// 16 cells per lane; the planes are allocated to a multiple of 16 cells, `cells` is width * height
__global__ void __launch_bounds__(KG_THREADS)
kg_update_kernel(KgGeom g, size_t cells, const uint32_t *__restrict__ pass, const uint32_t *__restrict__ hits,
                 uint8_t *__restrict__ state, int8_t *__restrict__ ros)
{
    const size_t c0 = ((size_t)blockIdx.x * KG_THREADS + threadIdx.x) * 16;
    if (c0 >= cells) return;
    if (c0 + 16 <= cells) {
        uint32_t sw[4], rw[4];
        for (int q = 0; q < 4; ++q) {
            const uint4 p = *reinterpret_cast<const uint4 *>(pass + c0 + 4 * q);
            const uint4 h = *reinterpret_cast<const uint4 *>(hits + c0 + 4 * q);
            uint32_t s0, s1, s2, s3, r0, r1, r2, r3;
            kg_update_cell(p.x, h.x, g, s0, r0);
            kg_update_cell(p.y, h.y, g, s1, r1);
            kg_update_cell(p.z, h.z, g, s2, r2);
            kg_update_cell(p.w, h.w, g, s3, r3);
            sw[q] = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
            rw[q] = r0 | (r1 << 8) | (r2 << 16) | (r3 << 24);
        }
        *reinterpret_cast<uint4 *>(state + c0) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
        *reinterpret_cast<uint4 *>(ros + c0) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
    } else {
        for (size_t c = c0; c < cells; ++c) {
            uint32_t s0, r0;
            kg_update_cell(pass[c], hits[c], g, s0, r0);
            state[c] = (uint8_t)s0;
            ros[c] = (int8_t)(uint8_t)r0;
        }
    }
}

}  // namespace s2d
