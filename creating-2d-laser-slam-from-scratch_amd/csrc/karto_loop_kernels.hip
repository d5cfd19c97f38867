// karto_loop_kernels.hip -- HIP kernels of the Karto loop-closure and near-chain candidate search (gfx950).
//
// Reference: MapperGraph on the scans' reference poses (lesson6/lib/open_karto/src/Mapper.cpp; the C-ABI is
// include/slam2d/karto_loop.h).
//   kl_reference_kernel  one workgroup per scan: LocalizedRangeScan::Update's barycentre (Karto.h:5374-5416).  The
//                        points of 1024 beams at a time are computed by all lanes into LDS; then one lane of wave 0
//                        adds the x components and one lane of wave 1 the y components in beam order, one at a time
//                        -- the reference's own order (a tree sum rounds differently); an invalid reading adds +0.0.
//   kl_refresh_kernel    the same value for the scans named by rows of device memory: one launch of a host-known size,
//                        a prefix sum of the rows' counts in every workgroup's LDS, one wave per scan.
//   kl_search_kernel     one workgroup per query.  All lanes: the squared distances and, per scan, four threshold
//                        bits.  Wave 0 and wave 1: the two breadth-first traversals (link and loop distance), each in
//                        queue-prefix batches of up to 64 vertices with wave-level operations only, no workgroup
//                        barrier: a batch's expansions get the tentative positions (queue position, adjacency
//                        position) by an integer atomicMin per vertex slot in LDS, so a vertex pushed twice keeps its
//                        first position, and an order-preserving compaction appends the winners.  All lanes again:
//                        FindPossibleLoopClosure's chains as the runs of "append" scans, FindNearChains' as the runs
//                        of in-range scans that hold a near-linked scan, ordered by the queue position of their first
//                        near-linked member (integer atomicMin per run, then a compaction over the queue positions);
//                        GetClosestScanToPose per near chain by one wave.
//   kl_closest_kernel    one wave per (scan, chain): GetClosestScanToPose and LinkChainToScan's distance test.
//   kl_emit_scan_kernel / kl_emit_write_kernel  the chains of a search as kt_match_batch_device's arrays.
//   kl_edit_vertices_kernel / kl_edit_edges_kernel  AddVertex / AddEdge on the device, and the adjacency rebuilt.
// All arithmetic is double with -ffp-contract=off and detmath.h's sin / cos; no float atomics anywhere.  The CPU
// restatement tests/ref/karto_loop_ref.c gives the same bits.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/slam2d/karto_loop.h"
#include "detmath.h"
#include "graph_edit_device.h"

namespace s2d {

constexpr int KL_THREADS = 256;
constexpr int KL_WAVES = KL_THREADS / 64;
constexpr int KL_REF_CHUNK = 1024;
constexpr int KL_UNSEEN = INT_MAX;

// per-scan bits of a query
constexpr int KL_F_LINK_RANGE = 1;  // d2 < link^2 + tol  (FindNearChains :1223, LinkChainToScan :1163)
constexpr int KL_F_LOOP_RANGE = 2;  // d2 < loop^2 + tol  (FindPossibleLoopClosure :1361)
constexpr int KL_F_LINK_VISIT = 4;  // d2 <= link^2 - tol (NearScanVisitor, Mapper.h:636)
constexpr int KL_F_LOOP_VISIT = 8;  // d2 <= loop^2 - tol

struct KlHdr {
    int n_scans, n_edges, pool_offset, pad_;
};

struct KlDev {
    int max_scans, max_edges, max_queries, chain_stride;
    // the laser and the parameters
    double minimum_angle, angular_resolution, minimum_range, range_threshold;
    int n_readings, use_barycenter, min_chain, pad_;
    double link_hi, link_lo, loop_hi, loop_lo;  // d * d + tol, d * d - tol
    // graphs
    const KlHdr *hdr;    // [G]
    const int *adj_off;  // [G][max_scans + 1]
    const int2 *adj;     // [G][2 max_edges]: other end, edge index
    double2 *ref;        // [G][max_scans]
    // query slots
    kl_result *res;             // [Q]
    kl_query *queries;          // [Q]: the last search's queries
    double *d2;                 // [Q][max_scans]
    int *near_link, *near_loop; // [Q][max_scans]
    kl_loop_chain *loop_chains; // [Q][chain_stride]
    kl_near_chain *near_chains; // [Q][chain_stride]
    int2 *emit_off;             // [Q + 1]: match and base-index offsets of a slot
    int *emit_info;             // [2]: total matches, status
};

// LDS of kl_search_kernel: pos0 int[N] | pos1 int[N + 2] | queue uint16[2][N] | flags uint8[N], padded
__host__ __device__ inline size_t kl_search_lds(int max_scans)
{
    return (size_t)max_scans * 13 + 32;
}

// wave-level ordering of LDS traffic between the lanes of one wave (no workgroup barrier)
__device__ __forceinline__ void kl_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int kl_wave_inscan(int v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive scan of v over the workgroup's KL_THREADS lanes (sw: KL_WAVES ints of LDS); *total is the sum
__device__ inline int kl_block_exscan(int v, int *sw, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = kl_wave_inscan(v, lane);
    __syncthreads();
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < KL_WAVES; ++w) {
        if (w < wave) base += sw[w];
        sum += sw[w];
    }
    *total = sum;
    return base + incl - v;
}

// =================================================================================================
// kl_reference_kernel: ranges + poses -> reference positions of scans [first, first + gridDim.x) of graph g
// =================================================================================================
__global__ void __launch_bounds__(KL_THREADS)
kl_reference_kernel(KlDev D, int g, int first, const double *__restrict__ ranges, const double *__restrict__ poses)
{
    __shared__ double s_px[KL_REF_CHUNK], s_py[KL_REF_CHUNK];
    __shared__ unsigned char s_ok[KL_REF_CHUNK];
    __shared__ double s_sum[2];
    __shared__ int s_cnt;

    const int b = blockIdx.x, tid = threadIdx.x, n = D.n_readings;
    const double *raw = ranges + (size_t)b * n;
    const double px = poses[3 * (size_t)b], py = poses[3 * (size_t)b + 1], ph = poses[3 * (size_t)b + 2];
    double sum = 0.0;  // wave 0 lane 0: x; wave 1 lane 0: y
    int cnt = 0;
    if (D.use_barycenter) {
        for (int c0 = 0; c0 < n; c0 += KL_REF_CHUNK) {
            const int cn = min(KL_REF_CHUNK, n - c0);
            for (int k = tid; k < cn; k += KL_THREADS) {
                const int i = c0 + k;
                const double r = raw[i];
                const bool ok = r >= D.minimum_range && r <= D.range_threshold;  // math::InRange
                s_ok[k] = ok ? 1 : 0;
                double x = 0.0, y = 0.0;
                if (ok) {
                    const double angle = ph + D.minimum_angle + (double)(unsigned)i * D.angular_resolution;
                    x = px + (r * sdm_cos(angle));
                    y = py + (r * sdm_sin(angle));
                }
                s_px[k] = x;
                s_py[k] = y;
            }
            __syncthreads();
            // An invalid reading's slot holds +0.0 and is added like the others, so the chain has no branch and its LDS
            // reads run ahead of the adds.  s + (+0.0) is s bit for bit unless s is -0.0, and the sum never is: it
            // starts from +0.0, and an IEEE sum in round-to-nearest is -0.0 only when both terms are.
            if (tid == 0) {
#pragma unroll 8
                for (int k = 0; k < cn; ++k) {
                    sum = sum + s_px[k];
                    cnt += s_ok[k];
                }
            } else if (tid == 64) {
#pragma unroll 8
                for (int k = 0; k < cn; ++k) sum = sum + s_py[k];
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        s_sum[0] = sum;
        s_cnt = cnt;
    } else if (tid == 64) {
        s_sum[1] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        double2 out;
        if (s_cnt > 0) {
            const double np = (double)s_cnt;
            out.x = s_sum[0] / np;
            out.y = s_sum[1] / np;
        } else {
            out.x = px;
            out.y = py;
        }
        D.ref[(size_t)g * D.max_scans + first + b] = out;
    }
}

// =================================================================================================
// kl_refresh_kernel: kl_reference_kernel's result for the scans that rows of device memory name
// =================================================================================================
// Row i names scans [first, first + count) of its graph, read from pool slots [pool_first, pool_first + count); count
// < 0 stands for "through the graph's last scan" of the device header.  The host knows none of the counts, so the
// launch has a fixed size (scan_refresh_plan.h) and every workgroup builds the same plan: the rows' resolved counts
// and their exclusive prefix sum in LDS.  Scan s of that list belongs to the row found by bisection, and the waves of
// the whole grid take the scans s = wave, wave + waves, ... -- one wave per scan, with no workgroup barrier after the
// plan.  A wave computes 64 points at a time into its own slice of LDS; then lane 0 adds the x components and lane 1
// the y components in beam order, in one loop, as kl_reference_kernel's two lanes do.  Workgroup 0 alone reports:
// d_resolved_out and the refused rows.
struct KlRefresh {
    const kl_refresh_row *rows;
    const double *ranges, *poses;  // [pool_scans][n_readings], [pool_scans][3]
    int2 *resolved;                // [n_rows] or NULL
    unsigned long long *info;      // ge_refuse's two words
    int n_rows, pool_scans, max_graphs;
    unsigned seq;
};

// the row's count as it is applied, 0 for a skipped or refused row; *status != KL_OK for a refused one
__device__ inline int kl_refresh_resolve(const KlDev &D, const KlRefresh &R, const kl_refresh_row &r, int *status)
{
    *status = KL_OK;
    if (r.graph < 0) return 0;
    if (r.graph >= R.max_graphs || r.first < 0) {
        *status = KL_EINVAL;
        return 0;
    }
    const int count = r.count >= 0 ? r.count : max(D.hdr[r.graph].n_scans - r.first, 0);
    if (r.first > D.max_scans - count) {
        *status = KL_ERANGE;  // scans beyond the context's max_scans
        return 0;
    }
    if (count > 0 && (r.pool_first < 0 || r.pool_first > R.pool_scans - count)) {
        *status = KL_ERANGE;  // a slot outside the pool
        return 0;
    }
    return count;
}

__global__ void __launch_bounds__(KL_THREADS) kl_refresh_kernel(KlDev D, KlRefresh R)
{
    __shared__ int s_off[KL_REFRESH_MAX_ROWS + 1];
    __shared__ int s_sw[KL_WAVES];
    __shared__ double s_pt[KL_WAVES][2][64];  // a wave's points: x components, y components

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = D.n_readings;
    for (int i = tid; i < R.n_rows; i += KL_THREADS) {
        const kl_refresh_row r = R.rows[i];
        int status;
        const int count = kl_refresh_resolve(D, R, r, &status);
        s_off[i] = count;
        if (blockIdx.x == 0) {
            if (status != KL_OK) ge_refuse(R.info, R.seq, i, status);
            if (R.resolved) R.resolved[i] = status == KL_OK && r.graph >= 0 ? make_int2(r.pool_first, count) : make_int2(0, 0);
        }
    }
    __syncthreads();
    const int total = ge_exscan_array(s_off, R.n_rows, s_sw);  // ends with a barrier: the last one

    double *sx = s_pt[wave][0], *sy = s_pt[wave][1];
    for (int s = blockIdx.x * KL_WAVES + wave; s < total; s += gridDim.x * KL_WAVES) {
        // the last row whose offset is <= s: rows without scans share their successor's offset and are passed over
        int lo = 0, hi = R.n_rows - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= s) lo = mid;
            else hi = mid - 1;
        }
        const kl_refresh_row r = R.rows[lo];
        const int j = s - s_off[lo];
        const size_t slot = (size_t)r.pool_first + j;
        const double *raw = R.ranges + slot * n;
        const double px = R.poses[3 * slot], py = R.poses[3 * slot + 1], ph = R.poses[3 * slot + 2];
        double sum = 0.0;  // lane 0: x; lane 1: y
        int cnt = 0;
        if (D.use_barycenter) {
            for (int c0 = 0; c0 < n; c0 += 64) {
                const int cn = min(64, n - c0), i = c0 + lane;
                bool ok = false;
                double x = 0.0, y = 0.0;
                if (lane < cn) {
                    const double rr = raw[i];
                    ok = rr >= D.minimum_range && rr <= D.range_threshold;  // math::InRange
                    if (ok) {
                        const double angle = ph + D.minimum_angle + (double)(unsigned)i * D.angular_resolution;
                        x = px + (rr * sdm_cos(angle));
                        y = py + (rr * sdm_sin(angle));
                    }
                }
                cnt += __popcll(__ballot(ok));
                sx[lane] = x;
                sy[lane] = y;
                kl_wave_sync();
                // +0.0 for an invalid reading, as in kl_reference_kernel: the sum's bits are the branching loop's
                if (lane < 2) {
                    const double *p = s_pt[wave][lane];
#pragma unroll 8
                    for (int k = 0; k < cn; ++k) sum = sum + p[k];
                }
                kl_wave_sync();
            }
        }
        const double sum_y = __shfl(sum, 1, 64);
        if (lane == 0) {
            double2 out;
            if (cnt > 0) {
                const double np = (double)cnt;
                out.x = sum / np;
                out.y = sum_y / np;
            } else {
                out.x = px;
                out.y = py;
            }
            D.ref[(size_t)r.graph * D.max_scans + r.first + j] = out;
        }
    }
}

// =================================================================================================
// kl_search_kernel
// =================================================================================================
// One traversal (BreadthFirstTraversal::Traverse, Mapper.h:568-612) by one wave.  pos[v]: KL_UNSEEN, the vertex's
// queue position (< N), or N + c while candidate c of the running batch claims it.  Returns the number of valid
// vertices written to near_out in visiting order.
__device__ inline int kl_traverse(int lane, int N, int n, int ne, int scan, int passbit, const int *__restrict__ adj_off,
                                  const int2 *__restrict__ adj, const unsigned char *flags, int *pos,
                                  unsigned short *qu, int *near_out)
{
    if (lane == 0) {
        qu[0] = (unsigned short)scan;
        pos[scan] = 0;
    }
    kl_wave_sync();
    int head = 0, tail = 1, nvalid = 0;
    while (head < tail) {
        const int batch = min(64, tail - head);
        int v = 0, deg = 0, a0 = 0;
        bool pass = false;
        if (lane < batch) {
            v = qu[head + lane];
            pass = (flags[v] & passbit) != 0;
        }
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            near_out[nvalid + __popcll(mask & ((1ull << lane) - 1ull))] = v;
            a0 = adj_off[v];
            deg = adj_off[v + 1] - a0;
        }
        nvalid += __popcll(mask);
        const int incl = kl_wave_inscan(deg, lane);
        const int base = N + incl - deg;
        if (__shfl(incl, 63, 64) > 0) {
            // the batch's expansions in (queue position, adjacency position) order claim their vertices
            for (int j = 0; j < deg; ++j) {
                const int2 e = adj[a0 + j];
                if (e.y < ne && e.x < n) atomicMin(&pos[e.x], base + j);
            }
            kl_wave_sync();
            int wins = 0;
            for (int j = 0; j < deg; ++j) {
                const int2 e = adj[a0 + j];
                wins += (e.y < ne && e.x < n && pos[e.x] == base + j) ? 1 : 0;
            }
            const int wincl = kl_wave_inscan(wins, lane);
            int r = tail + wincl - wins;
            for (int j = 0; j < deg; ++j) {
                const int2 e = adj[a0 + j];
                if (e.y < ne && e.x < n && pos[e.x] == base + j) {
                    qu[r] = (unsigned short)e.x;
                    pos[e.x] = r;
                    ++r;
                }
            }
            tail += __shfl(wincl, 63, 64);
        }
        head += batch;
        kl_wave_sync();
    }
    return nvalid;
}

// The maximal runs of is(i) over [lo, n): starts[k], ends[k] (inclusive) in LDS; returns their number.  Thread t
// owns the contiguous indices [t * chunk, (t + 1) * chunk), so both compactions keep the order and the k-th start
// pairs with the k-th end.
template <class Pred>
__device__ inline int kl_runs(int n, Pred is, unsigned short *starts, unsigned short *ends, int *sw)
{
    const int chunk = (n + KL_THREADS - 1) / KL_THREADS;
    const int i0 = min((int)threadIdx.x * chunk, n), i1 = min(i0 + chunk, n);
    int ns = 0, nend = 0;
    for (int i = i0; i < i1; ++i) {
        const bool a = is(i);
        ns += (a && !(i > 0 && is(i - 1))) ? 1 : 0;
        nend += (a && !(i + 1 < n && is(i + 1))) ? 1 : 0;
    }
    int total, total_e;
    int ks = kl_block_exscan(ns, sw, &total);
    int ke = kl_block_exscan(nend, sw, &total_e);
    for (int i = i0; i < i1; ++i) {
        const bool a = is(i);
        if (a && !(i > 0 && is(i - 1))) starts[ks++] = (unsigned short)i;
        if (a && !(i + 1 < n && is(i + 1))) ends[ke++] = (unsigned short)i;
    }
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(KL_THREADS)
kl_search_kernel(KlDev D, const kl_query *__restrict__ queries, int G)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char kl_smem[];
    __shared__ int sw[KL_WAVES];
    __shared__ int s_nvalid[2], s_acc[2];

    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = D.max_scans;
    const kl_query q = queries[slot];
    if (tid == 0) D.queries[slot] = q;
    kl_result res{};
    res.status = KL_EINVAL;
    int n = 0, ne = 0;
    bool ok = q.graph >= 0 && q.graph < G;
    if (ok) {
        const KlHdr h = D.hdr[q.graph];
        n = q.n_scans < 0 ? h.n_scans : q.n_scans;
        ne = q.n_edges < 0 ? h.n_edges : q.n_edges;
        ok = n <= h.n_scans && ne <= h.n_edges && h.n_scans <= N && q.scan >= 0 && q.scan < n && q.start_num >= 0;
    }
    if (!ok) {  // uniform over the workgroup
        if (tid == 0) D.res[slot] = res;
        return;
    }
    int *pos0 = reinterpret_cast<int *>(kl_smem);                         // [N] link traversal
    int *pos1 = pos0 + N;                                                 // [N] loop traversal
    unsigned short *qu0 = reinterpret_cast<unsigned short *>(pos1 + N + 2);  // [N]; pos1 has 2 ints of slack (step 4)
    unsigned short *qu1 = qu0 + N;                                        // [N]
    unsigned char *flags = reinterpret_cast<unsigned char *>(qu1 + N);    // [N]

    const double2 *ref = D.ref + (size_t)q.graph * N;
    const int *adj_off = D.adj_off + (size_t)q.graph * (N + 1);
    const int2 *adj = D.adj + (size_t)q.graph * 2 * D.max_edges;
    double *d2 = D.d2 + (size_t)slot * N;
    const double2 c = ref[q.scan];

    // 1. squared distances (Vector2::SquaredDistance, Karto.h:1011-1032) and the threshold bits
    for (int i = tid; i < n; i += KL_THREADS) {
        const double2 p = ref[i];
        const double dx = p.x - c.x, dy = p.y - c.y;
        const double d = dx * dx + dy * dy;
        d2[i] = d;
        flags[i] = (unsigned char)((d < D.link_hi ? KL_F_LINK_RANGE : 0) | (d < D.loop_hi ? KL_F_LOOP_RANGE : 0) |
                                   (d <= D.link_lo ? KL_F_LINK_VISIT : 0) | (d <= D.loop_lo ? KL_F_LOOP_VISIT : 0));
        pos0[i] = KL_UNSEEN;
        pos1[i] = KL_UNSEEN;
    }
    __syncthreads();

    // 2. the two traversals, one wave each
    if (wave < 2) {
        const int nv = kl_traverse(lane, N, n, ne, q.scan, wave ? KL_F_LOOP_VISIT : KL_F_LINK_VISIT, adj_off, adj, flags,
                                   wave ? pos1 : pos0, wave ? qu1 : qu0,
                                   (wave ? D.near_loop : D.near_link) + (size_t)slot * N);
        if (lane == 0) s_nvalid[wave] = nv;
    }
    __syncthreads();
    res.n_scans = n;
    res.n_near_link = s_nvalid[0];
    res.n_near_loop = s_nvalid[1];

    // 3. FindPossibleLoopClosure: runs of A = in range and not near-linked, over i >= start_num
    unsigned short *starts = qu0, *ends = qu0 + (N / 2 + 1);  // the queues' 2 N shorts
    {
        const int start = q.start_num;
        auto isA = [&](int i) {
            return i >= start && (flags[i] & KL_F_LOOP_RANGE) && !(pos1[i] != KL_UNSEEN && (flags[i] & KL_F_LOOP_VISIT));
        };
        const int K = kl_runs(n, isA, starts, ends, sw);
        const int chunk = (K + KL_THREADS - 1) / KL_THREADS;
        const int k0 = min(tid * chunk, K), k1 = min(k0 + chunk, K);
        int keep = 0, len = 0;
        for (int k = k0; k < k1; ++k) {
            const int b = starts[k], f = ends[k] + 1, l = f - b;
            // a run that reaches the end of the scans is returned at any length (:1393); one followed by an
            // out-of-range scan if it is long enough (:1381); one followed by a near-linked scan is cleared (:1367)
            if (f == n || (!(flags[f] & KL_F_LOOP_RANGE) && l >= D.min_chain)) {
                ++keep;
                len += l;
            }
        }
        int nchains, total_len;
        int r = kl_block_exscan(keep, sw, &nchains);
        kl_block_exscan(len, sw, &total_len);
        kl_loop_chain *out = D.loop_chains + (size_t)slot * D.chain_stride;
        for (int k = k0; k < k1; ++k) {
            const int b = starts[k], f = ends[k] + 1, l = f - b;
            if (f == n || (!(flags[f] & KL_F_LOOP_RANGE) && l >= D.min_chain)) out[r++] = kl_loop_chain{b, l, f, 0};
        }
        res.n_loop_chains = nchains;
        res.loop_index_total = total_len;
        __syncthreads();
    }

    // 4. FindNearChains: runs of R = d2 < link^2 + tol that hold a near-linked scan other than the query; the query's
    //    run is invalid.  pos1 is free now: runmin int[N / 2 + 1] | slot16 uint16[N]
    {
        auto isR = [&](int i) { return (flags[i] & KL_F_LINK_RANGE) != 0; };
        const int K = kl_runs(n, isR, starts, ends, sw);
        int *runmin = pos1;
        unsigned short *slot16 = reinterpret_cast<unsigned short *>(pos1 + (N / 2 + 1));
        const int tail = [&] {  // queue length of the link traversal: the seen vertices
            int cnt = 0;
            for (int i = tid; i < n; i += KL_THREADS) cnt += pos0[i] != KL_UNSEEN ? 1 : 0;
            int total;
            kl_block_exscan(cnt, sw, &total);
            return total;
        }();
        for (int k = tid; k < K; k += KL_THREADS) runmin[k] = KL_UNSEEN;
        for (int p = tid; p < tail; p += KL_THREADS) slot16[p] = 0xFFFF;
        if (tid == 0) s_acc[0] = s_acc[1] = 0;
        __syncthreads();
        auto run_of = [&](int v) {  // the largest k with starts[k] <= v
            int lo = 0, hi = K - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int)starts[mid] <= v) lo = mid;
                else hi = mid - 1;
            }
            return lo;
        };
        for (int v = tid; v < n; v += KL_THREADS)
            if (v != q.scan && pos0[v] != KL_UNSEEN && (flags[v] & KL_F_LINK_VISIT) && isR(v))
                atomicMin(&runmin[run_of(v)], pos0[v]);
        __syncthreads();
        const int kq = isR(q.scan) ? run_of(q.scan) : -1;
        for (int k = tid; k < K; k += KL_THREADS)
            if (k != kq && runmin[k] != KL_UNSEEN) slot16[runmin[k]] = (unsigned short)k;
        __syncthreads();
        // the chains in the order of their first near-linked member's queue position
        const int chunk = (tail + KL_THREADS - 1) / KL_THREADS;
        const int p0 = min(tid * chunk, tail), p1 = min(p0 + chunk, tail);
        int cnt = 0;
        for (int p = p0; p < p1; ++p) cnt += slot16[p] != 0xFFFF ? 1 : 0;
        int nchains;
        int r = kl_block_exscan(cnt, sw, &nchains);
        kl_near_chain *out = D.near_chains + (size_t)slot * D.chain_stride;
        for (int p = p0; p < p1; ++p)
            if (slot16[p] != 0xFFFF) {
                const int k = slot16[p], b = starts[k], l = ends[k] + 1 - b;
                out[r++] = kl_near_chain{b, l, -1, l >= D.min_chain ? KL_CHAIN_LONG : 0};
            }
        __syncthreads();
        // GetClosestScanToPose (strict <: the first minimum) and LinkChainToScan's test, one wave per chain
        for (int ch = wave; ch < nchains; ch += KL_WAVES) {
            const int b = out[ch].begin, l = out[ch].length;
            double best = DBL_MAX;
            int bi = INT_MAX;
            for (int i = b + lane; i < b + l; i += 64) {
                const double d = d2[i];
                if (d < best) {
                    best = d;
                    bi = i;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double od = __shfl_xor(best, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (od < best || (od == best && oi < bi)) {
                    best = od;
                    bi = oi;
                }
            }
            if (lane == 0) {
                const int fl = out[ch].flags | ((bi != INT_MAX && best < D.link_hi) ? KL_CHAIN_LINKED : 0);
                out[ch].closest = bi != INT_MAX ? bi : -1;
                out[ch].flags = fl;
                if (fl & KL_CHAIN_LONG) {
                    atomicAdd(&s_acc[0], 1);
                    atomicAdd(&s_acc[1], l);
                }
            }
        }
        __syncthreads();
        res.n_near_chains = nchains;
        res.n_near_long = s_acc[0];
        res.near_index_total = s_acc[1];
    }
    res.status = KL_OK;
    if (tid == 0) D.res[slot] = res;
}

// =================================================================================================
// kl_closest_kernel: one wave per item
// =================================================================================================
__global__ void __launch_bounds__(64)
kl_closest_kernel(KlDev D, const kl_closest_item *__restrict__ items, kl_closest *__restrict__ out, int G)
{
    const int it = blockIdx.x, lane = threadIdx.x;
    const kl_closest_item q = items[it];
    kl_closest res{-1, 0};
    bool ok = q.graph >= 0 && q.graph < G;
    if (ok) {
        const KlHdr h = D.hdr[q.graph];
        ok = h.n_scans <= D.max_scans && q.scan >= 0 && q.scan < h.n_scans && q.begin >= 0 && q.length >= 1 &&
             q.begin < h.n_scans && q.length <= h.n_scans - q.begin;
    }
    if (ok) {
        const double2 *ref = D.ref + (size_t)q.graph * D.max_scans;
        const double2 c = ref[q.scan];
        double best = DBL_MAX;
        int bi = INT_MAX;
        for (int i = q.begin + lane; i < q.begin + q.length; i += 64) {
            const double2 p = ref[i];
            const double dx = c.x - p.x, dy = c.y - p.y;
            const double d = dx * dx + dy * dy;
            if (d < best) {
                best = d;
                bi = i;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < best || (od == best && oi < bi)) {
                best = od;
                bi = oi;
            }
        }
        if (bi != INT_MAX) {
            res.closest = bi;
            res.linked = best < D.link_hi ? 1 : 0;
        }
    }
    if (lane == 0) out[it] = res;
}

// =================================================================================================
// kl_emit_scan_kernel (one workgroup) and kl_emit_write_kernel (one workgroup per slot)
// =================================================================================================
__global__ void __launch_bounds__(KL_THREADS)
kl_emit_scan_kernel(KlDev D, int count, int which, int capacity, int *__restrict__ base_begin, int *__restrict__ n_matches)
{
    __shared__ int sw[KL_WAVES];
    const int tid = threadIdx.x;
    int run_m = 0, run_i = 0;
    for (int s0 = 0; s0 < count; s0 += KL_THREADS) {
        const int s = s0 + tid;
        int m = 0, ix = 0;
        if (s < count && D.res[s].status == KL_OK) {
            m = which == KL_NEAR_CHAINS ? D.res[s].n_near_long : D.res[s].n_loop_chains;
            ix = which == KL_NEAR_CHAINS ? D.res[s].near_index_total : D.res[s].loop_index_total;
        }
        int tm, ti;
        const int em = kl_block_exscan(m, sw, &tm);
        const int ei = kl_block_exscan(ix, sw, &ti);
        if (s < count) D.emit_off[s] = make_int2(run_m + em, run_i + ei);
        run_m += tm;
        run_i += ti;
    }
    if (tid == 0) {
        D.emit_off[count] = make_int2(run_m, run_i);
        D.emit_info[0] = run_m;
        D.emit_info[1] = run_m > capacity ? KL_EMIT_OVERFLOW : 0;
        *n_matches = min(run_m, capacity);
        base_begin[0] = 0;
    }
}

__global__ void __launch_bounds__(KL_THREADS)
kl_emit_write_kernel(KlDev D, int which, int capacity, int *__restrict__ query_out, int *__restrict__ base_begin,
                     int *__restrict__ base_index, kl_source *__restrict__ source)
{
    __shared__ int sw[KL_WAVES];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const kl_result res = D.res[slot];
    if (res.status != KL_OK) return;
    const int2 off = D.emit_off[slot];
    const kl_query q = D.queries[slot];
    const int pool = D.hdr[q.graph].pool_offset;
    const int nch = which == KL_NEAR_CHAINS ? res.n_near_chains : res.n_loop_chains;
    const kl_loop_chain *lc = D.loop_chains + (size_t)slot * D.chain_stride;
    const kl_near_chain *nc = D.near_chains + (size_t)slot * D.chain_stride;
    // this slot's chains in chain order; thread t owns a contiguous piece of them
    const int chunk = (nch + KL_THREADS - 1) / KL_THREADS;
    const int c0 = min(tid * chunk, nch), c1 = min(c0 + chunk, nch);
    int m = 0, ix = 0;
    for (int c = c0; c < c1; ++c) {
        const bool keep = which == KL_NEAR_CHAINS ? (nc[c].flags & KL_CHAIN_LONG) != 0 : true;
        if (keep) {
            ++m;
            ix += which == KL_NEAR_CHAINS ? nc[c].length : lc[c].length;
        }
    }
    int tm, ti;
    int mi = off.x + kl_block_exscan(m, sw, &tm);
    int ii = off.y + kl_block_exscan(ix, sw, &ti);
    for (int c = c0; c < c1; ++c) {
        const bool keep = which == KL_NEAR_CHAINS ? (nc[c].flags & KL_CHAIN_LONG) != 0 : true;
        if (!keep) continue;
        const int b = which == KL_NEAR_CHAINS ? nc[c].begin : lc[c].begin;
        const int l = which == KL_NEAR_CHAINS ? nc[c].length : lc[c].length;
        if (mi < capacity) {
            query_out[mi] = pool + q.scan;
            source[mi] = kl_source{slot, c};
            base_begin[mi + 1] = ii + l;
            for (int j = 0; j < l; ++j) base_index[ii + j] = pool + b + j;
        }
        ++mi;
        ii += l;
    }
}

// =================================================================================================
// kl_edit_vertices_kernel / kl_edit_edges_kernel: AddVertex and AddEdge on the device (graph_edit_device.h: one
// workgroup per row, the first row of a graph leads it).  Wave 0 of the leader applies the graph's rows in row order;
// AddEdge's lookup runs over the source's adjacency as uploaded or rebuilt (all 64 lanes: an entry (other end, e)
// matches when ends[e].y is the target) and over the edges this call has appended so far.  Then all lanes rebuild the
// adjacency from the edge list by a stable bucket fill over the 2m edge ends, which is KlGraph::compile()'s order.
// LDS of the edges kernel: (max_scans + 1 + GE_THREADS + GE_WAVES + 1) ints.
// =================================================================================================
struct KlEdit {
    KlHdr *hdr;
    int *adj_off;
    int2 *adj;
    int2 *ends;                // [G][max_edges]: source, target, in insertion order
    unsigned long long *info;  // ge_refuse
    int max_scans, max_edges, G;
    unsigned seq;
};

__global__ void __launch_bounds__(GE_THREADS)
kl_edit_vertices_kernel(KlEdit E, int count, const int *__restrict__ graph, const int *__restrict__ expect,
                        int *__restrict__ id_out, int *__restrict__ status_out)
{
    const int row = blockIdx.x, lane = threadIdx.x & 63;
    const int g = graph[row];
    if (g < 0 || g >= E.G) {
        if (threadIdx.x == 0) {
            if (id_out) id_out[row] = -1;
            if (status_out) status_out[row] = g < 0 ? KL_OK : KL_EINVAL;
            if (g >= 0) ge_refuse(E.info, E.seq, row, KL_EINVAL);
        }
        return;
    }
    if (!ge_is_leader(graph, sizeof(int), row, g)) return;
    if (threadIdx.x >= 64) return;  // wave 0 alone from here: no workgroup barrier below
    const int n0 = E.hdr[g].n_scans;
    int n = n0;
    for (int base = row; base < count; base += 64) {
        const int j = base + lane;
        unsigned long long mask = __ballot(j < count && graph[j] == g);
        while (mask) {
            const int r = base + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int ex = expect ? expect[r] : -1;
            int st = KL_OK, id = -1;
            if (ex >= 0 && ex != n) st = KL_EINVAL;
            else if (n >= E.max_scans) st = KL_ERANGE;
            else id = n++;
            if (lane == 0) {
                if (id_out) id_out[r] = id;
                if (status_out) status_out[r] = st;
                if (st != KL_OK) ge_refuse(E.info, E.seq, r, st);
            }
        }
    }
    if (n == n0) return;
    int *off = E.adj_off + (size_t)g * (E.max_scans + 1);
    const int end = n0 > 0 ? off[n0] : 0;  // a graph never uploaded has no offset yet
    for (int k = (n0 > 0 ? n0 + 1 : 0) + lane; k <= n; k += 64) off[k] = end;
    if (lane == 0) E.hdr[g].n_scans = n;
}

__global__ void __launch_bounds__(GE_THREADS)
kl_edit_edges_kernel(KlEdit E, int count, const kl_edge_row *__restrict__ rows, int *__restrict__ is_new_out,
                     int *__restrict__ status_out)
{
    extern __shared__ int kl_edit_smem[];
    int *cur = kl_edit_smem, *s_b = cur + E.max_scans + 1, *sw = s_b + GE_THREADS, *s_m = sw + GE_WAVES;
    const int row = blockIdx.x, lane = threadIdx.x & 63;
    const int g = rows[row].graph;
    if (g < 0 || g >= E.G) {
        if (threadIdx.x == 0) {
            if (is_new_out) is_new_out[row] = 0;
            if (status_out) status_out[row] = g < 0 ? KL_OK : KL_EINVAL;
            if (g >= 0) ge_refuse(E.info, E.seq, row, KL_EINVAL);
        }
        return;
    }
    if (!ge_is_leader(rows, sizeof(kl_edge_row), row, g)) return;
    const KlHdr h = E.hdr[g];
    const int n = h.n_scans, m0 = h.n_edges;
    int *off = E.adj_off + (size_t)g * (E.max_scans + 1);
    int2 *adj = E.adj + (size_t)g * 2 * E.max_edges;
    int2 *ends = E.ends + (size_t)g * E.max_edges;
    if (threadIdx.x < 64) {
        int m = m0;
        for (int base = row; base < count; base += 64) {
            const int j = base + lane;
            unsigned long long mask = __ballot(j < count && rows[j].graph == g);
            while (mask) {
                const int r = base + __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int s = rows[r].source, t = rows[r].target;
                int st = KL_OK, nw = 0;
                if (s < 0 || s >= n || t < 0 || t >= n || s == t) {
                    st = KL_EINVAL;
                } else {
                    int found = 0;
                    const int a1 = off[s + 1];
                    for (int k = off[s] + lane; k < a1; k += 64) found |= ends[adj[k].y].y == t;
                    for (int e = m0 + lane; e < m; e += 64) {
                        const int2 ee = ends[e];
                        found |= ee.x == s && ee.y == t;
                    }
                    if (__ballot(found) == 0) {
                        if (m >= E.max_edges) {
                            st = KL_ERANGE;
                        } else {
                            if (lane == 0) ends[m] = make_int2(s, t);
                            ++m;
                            nw = 1;
                            ge_fence();
                        }
                    }
                }
                if (lane == 0) {
                    if (is_new_out) is_new_out[r] = nw;
                    if (status_out) status_out[r] = st;
                    if (st != KL_OK) ge_refuse(E.info, E.seq, r, st);
                }
            }
        }
        if (lane == 0) *s_m = m;
    }
    __threadfence_block();
    __syncthreads();
    const int m = *s_m;
    if (m == m0) return;
    ge_bucket_fill(
        n, 2 * m, cur, s_b, sw, off,
        [&](int x) {
            const int2 e = ends[x >> 1];
            return (x & 1) ? e.y : e.x;
        },
        [&](int x, int pos) {
            const int2 e = ends[x >> 1];
            adj[pos] = make_int2((x & 1) ? e.x : e.y, x >> 1);
        });
    if (threadIdx.x == 0) E.hdr[g].n_edges = m;
}

}  // namespace s2d
