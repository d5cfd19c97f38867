// karto_link_kernels.hip -- HIP kernels of the Karto graph-linking stage (gfx950).
//
// Reference: MapperGraph::AddEdges, TryCloseLoop's tests, LinkScans / LinkInfo, SpaSolver::AddConstraint's precision
// matrix and ComputeWeightedMean (lesson6/lib/open_karto; the C-ABI and the arithmetic, operation by operation, are
// in include/slam2d/karto_link.h).
//   ke_add_edges_kernel     one wave per AddEdges job, four jobs per workgroup, wave-level operations only (no
//                           workgroup barrier: the jobs of a workgroup are independent).  Lane i prepares item i of a
//                           batch of 64: a near match's link record (rotation, the two 3 x 3 products, the inverse,
//                           the pose difference), its position in the row by a ballot prefix count; then a mean-list
//                           item's inverse.  The ordered sums of ComputeWeightedMean are taken by every lane alike from
//                           the items' values in list order (one lane's value at a time, by a wave shuffle), so the
//                           bits do not depend on the schedule.  The item's inverse is computed twice (before and after
//                           the inverse of the sum is known) rather than kept: the same operations give the same bits.
//   ke_coarse_scan_kernel   one workgroup: TryCloseLoop's coarse test per match and an order-preserving compaction
//                           (a workgroup prefix sum over 256 matches at a time) into the fine batch's arrays.
//   ke_coarse_write_kernel  one workgroup per tmp row: the query scan's ranges, the coarse mean, the base list.
//   ke_fine_kernel          one lane per search slot: the slot's first fine match that is not rejected.
//   ke_close_kernel         one lane per slot: the KE_LOOP record.
// All arithmetic is double with -ffp-contract=off and detmath.h's sin / cos / atan2; no atomics anywhere.  This stage
// is latency-bound (a few hundred dependent double operations per job and a few hundred bytes of traffic).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/slam2d/karto_link.h"
#include "detmath.h"
#include "karto_pose_math.h"

namespace s2d {

constexpr int KE_THREADS = 256;
constexpr int KE_JOBS_PER_BLOCK = KE_THREADS / 64;

// LinkInfo::Update (Mapper.h:138-152) and AddConstraint's precision matrix (spa_solver.cc:81-88)
KE_FN int ke_link_info(const double *pose1, const double *pose2, const double *cov, double *diff, double *prec)
{
    // Transform transform(rPose1, Pose2()): SetTransform (Karto.h:2909-2935)
    double rot[9], tr[3];
    if (pose1[0] == 0.0 && pose1[1] == 0.0 && pose1[2] == 0.0) {
        for (int k = 0; k < 9; ++k) rot[k] = (k % 4 == 0) ? 1.0 : 0.0;
        tr[0] = tr[1] = tr[2] = 0.0;
    } else {
        ke_from_axis_angle(0.0, 0.0, 1.0, 0.0 - pose1[2], rot);
        if (pose1[0] != 0.0 || pose1[1] != 0.0) {
            double rp[3];
            ke_mul_pose(rot, pose1, rp);
            tr[0] = 0.0 - rp[0];
            tr[1] = 0.0 - rp[1];
        } else {
            tr[0] = 0.0;
            tr[1] = 0.0;
        }
        tr[2] = 0.0 - pose1[2];
    }
    // TransformPose (Karto.h:2881-2887)
    double rp2[3];
    ke_mul_pose(rot, pose2, rp2);
    const double dx = tr[0] + rp2[0], dy = tr[1] + rp2[1];
    const double dh = ke_normalize_angle(pose2[2] + tr[2]);
    // rotationMatrix * rCovariance * rotationMatrix.Transpose()
    double r1[9], r1t[9], a[9], c[9];
    ke_from_axis_angle(0.0, 0.0, 1.0, -pose1[2], r1);
    for (int row = 0; row < 3; ++row)
        for (int col = 0; col < 3; ++col) r1t[3 * row + col] = r1[3 * col + row];
    ke_mul(r1, cov, a);
    ke_mul(a, r1t, c);
    double p[9];
    if (!ke_inverse(c, p)) {
        for (int k = 0; k < 3; ++k) diff[k] = 0.0;
        for (int k = 0; k < 9; ++k) prec[k] = 0.0;
        return KE_SINGULAR;
    }
    p[3] = p[1];
    p[6] = p[2];
    p[7] = p[5];
    diff[0] = dx;
    diff[1] = dy;
    diff[2] = dh;
    for (int k = 0; k < 9; ++k) prec[k] = p[k];
    return KE_OK;
}

// LinkScans' record: the from-scan's sensor pose is read from the pool
__device__ static inline void ke_emit_link(ke_link *rec, int from, int to, int kind, const double *from_pose,
                                           const double *mean, const double *cov)
{
    double p1[3] = {from_pose[0], from_pose[1], from_pose[2]};
    ke_link r;
    r.from = from;
    r.to = to;
    r.kind = kind;
    r.status = ke_link_info(p1, mean, cov, r.diff, r.precision);
    *rec = r;
}

struct KeAddArgs {
    int count, max_links, pool_scans, n_seq, n_running, n_near, chain_stride, n_slots, flags, pad_;
    double link_threshold;  // link_match_minimum_response_fine - KL_TOLERANCE
    const ke_job *jobs;
    double *pool_poses;
    const kt_result *seq;
    const kl_closest *running;
    const kt_result *near;
    const kl_source *near_source;
    const kl_near_chain *near_chains;
    ke_link *links;
    ke_job_out *out;
};

// a near match of the job: 0 not accepted, 1 accepted (joins the mean list), 2 accepted and its chain linked (*from
// = the chain's closest scan), 3 an index out of range
__device__ static inline int ke_near_state(const KeAddArgs &a, const ke_job &jb, int k, int *from)
{
    const int m = jb.near_first + k;
    if (!(a.near[m].response > a.link_threshold)) return 0;
    const kl_source src = a.near_source[m];
    if (src.slot < 0 || src.slot >= a.n_slots || src.chain < 0 || src.chain >= a.chain_stride) return 3;
    const kl_near_chain ch = a.near_chains[(size_t)src.slot * a.chain_stride + src.chain];
    if (!(ch.flags & KL_CHAIN_LINKED)) return 1;
    if (ch.closest < 0 || (long long)jb.pool_offset + ch.closest >= a.pool_scans) return 3;
    *from = ch.closest;
    return 2;
}

__global__ void __launch_bounds__(KE_THREADS) ke_add_edges_kernel(KeAddArgs a)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * KE_JOBS_PER_BLOCK + (threadIdx.x >> 6);
    if (j >= a.count) return;  // the whole wave
    const ke_job jb = a.jobs[j];
    ke_job_out o;
    o.n_links = o.n_means = 0;
    o.status = KE_OK;
    o.graph = jb.graph;
    o.pose[0] = o.pose[1] = o.pose[2] = 0.0;
    const long long slot = (long long)jb.pool_offset + jb.scan;
    if (jb.scan < 0 || jb.pool_offset < 0 || slot >= a.pool_scans) {
        o.status = KE_EINVAL;
        if (lane == 0) a.out[j] = o;
        return;
    }
    double pose[3];
    for (int k = 0; k < 3; ++k) o.pose[k] = pose[k] = a.pool_poses[slot * 3 + k];
    const bool has_prev = jb.prev >= 0;
    bool bad = jb.running < -1 || jb.running >= a.n_running || jb.near_count < 0 || jb.near_first < 0 ||
               (long long)jb.near_first + jb.near_count > a.n_near;
    if (has_prev)
        bad = bad || (long long)jb.pool_offset + jb.prev >= a.pool_scans || jb.seq_result < 0 || jb.seq_result >= a.n_seq;
    // the running scans are linked only where a previous scan exists (AddEdges' else branch, Mapper.cpp:955-963)
    int run_from = -1;
    if (!bad && has_prev && jb.running >= 0) {
        const kl_closest rc = a.running[jb.running];
        if (rc.linked) {
            run_from = rc.closest;
            if (run_from < 0 || (long long)jb.pool_offset + run_from >= a.pool_scans) bad = true;
        }
    }
    // the records the job needs
    int n_links = (has_prev ? 1 : 0) + (run_from >= 0 ? 1 : 0);
    if (!bad) {
        for (int base = 0; base < jb.near_count; base += 64) {
            const int k = base + lane;
            int from = -1;
            const int st = k < jb.near_count ? ke_near_state(a, jb, k, &from) : 0;
            if (__ballot(st == 3) != 0) bad = true;
            n_links += __popcll(__ballot(st == 2));
        }
    }
    if (bad || n_links > a.max_links) {
        o.status = bad ? KE_EINVAL : KE_ERANGE;
        if (lane == 0) a.out[j] = o;
        return;
    }
    o.n_links = n_links;

    // rCovariance
    double rcov[9];
    for (int k = 0; k < 9; ++k) rcov[k] = has_prev ? a.seq[jb.seq_result].covariance[k] : 0.0;
    ke_link *row = a.links + (size_t)j * a.max_links;
    const double *pool = a.pool_poses;
    if (lane == 0 && has_prev)
        ke_emit_link(row, jb.prev, jb.scan, KE_PREV, pool + ((long long)jb.pool_offset + jb.prev) * 3, pose, rcov);
    if (lane == 1 && run_from >= 0)
        ke_emit_link(row + 1, run_from, jb.scan, KE_RUNNING, pool + ((long long)jb.pool_offset + run_from) * 3, pose, rcov);
    int idx = (has_prev ? 1 : 0) + (run_from >= 0 ? 1 : 0);
    for (int base = 0; base < jb.near_count; base += 64) {
        const int k = base + lane;
        int from = -1;
        const int st = k < jb.near_count ? ke_near_state(a, jb, k, &from) : 0;
        const unsigned long long mask = __ballot(st == 2);
        if (st == 2) {
            const int at = idx + __popcll(mask & ((1ull << lane) - 1ull));
            const kt_result *r = a.near + jb.near_first + k;
            double mean[3], cov[9];
            for (int e = 0; e < 3; ++e) mean[e] = r->mean[e];
            for (int e = 0; e < 9; ++e) cov[e] = r->covariance[e];
            ke_emit_link(row + at, from, jb.scan, KE_NEAR, pool + ((long long)jb.pool_offset + from) * 3, mean, cov);
        }
        idx += __popcll(mask);
    }

    // ComputeWeightedMean over [scanPose, rCov] (when a previous scan exists), then the accepted near matches
    const int head = has_prev ? 1 : 0;
    const int items = head + jb.near_count;
    double sum[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n_means = 0;
    bool singular = false;
    for (int base = 0; base < items; base += 64) {
        const int t = base + lane;
        int act = 0, sing = 0;
        double inv[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (t < items) {
            const double *cov = rcov;
            act = 1;
            if (t >= head) {
                const kt_result *r = a.near + jb.near_first + (t - head);
                act = r->response > a.link_threshold ? 1 : 0;
                cov = r->covariance;
            }
            if (act) {
                double c[9];
                for (int e = 0; e < 9; ++e) c[e] = cov[e];
                sing = ke_inverse(c, inv) ? 0 : 1;
            }
        }
        const int lim = min(64, items - base);
        for (int i = 0; i < lim; ++i) {
            const int ai = __shfl(act, i);
            const int si = __shfl(sing, i);
            double v[9];
            for (int e = 0; e < 9; ++e) v[e] = __shfl(inv[e], i);
            if (ai) {
                for (int e = 0; e < 9; ++e) sum[e] += v[e];
                n_means += 1;
                singular = singular || si != 0;
            }
        }
    }
    o.n_means = n_means;
    double inv_sum[9];
    if (n_means > 0 && !singular) singular = !ke_inverse(sum, inv_sum);
    if (n_means == 0 || singular) {
        if (singular) o.status = KE_SINGULAR;
        if (lane == 0) a.out[j] = o;
        return;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    double thetaX = 0.0, thetaY = 0.0;
    for (int base = 0; base < items; base += 64) {
        const int t = base + lane;
        int act = 0;
        double wp[3] = {0.0, 0.0, 0.0}, cs = 0.0, sn = 0.0;
        if (t < items) {
            const double *cov = rcov;
            double mean[3] = {pose[0], pose[1], pose[2]};
            act = 1;
            if (t >= head) {
                const kt_result *r = a.near + jb.near_first + (t - head);
                act = r->response > a.link_threshold ? 1 : 0;
                cov = r->covariance;
                for (int e = 0; e < 3; ++e) mean[e] = r->mean[e];
            }
            if (act) {
                double c[9], inv[9], weight[9];
                for (int e = 0; e < 9; ++e) c[e] = cov[e];
                ke_inverse(c, inv);
                cs = sdm_cos(mean[2]);
                sn = sdm_sin(mean[2]);
                ke_mul(inv_sum, inv, weight);
                ke_mul_pose(weight, mean, wp);
            }
        }
        const int lim = min(64, items - base);
        for (int i = 0; i < lim; ++i) {
            const int ai = __shfl(act, i);
            const double ci = __shfl(cs, i), si = __shfl(sn, i);
            const double w0 = __shfl(wp[0], i), w1 = __shfl(wp[1], i), w2 = __shfl(wp[2], i);
            if (ai) {
                thetaX += ci;
                thetaY += si;
                // Pose2::operator+= (Karto.h:2117-2121)
                acc[0] += w0;
                acc[1] += w1;
                acc[2] = ke_normalize_angle(acc[2] + w2);
            }
        }
    }
    thetaX /= (double)n_means;
    thetaY /= (double)n_means;
    o.pose[0] = acc[0];
    o.pose[1] = acc[1];
    o.pose[2] = sdm_atan2(thetaY, thetaX);
    if (lane == 0) {
        a.out[j] = o;
        if (a.flags & KE_WRITE_POSE)
            for (int k = 0; k < 3; ++k) a.pool_poses[slot * 3 + k] = o.pose[k];
    }
}

struct KeCoarseArgs {
    int max_matches, pool_scans, tmp_first, capacity, base_capacity, n_readings;
    double min_coarse, max_var;
    const int *n_matches;
    const kt_result *coarse;
    const int *query, *base_begin, *base_index;
    const double *pool_ranges;
    int *fine_query, *fine_base_begin, *fine_base_index, *fine_of, *n_fine;
    double *tmp_ranges, *tmp_poses;
    int *info;  // [2]: accepted before the cut, status bits
};

__global__ void __launch_bounds__(KE_THREADS) ke_coarse_scan_kernel(KeCoarseArgs a)
{
    __shared__ int s_acc[KE_THREADS];
    __shared__ long long s_len[KE_THREADS];
    __shared__ int s_einval;
    const int tid = threadIdx.x;
    const int n = max(0, min(*a.n_matches, a.max_matches));
    if (tid == 0) s_einval = 0;
    __syncthreads();
    int accepted = 0, kept = 0;  // the same in every thread
    long long base_sum = 0;
    for (int base = 0; base < n; base += KE_THREADS) {
        const int m = base + tid;
        int acc = 0;
        long long len = 0;
        if (m < n) {
            const kt_result *r = a.coarse + m;
            if (r->response > a.min_coarse && r->covariance[0] < a.max_var && r->covariance[4] < a.max_var) {
                const int q = a.query[m], b0 = a.base_begin[m], b1 = a.base_begin[m + 1];
                if (q < 0 || q >= a.pool_scans || b0 < 0 || b1 < b0) {
                    s_einval = 1;
                } else {
                    acc = 1;
                    len = b1 - b0;
                }
            }
        }
        s_acc[tid] = acc;
        s_len[tid] = len;
        __syncthreads();
        for (int d = 1; d < KE_THREADS; d <<= 1) {  // inclusive prefix sums
            const int pa = tid >= d ? s_acc[tid - d] : 0;
            const long long pl = tid >= d ? s_len[tid - d] : 0;
            __syncthreads();
            s_acc[tid] += pa;
            s_len[tid] += pl;
            __syncthreads();
        }
        const int f = accepted + s_acc[tid] - acc;
        const long long begin = base_sum + s_len[tid] - len;
        // f and begin + len do not decrease along the matches: the kept matches are the first of the accepted ones
        const int keep = acc && f < a.capacity && begin + len <= a.base_capacity;
        if (keep) {
            a.fine_query[f] = a.tmp_first + f;
            a.fine_of[f] = m;
            a.fine_base_begin[f] = (int)begin;
            a.fine_base_begin[f + 1] = (int)(begin + len);
        }
        const int tot_acc = s_acc[KE_THREADS - 1];
        const long long tot_len = s_len[KE_THREADS - 1];
        __syncthreads();
        s_acc[tid] = keep;
        __syncthreads();
        for (int d = KE_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) s_acc[tid] += s_acc[tid + d];
            __syncthreads();
        }
        kept += s_acc[0];
        accepted += tot_acc;
        base_sum += tot_len;
        __syncthreads();
    }
    if (tid == 0) {
        if (kept == 0) a.fine_base_begin[0] = 0;
        *a.n_fine = kept;
        a.info[0] = accepted;
        a.info[1] = (kept < accepted ? KE_LOOP_OVERFLOW : 0) | (s_einval ? KE_LOOP_EINVAL : 0);
    }
}

__global__ void __launch_bounds__(KE_THREADS) ke_coarse_write_kernel(KeCoarseArgs a)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    const int nf = *a.n_fine;
    double *ranges = a.tmp_ranges + (size_t)f * a.n_readings;
    double *pose = a.tmp_poses + (size_t)f * 3;
    if (f >= nf) {  // an unused row: a scan with no valid reading at the origin
        for (int i = tid; i < a.n_readings; i += KE_THREADS) ranges[i] = __builtin_inf();
        if (tid < 3) pose[tid] = 0.0;
        return;
    }
    const int m = a.fine_of[f];
    const double *src = a.pool_ranges + (size_t)a.query[m] * a.n_readings;
    for (int i = tid; i < a.n_readings; i += KE_THREADS) ranges[i] = src[i];
    if (tid < 3) pose[tid] = a.coarse[m].mean[tid];
    const int b0 = a.base_begin[m], len = a.base_begin[m + 1] - b0, out0 = a.fine_base_begin[f];
    for (int i = tid; i < len; i += KE_THREADS) a.fine_base_index[out0 + i] = a.base_index[b0 + i];
}

struct KeFineArgs {
    int count, capacity, max_matches, chain_stride, pool_scans, flags;
    double min_fine;
    const int *n_fine;
    const kt_result *fine;
    const int *fine_of;
    const kl_source *source;
    const int *query;
    const kl_loop_chain *loop_chains;
    ke_closure *closures;
    double *pool_poses;
};

// the search slot of fine match f, or INT_MAX when its coarse match is out of range
__device__ static inline int ke_fine_slot(const KeFineArgs &a, int f)
{
    const int m = a.fine_of[f];
    return (m < 0 || m >= a.max_matches) ? INT_MAX : a.source[m].slot;
}

__global__ void __launch_bounds__(64) ke_fine_kernel(KeFineArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.count) return;
    const int nf = max(0, min(*a.n_fine, a.capacity));
    ke_closure c;
    c.chain = c.resume = c.fine = -1;
    c.pad_ = 0;
    for (int k = 0; k < 3; ++k) c.pose[k] = 0.0;
    for (int k = 0; k < 9; ++k) c.covariance[k] = 0.0;
    int lo = 0, hi = nf;  // the slot's first fine match: the matches are ordered by slot
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (ke_fine_slot(a, mid) < s) lo = mid + 1;
        else hi = mid;
    }
    for (int f = lo; f < nf && ke_fine_slot(a, f) == s; ++f) {
        const kt_result *r = a.fine + f;
        if (r->response < a.min_fine) continue;  // REJECTED (Mapper.cpp:1023); a NaN response is not
        const int m = a.fine_of[f];
        const int chain = a.source[m].chain;
        if (chain < 0 || chain >= a.chain_stride) continue;
        c.chain = chain;
        c.resume = a.loop_chains[(size_t)s * a.chain_stride + chain].resume;
        c.fine = f;
        for (int k = 0; k < 3; ++k) c.pose[k] = r->mean[k];
        for (int k = 0; k < 9; ++k) c.covariance[k] = r->covariance[k];
        if (a.flags & KE_WRITE_POSE) {
            const int q = a.query[m];
            if (q >= 0 && q < a.pool_scans)
                for (int k = 0; k < 3; ++k) a.pool_poses[(size_t)q * 3 + k] = c.pose[k];
        }
        break;
    }
    a.closures[s] = c;
}

__global__ void __launch_bounds__(64) ke_close_kernel(int count, int max_links, int pool_scans, const ke_job *jobs,
                                                      const ke_closure *closures, const kl_closest *closest,
                                                      const double *pool_poses, ke_link *links, ke_job_out *out)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= count) return;
    const ke_job jb = jobs[s];
    ke_job_out o;
    o.n_links = o.n_means = 0;
    o.status = KE_OK;
    o.graph = jb.graph;
    o.pose[0] = o.pose[1] = o.pose[2] = 0.0;
    const long long slot = (long long)jb.pool_offset + jb.scan;
    if (jb.scan < 0 || jb.pool_offset < 0 || slot >= pool_scans) {
        o.status = KE_EINVAL;
        out[s] = o;
        return;
    }
    const ke_closure c = closures[s];
    for (int k = 0; k < 3; ++k) o.pose[k] = c.chain >= 0 ? c.pose[k] : pool_poses[slot * 3 + k];
    if (c.chain >= 0) {
        const kl_closest cl = closest[s];
        if (cl.linked) {
            if (cl.closest < 0 || (long long)jb.pool_offset + cl.closest >= pool_scans) {
                o.status = KE_EINVAL;
            } else {
                ke_emit_link(links + (size_t)s * max_links, cl.closest, jb.scan, KE_LOOP,
                             pool_poses + ((long long)jb.pool_offset + cl.closest) * 3, c.pose, c.covariance);
                o.n_links = 1;
            }
        }
    }
    out[s] = o;
}

}  // namespace s2d
