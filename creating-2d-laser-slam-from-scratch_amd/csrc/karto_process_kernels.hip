// karto_process_kernels.hip -- HIP kernels of the Karto scan-intake stage (gfx950).
//
// Reference: Mapper::Process' odometry carry and HasMovedEnough, LocalizedRangeScan::SetSensorPose / GetSensorAt,
// ScanManager::AddRunningScan and the node's readings loop (lesson6/lib/open_karto, lesson6/src/karto_slam.cc; the
// C-ABI and the arithmetic, operation by operation, are in include/slam2d/karto_process.h).
//   kp_intake_kernel     one wave per candidate, four candidates per workgroup, no workgroup barrier (the candidates
//                        are independent).  The decision is one chain of a few hundred dependent double operations:
//                        every lane evaluates it alike and lane 0 writes the record.
//   kp_compact_kernel    one workgroup: order-preserving prefix counts (256 candidates at a time) of the accepted
//                        candidates (job index), of those with a last scan (seq index) and of their running scans
//                        (the base lists' begins); the ke_job, kl_query and kl_closest_item rows.
//   kp_store_kernel      one workgroup per accepted candidate: the ranges row as double from the float row -- the only
//                        bandwidth part: the reversed row is READ backwards, so the stores stay coalesced -- the pool
//                        pose and the match's base list.
//   kp_apply_kernel      one lane per candidate: SetSensorPose(bestPose).
//   kp_bind_near_kernel  one lane per job: its range of the near batch, by bisection over d_source[].slot.
//   kp_advance_kernel    one wave per candidate: AddRunningScan's trim as a ballot over 64 fronts per round (each
//                        front's test is independent of the others, so the result is the serial loop's), then
//                        SetLastScan.
// All arithmetic is double with -ffp-contract=off and detmath.h's sin / cos / atan2; no atomics anywhere.  Every
// launch but kp_store_kernel is latency-bound.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/slam2d/karto_process.h"
#include "detmath.h"
#include "karto_pose_math.h"

namespace s2d {

constexpr int KP_THREADS = 256;
constexpr int KP_PER_BLOCK = KP_THREADS / 64;

// Pose2::operator+ / operator- (Karto.h:2128-2141)
KE_FN void kp_pose_add(const double *a, const double *b, double *out)
{
    out[0] = a[0] + b[0];
    out[1] = a[1] + b[1];
    out[2] = ke_normalize_angle(a[2] + b[2]);
}

KE_FN void kp_pose_sub(const double *a, const double *b, double *out)
{
    out[0] = a[0] - b[0];
    out[1] = a[1] - b[1];
    out[2] = ke_normalize_angle(a[2] - b[2]);
}

struct KpTransform {
    double rot[9], tr[3];
};

// Transform::SetTransform (Karto.h:2909-2935); the inverse rotation is never read
KE_FN void kp_set_transform(const double *p1, const double *p2, KpTransform *t)
{
    if (p1[0] == p2[0] && p1[1] == p2[1] && p1[2] == p2[2]) {
        for (int k = 0; k < 9; ++k) t->rot[k] = (k % 4 == 0) ? 1.0 : 0.0;
        t->tr[0] = t->tr[1] = t->tr[2] = 0.0;
        return;
    }
    ke_from_axis_angle(0.0, 0.0, 1.0, p2[2] - p1[2], t->rot);
    double np[3];
    if (p1[0] != 0.0 || p1[1] != 0.0) {
        double rp[3];
        ke_mul_pose(t->rot, p1, rp);
        kp_pose_sub(p2, rp, np);
    } else {
        np[0] = p2[0];
        np[1] = p2[1];
    }
    t->tr[0] = np[0];
    t->tr[1] = np[1];
    t->tr[2] = p2[2] - p1[2];
}

// Transform::TransformPose (Karto.h:2881-2887)
KE_FN void kp_transform_pose(const KpTransform *t, const double *src, double *out)
{
    double rp[3], np[3];
    ke_mul_pose(t->rot, src, rp);
    kp_pose_add(t->tr, rp, np);
    out[0] = np[0];
    out[1] = np[1];
    out[2] = ke_normalize_angle(src[2] + t->tr[2]);
}

// LocalizedRangeScan::GetSensorAt (Karto.h:5310-5313) with the offset Pose2()
KE_FN void kp_sensor_at(const double *pose, double *out)
{
    const double origin[3] = {0.0, 0.0, 0.0};
    KpTransform t;
    kp_set_transform(origin, pose, &t);
    kp_transform_pose(&t, origin, out);
}

// The corrected pose LocalizedRangeScan::SetSensorPose (Karto.h:5289-5300) gives, with the offset Pose2()
KE_FN void kp_corrected_of(const double *scan_pose, double *out)
{
    const double off[3] = {0.0, 0.0, 0.0};
    const double offsetLength = sqrt(off[0] * off[0] + off[1] * off[1]);
    const double offsetHeading = off[2];
    const double angleoffset = sdm_atan2(off[1], off[0]);
    const double correctedHeading = ke_normalize_angle(scan_pose[2]);
    const double world[3] = {offsetLength * sdm_cos(correctedHeading + angleoffset - offsetHeading),
                             offsetLength * sdm_sin(correctedHeading + angleoffset - offsetHeading), offsetHeading};
    kp_pose_sub(scan_pose, world, out);
}

struct KpGate {
    double min_time, min_heading, thr_travel;  // thr_travel = Square(minimum_travel_distance) - KT_TOLERANCE
};

// Mapper::Process up to HasMovedEnough (Mapper.cpp:2018-2031) for a scan with a last scan: the odometry carry from
// the last scan's current sensor pose, then the gate.  Returns HasMovedEnough.
KE_FN bool kp_carry_and_gate(const KpGate &gate, const double *last_sensor, const double *last_odom, double last_time,
                             double time, const double *odom, double *corrected)
{
    double last_corrected[3];
    kp_corrected_of(last_sensor, last_corrected);
    KpTransform t;
    kp_set_transform(last_odom, last_corrected, &t);
    kp_transform_pose(&t, odom, corrected);
    // HasMovedEnough (Mapper.cpp:2087-2120)
    const double timeInterval = time - last_time;
    if (timeInterval >= gate.min_time) return true;
    double lastScannerPose[3], scannerPose[3];
    kp_sensor_at(last_odom, lastScannerPose);
    kp_sensor_at(odom, scannerPose);
    const double deltaHeading = ke_normalize_angle(scannerPose[2] - lastScannerPose[2]);
    if (fabs(deltaHeading) >= gate.min_heading) return true;
    const double dx = lastScannerPose[0] - scannerPose[0], dy = lastScannerPose[1] - scannerPose[1];
    const double squaredTravelDistance = dx * dx + dy * dy;
    if (squaredTravelDistance >= gate.thr_travel) return true;
    return false;
}

// what kp_advance_kernel needs of an accepted candidate (SetLastScan)
struct KpPending {
    double time, odom[3];
};

struct KpArgs {
    int g_first, count, n_rows, pool_scans, max_scans, n_readings, inverted, base_capacity;
    KpGate gate;
    const kp_candidate *cand;
    const float *ranges_f32;
    const kp_state *state;
    const int *pool_offset;
    double *pool_ranges, *pool_poses;
    kp_intake *rec;
    KpPending *pending;
    int *query, *base_begin, *base_index, *n_seq, *n_jobs, *counts;
    ke_job *jobs;
    kl_query *queries;
    kl_closest_item *items;
};

__global__ void __launch_bounds__(KP_THREADS) kp_intake_kernel(KpArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * KP_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= a.count) return;  // the whole wave
    const int g = a.g_first + i;
    const kp_candidate c = a.cand[i];
    const kp_state st = a.state[g];
    kp_intake r;
    r.status = KP_OK;
    r.accepted = 0;
    r.scan = r.prev = r.job = r.seq = -1;
    r.run_begin = st.run_begin;
    r.run_length = st.run_length;
    r.match_status = 0;
    r.pad_ = 0;
    for (int k = 0; k < 3; ++k) r.corrected[k] = r.sensor[k] = 0.0;
    KpPending pd;
    pd.time = c.time;
    for (int k = 0; k < 3; ++k) pd.odom[k] = c.odom[k];
    const long long off = a.pool_offset[g];
    bool moved = false;
    if (c.row < 0) {
        // no scan for this graph this round
    } else if (c.row >= a.n_rows) {
        r.status = KP_EINVAL;
    } else if (st.n_scans <= 0) {
        // SetOdometricPose / SetCorrectedPose (karto_slam.cc:439-440); HasMovedEnough: pLastScan == NULL
        for (int k = 0; k < 3; ++k) r.corrected[k] = c.odom[k];
        moved = true;
    } else {
        r.prev = st.n_scans - 1;
        const long long last = off + r.prev;
        if (last >= a.pool_scans) {
            r.status = KP_EINVAL;
        } else {
            double last_sensor[3];
            for (int k = 0; k < 3; ++k) last_sensor[k] = a.pool_poses[last * 3 + k];
            moved = kp_carry_and_gate(a.gate, last_sensor, st.last_odom, st.last_time, c.time, c.odom, r.corrected);
        }
    }
    if (r.status == KP_OK && c.row >= 0) kp_sensor_at(r.corrected, r.sensor);
    if (moved) {
        if (st.n_scans >= a.max_scans) r.status = KP_ERANGE;
        else if (off + st.n_scans >= a.pool_scans) r.status = KP_EINVAL;
        else {
            r.accepted = 1;
            r.scan = st.n_scans;
        }
    }
    if (lane == 0) {
        a.rec[i] = r;
        a.pending[i] = pd;
    }
}

__global__ void __launch_bounds__(KP_THREADS) kp_compact_kernel(KpArgs a)
{
    __shared__ int s_job[KP_THREADS], s_seq[KP_THREADS], s_len[KP_THREADS];
    const int tid = threadIdx.x;
    int n_jobs = 0, n_seq = 0, n_base = 0;  // the same in every thread
    for (int base = 0; base < a.count; base += KP_THREADS) {
        const int i = base + tid;
        int acc = 0, seq = 0, len = 0, scan = -1, prev = -1, rb = 0;
        if (i < a.count) {
            const kp_intake *r = a.rec + i;
            acc = r->accepted;
            scan = r->scan;
            prev = r->prev;
            rb = r->run_begin;
            seq = acc && prev >= 0;
            len = seq ? r->run_length : 0;
        }
        s_job[tid] = acc;
        s_seq[tid] = seq;
        s_len[tid] = len;
        __syncthreads();
        for (int d = 1; d < KP_THREADS; d <<= 1) {  // inclusive prefix sums
            const int pj = tid >= d ? s_job[tid - d] : 0;
            const int ps = tid >= d ? s_seq[tid - d] : 0;
            const int pl = tid >= d ? s_len[tid - d] : 0;
            __syncthreads();
            s_job[tid] += pj;
            s_seq[tid] += ps;
            s_len[tid] += pl;
            __syncthreads();
        }
        if (i < a.count) {
            const int g = a.g_first + i;
            const int off = a.pool_offset[g];
            const int j = acc ? n_jobs + s_job[tid] - 1 : -1;
            const int s = seq ? n_seq + s_seq[tid] - 1 : -1;
            a.rec[i].job = j;
            a.rec[i].seq = s;
            if (acc) {
                if (a.jobs) {
                    ke_job jb;
                    jb.graph = g;
                    jb.scan = scan;
                    jb.pool_offset = off;
                    jb.prev = prev;
                    jb.seq_result = s;
                    jb.running = s;
                    jb.near_first = jb.near_count = 0;
                    a.jobs[j] = jb;
                }
                if (a.queries) {
                    kl_query q;
                    q.graph = g;
                    q.scan = scan;
                    q.start_num = 0;
                    q.n_scans = q.n_edges = -1;
                    a.queries[j] = q;
                }
            }
            if (seq) {
                const int b0 = n_base + s_len[tid] - len;
                a.query[s] = off + scan;
                a.base_begin[s] = b0;
                a.base_begin[s + 1] = b0 + len;
                if (a.items) {
                    kl_closest_item it;
                    it.graph = g;
                    it.scan = scan;
                    it.begin = rb;
                    it.length = len;
                    a.items[s] = it;
                }
            }
        }
        n_jobs += s_job[KP_THREADS - 1];
        n_seq += s_seq[KP_THREADS - 1];
        n_base += s_len[KP_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        if (n_seq == 0) a.base_begin[0] = 0;
        *a.n_seq = n_seq;
        *a.n_jobs = n_jobs;
        a.counts[0] = n_jobs;
        a.counts[1] = n_seq;
    }
}

__global__ void __launch_bounds__(KP_THREADS) kp_store_kernel(KpArgs a)
{
    const int i = blockIdx.x, tid = threadIdx.x;
    const kp_intake r = a.rec[i];
    if (!r.accepted) return;  // the whole workgroup
    const int off = a.pool_offset[a.g_first + i];
    const size_t slot = (size_t)off + r.scan;  // < pool_scans: kp_intake_kernel accepted it
    const int n = a.n_readings;
    const float *src = a.ranges_f32 + (size_t)a.cand[i].row * n;
    double *dst = a.pool_ranges + slot * n;
    // readings.push_back(*it) over the float ranges, from the back when the laser is inverted (karto_slam.cc:417-434)
    for (int k = tid; k < n; k += KP_THREADS) dst[k] = (double)src[a.inverted ? n - 1 - k : k];
    if (tid < 3) a.pool_poses[slot * 3 + tid] = r.sensor[tid];
    if (r.seq >= 0) {
        const int b0 = a.base_begin[r.seq];
        for (int k = tid; k < r.run_length; k += KP_THREADS)
            if (b0 + k < a.base_capacity) a.base_index[b0 + k] = off + r.run_begin + k;
    }
}

__global__ void __launch_bounds__(64) kp_apply_kernel(int g_first, int count, int n_seq, int pool_scans,
                                                      const int *pool_offset, const kt_result *seq, kp_intake *rec,
                                                      double *pool_poses)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    kp_intake r = rec[i];
    if (!r.accepted || r.seq < 0) return;
    if (r.seq >= n_seq) {
        rec[i].match_status = KP_EINVAL;
        return;
    }
    const kt_result *m = seq + r.seq;
    r.match_status = m->status;
    if (m->status == KT_OK) {
        const size_t slot = (size_t)pool_offset[g_first + i] + r.scan;
        for (int k = 0; k < 3; ++k) r.sensor[k] = m->mean[k];
        kp_corrected_of(r.sensor, r.corrected);
        if (slot < (size_t)pool_scans)
            for (int k = 0; k < 3; ++k) pool_poses[slot * 3 + k] = r.sensor[k];
    }
    rec[i] = r;
}

__global__ void __launch_bounds__(64) kp_bind_near_kernel(const int *counts, int max_jobs, ke_job *jobs,
                                                          const kl_source *source, const int *n_matches,
                                                          int max_matches)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= min(counts[0], max_jobs)) return;
    const int n = max(0, min(*n_matches, max_matches));
    int first[2];
    for (int e = 0; e < 2; ++e) {  // the first match with slot >= j, then with slot >= j + 1
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (source[mid].slot < j + e) lo = mid + 1;
            else hi = mid;
        }
        first[e] = lo;
    }
    jobs[j].near_first = first[0];
    jobs[j].near_count = first[1] - first[0];
}

struct KpAdvanceArgs {
    int g_first, count, pool_scans, buffer_size;
    double thr_buffer;  // Square(scan_buffer_maximum_scan_distance) - KT_TOLERANCE
    const int *pool_offset;
    const double *pool_poses;
    const kp_intake *rec;
    const KpPending *pending;
    kp_state *state;
    kp_advanced *adv;
};

__global__ void __launch_bounds__(KP_THREADS) kp_advance_kernel(KpAdvanceArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * KP_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= a.count) return;  // the whole wave
    const int g = a.g_first + i;
    const kp_intake r = a.rec[i];
    kp_state st = a.state[g];
    kp_advanced o;
    o.accepted = 0;
    o.corrected[0] = o.corrected[1] = o.corrected[2] = 0.0;
    const long long off = a.pool_offset[g];
    if (r.accepted && r.scan == st.n_scans && off + r.scan < a.pool_scans) {
        const int back = r.scan;
        const int front = st.run_length > 0 ? max(0, st.run_begin) : back;
        const double *pool = a.pool_poses + off * 3;
        const double bx = pool[(size_t)back * 3], by = pool[(size_t)back * 3 + 1];
        int new_front = back;
        for (int base = front; base <= back; base += 64) {
            const int f = base + lane;
            bool keep = false;
            if (f <= back) {
                const double dx = pool[(size_t)f * 3] - bx, dy = pool[(size_t)f * 3 + 1] - by;
                const double squaredDistance = dx * dx + dy * dy;
                keep = back - f + 1 <= a.buffer_size && !(squaredDistance > a.thr_buffer);
            }
            const unsigned long long mask = __ballot(keep);
            if (mask != 0) {  // wave-uniform
                new_front = base + __ffsll(mask) - 1;
                break;
            }
        }
        st.run_begin = new_front;
        st.run_length = back - new_front + 1;
        st.n_scans = back + 1;
        const KpPending pd = a.pending[i];
        st.last_time = pd.time;
        for (int k = 0; k < 3; ++k) st.last_odom[k] = pd.odom[k];
        double sensor[3] = {bx, by, pool[(size_t)back * 3 + 2]};
        kp_corrected_of(sensor, o.corrected);
        o.accepted = 1;
        if (lane == 0) a.state[g] = st;
    }
    o.run_begin = st.run_begin;
    o.run_length = st.run_length;
    o.n_scans = st.n_scans;
    if (lane == 0) a.adv[i] = o;
}

}  // namespace s2d
