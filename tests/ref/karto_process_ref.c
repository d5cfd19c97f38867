/* tests/ref/karto_process_ref.c -- CPU restatement of the Karto scan-intake stage (include/slam2d/karto_process.h) the
 * GPU is held to: the odometry carry, HasMovedEnough, SetSensorPose, the compacted arrays that join the stages and
 * AddRunningScan, sequentially, one candidate after the other.  Test infrastructure: built on demand by
 * tests/ref/karto_process_ref.py with gcc -O2 -ffp-contract=off; sin / cos / atan2 are csrc/detmath.h's.  The literal
 * transcription of the reference members is tests/ref/karto_process_plain.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "detmath.h"
#include "slam2d/karto_process.h"

#define R_PI 3.14159265358979323846
#define R_2PI 6.28318530717958647692

typedef struct { double m[3][3]; } M3;
typedef struct { double x, y, h; } P2;
typedef struct { M3 rot; P2 tr; } TF;

static double normalize_angle(double angle)
{
    if (!(fabs(angle) < 4294967296.0)) return NAN;
    while (angle < -R_PI) {
        if (angle < -R_2PI) angle += (uint32_t)(angle / -R_2PI) * R_2PI;
        else angle += R_2PI;
    }
    while (angle > R_PI) {
        if (angle > R_2PI) angle -= (uint32_t)(angle / R_2PI) * R_2PI;
        else angle -= R_2PI;
    }
    return angle;
}

static M3 from_axis_angle(double x, double y, double z, double radians)
{
    M3 r;
    double c = sdm_cos(radians), s = sdm_sin(radians), omc = 1.0 - c;
    double xx = x * x, yy = y * y, zz = z * z;
    double xy = x * y * omc, xz = x * z * omc, yz = y * z * omc;
    double xs = x * s, ys = y * s, zs = z * s;
    r.m[0][0] = xx * omc + c; r.m[0][1] = xy - zs;       r.m[0][2] = xz + ys;
    r.m[1][0] = xy + zs;      r.m[1][1] = yy * omc + c;  r.m[1][2] = yz - xs;
    r.m[2][0] = xz - ys;      r.m[2][1] = yz + xs;       r.m[2][2] = zz * omc + c;
    return r;
}

static P2 m3_pose(const M3 *m, P2 p)
{
    P2 o;
    o.x = m->m[0][0] * p.x + m->m[0][1] * p.y + m->m[0][2] * p.h;
    o.y = m->m[1][0] * p.x + m->m[1][1] * p.y + m->m[1][2] * p.h;
    o.h = m->m[2][0] * p.x + m->m[2][1] * p.y + m->m[2][2] * p.h;
    return o;
}

static P2 p2_add(P2 a, P2 b) { P2 o = {a.x + b.x, a.y + b.y, normalize_angle(a.h + b.h)}; return o; }
static P2 p2_sub(P2 a, P2 b) { P2 o = {a.x - b.x, a.y - b.y, normalize_angle(a.h - b.h)}; return o; }
static P2 p2_of(const double *v) { P2 o = {v[0], v[1], v[2]}; return o; }
static void p2_to(P2 p, double *v) { v[0] = p.x; v[1] = p.y; v[2] = p.h; }

/* Transform::SetTransform */
static TF set_transform(P2 p1, P2 p2)
{
    TF t;
    if (p1.x == p2.x && p1.y == p2.y && p1.h == p2.h) {
        memset(&t, 0, sizeof(t));
        t.rot.m[0][0] = t.rot.m[1][1] = t.rot.m[2][2] = 1.0;
        return t;
    }
    t.rot = from_axis_angle(0, 0, 1, p2.h - p1.h);
    P2 np = p2;
    if (p1.x != 0.0 || p1.y != 0.0) np = p2_sub(p2, m3_pose(&t.rot, p1));
    t.tr.x = np.x;
    t.tr.y = np.y;
    t.tr.h = p2.h - p1.h;
    return t;
}

/* Transform::TransformPose */
static P2 transform_pose(const TF *t, P2 s)
{
    P2 np = p2_add(t->tr, m3_pose(&t->rot, s));
    P2 o = {np.x, np.y, normalize_angle(s.h + t->tr.h)};
    return o;
}

/* GetSensorAt with the offset Pose2() */
static P2 sensor_at(P2 pose)
{
    P2 zero = {0.0, 0.0, 0.0};
    TF t = set_transform(zero, pose);
    return transform_pose(&t, zero);
}

/* the corrected pose SetSensorPose gives, with the offset Pose2() */
static P2 corrected_of(P2 scan_pose)
{
    P2 off = {0.0, 0.0, 0.0};
    double offsetLength = sqrt(off.x * off.x + off.y * off.y);
    double offsetHeading = off.h;
    double angleoffset = sdm_atan2(off.y, off.x);
    double correctedHeading = normalize_angle(scan_pose.h);
    P2 world = {offsetLength * sdm_cos(correctedHeading + angleoffset - offsetHeading),
                offsetLength * sdm_sin(correctedHeading + angleoffset - offsetHeading), offsetHeading};
    return p2_sub(scan_pose, world);
}

void kpr_sensor_at(const double *pose, double *out) { p2_to(sensor_at(p2_of(pose)), out); }
void kpr_corrected_of(const double *pose, double *out) { p2_to(corrected_of(p2_of(pose)), out); }

/* Square(d) - KT_TOLERANCE, as kp_create computes it */
double kpr_threshold(double d) { return d * d - KL_TOLERANCE; }

/* 0: kp_create would refuse */
int kpr_check_create(const kp_params *p, int n_readings, int max_scans)
{
    if (n_readings < 1 || n_readings > 4096 || max_scans < 1 || max_scans > KL_MAX_SCANS) return 0;
    if (p->scan_buffer_size < 1) return 0;
    if (p->minimum_time_interval != p->minimum_time_interval || p->minimum_travel_distance != p->minimum_travel_distance ||
        p->minimum_travel_heading != p->minimum_travel_heading)
        return 0;
    if (p->inverted != 0 && p->inverted != 1) return 0;
    if (!(kpr_threshold(p->scan_buffer_maximum_scan_distance) >= 0.0)) return 0;
    return 1;
}

static int has_moved_enough(const kp_params *p, const kp_state *st, double time, P2 odom)
{
    double timeInterval = time - st->last_time;
    if (timeInterval >= p->minimum_time_interval) return 1;
    P2 last = sensor_at(p2_of(st->last_odom)), cur = sensor_at(odom);
    double deltaHeading = normalize_angle(cur.h - last.h);
    if (fabs(deltaHeading) >= p->minimum_travel_heading) return 1;
    double dx = last.x - cur.x, dy = last.y - cur.y;
    if (dx * dx + dy * dy >= kpr_threshold(p->minimum_travel_distance)) return 1;
    return 0;
}

/* kp_intake_device.  Rows the call does not write are left as they are (the loader poisons them). */
void kpr_intake(const kp_params *p, int n_readings, int max_scans, int g_first, int count, const int *pool_offset,
                const kp_state *state, const kp_candidate *cand, const float *ranges_f32, int n_rows, double *pool_ranges,
                double *pool_poses, int pool_scans, kp_intake *rec, int *query, int *base_begin, int *base_index, int *n_seq_out,
                ke_job *jobs, kl_query *queries, int *n_jobs_out, kl_closest_item *items)
{
    int n_jobs = 0, n_seq = 0, n_base = 0;
    for (int i = 0; i < count; ++i) {
        const int g = g_first + i;
        const kp_candidate *c = cand + i;
        const kp_state *st = state + g;
        const long long off = pool_offset[g];
        kp_intake r;
        memset(&r, 0, sizeof(r));
        r.scan = r.prev = r.job = r.seq = -1;
        r.run_begin = st->run_begin;
        r.run_length = st->run_length;
        int moved = 0;
        P2 corrected = {0.0, 0.0, 0.0};
        if (c->row < 0) {
        } else if (c->row >= n_rows) {
            r.status = KP_EINVAL;
        } else if (st->n_scans <= 0) {
            corrected = p2_of(c->odom);
            moved = 1;
        } else {
            r.prev = st->n_scans - 1;
            if (off + r.prev >= pool_scans) {
                r.status = KP_EINVAL;
            } else {
                P2 lastCorrected = corrected_of(p2_of(pool_poses + (off + r.prev) * 3));
                TF lastTransform = set_transform(p2_of(st->last_odom), lastCorrected);
                corrected = transform_pose(&lastTransform, p2_of(c->odom));
                moved = has_moved_enough(p, st, c->time, p2_of(c->odom));
            }
        }
        p2_to(corrected, r.corrected);
        if (r.status == KP_OK && c->row >= 0) p2_to(sensor_at(corrected), r.sensor);
        if (moved) {
            if (st->n_scans >= max_scans) r.status = KP_ERANGE;
            else if (off + st->n_scans >= pool_scans) r.status = KP_EINVAL;
            else {
                r.accepted = 1;
                r.scan = st->n_scans;
            }
        }
        if (r.accepted) {
            const long long slot = off + r.scan;
            const float *src = ranges_f32 + (size_t)c->row * n_readings;
            for (int k = 0; k < n_readings; ++k)
                pool_ranges[slot * n_readings + k] = (double)src[p->inverted ? n_readings - 1 - k : k];
            for (int k = 0; k < 3; ++k) pool_poses[slot * 3 + k] = r.sensor[k];
            r.job = n_jobs++;
            if (r.prev >= 0) {
                r.seq = n_seq++;
                query[r.seq] = (int)slot;
                base_begin[r.seq] = n_base;
                for (int k = 0; k < r.run_length; ++k) base_index[n_base++] = (int)off + r.run_begin + k;
                base_begin[r.seq + 1] = n_base;
                kl_closest_item it = {g, r.scan, r.run_begin, r.run_length};
                items[r.seq] = it;
            }
            ke_job jb = {g, r.scan, (int)off, r.prev, r.seq, r.seq, 0, 0};
            jobs[r.job] = jb;
            kl_query q = {g, r.scan, 0, -1, -1};
            queries[r.job] = q;
        }
        rec[i] = r;
    }
    if (n_seq == 0) base_begin[0] = 0;
    *n_seq_out = n_seq;
    *n_jobs_out = n_jobs;
}

/* kp_apply_match_device */
void kpr_apply(int g_first, int count, const int *pool_offset, const kt_result *seq, int n_seq, kp_intake *rec,
               double *pool_poses, int pool_scans)
{
    for (int i = 0; i < count; ++i) {
        kp_intake *r = rec + i;
        if (!r->accepted || r->seq < 0) continue;
        if (r->seq >= n_seq) {
            r->match_status = KP_EINVAL;
            continue;
        }
        const kt_result *m = seq + r->seq;
        r->match_status = m->status;
        if (m->status != KT_OK) continue;
        const long long slot = (long long)pool_offset[g_first + i] + r->scan;
        for (int k = 0; k < 3; ++k) r->sensor[k] = m->mean[k];
        p2_to(corrected_of(p2_of(r->sensor)), r->corrected);
        if (slot < pool_scans)
            for (int k = 0; k < 3; ++k) pool_poses[slot * 3 + k] = r->sensor[k];
    }
}

/* kp_bind_near_device */
void kpr_bind_near(int n_jobs, ke_job *jobs, const kl_source *source, int n_matches)
{
    for (int j = 0; j < n_jobs; ++j) {
        int first = 0, n = 0;
        while (first < n_matches && source[first].slot < j) ++first;
        while (first + n < n_matches && source[first + n].slot < j + 1) ++n;
        jobs[j].near_first = first;
        jobs[j].near_count = n;
    }
}

/* kp_advance_device: the new front is the first f with back - f + 1 <= size && !(d2(f, back) > thr) */
void kpr_advance(const kp_params *p, int g_first, int count, const int *pool_offset, const kp_intake *rec,
                 const kp_candidate *cand, const double *pool_poses, int pool_scans, kp_state *state, kp_advanced *adv)
{
    const double thr = kpr_threshold(p->scan_buffer_maximum_scan_distance);
    for (int i = 0; i < count; ++i) {
        const int g = g_first + i;
        const kp_intake *r = rec + i;
        kp_state *st = state + g;
        const long long off = pool_offset[g];
        kp_advanced o;
        memset(&o, 0, sizeof(o));
        if (r->accepted && r->scan == st->n_scans && off + r->scan < pool_scans) {
            const int back = r->scan;
            const double *pool = pool_poses + off * 3;
            int f = st->run_length > 0 ? (st->run_begin > 0 ? st->run_begin : 0) : back;
            for (; f < back; ++f) {
                const double dx = pool[f * 3] - pool[back * 3], dy = pool[f * 3 + 1] - pool[back * 3 + 1];
                if (back - f + 1 <= p->scan_buffer_size && !(dx * dx + dy * dy > thr)) break;
            }
            st->run_begin = f;
            st->run_length = back - f + 1;
            st->n_scans = back + 1;
            st->last_time = cand[i].time;
            memcpy(st->last_odom, cand[i].odom, sizeof(st->last_odom));
            p2_to(corrected_of(p2_of(pool + back * 3)), o.corrected);
            o.accepted = 1;
        }
        o.run_begin = st->run_begin;
        o.run_length = st->run_length;
        o.n_scans = st->n_scans;
        adv[i] = o;
    }
}
