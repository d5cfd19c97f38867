/* tests/ref/karto_link_ref.c -- CPU restatement of the Karto graph-linking stage (include/slam2d/karto_link.h) the
 * GPU is held to: AddEdges, the tests of TryCloseLoop, LinkInfo, AddConstraint's precision matrix and
 * ComputeWeightedMean, sequentially, one job after the other, with the lists the reference builds.  Test
 * infrastructure: built on demand by tests/ref/karto_link_ref.py with gcc -O2 -ffp-contract=off; sin / cos / atan2
 * are csrc/detmath.h's.  The literal transcription of the reference members is tests/ref/karto_link_plain.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "detmath.h"
#include "slam2d/karto_link.h"

#define R_PI 3.14159265358979323846
#define R_2PI 6.28318530717958647692

double ker_sin(double x) { return sdm_sin(x); }
double ker_cos(double x) { return sdm_cos(x); }
double ker_atan2(double y, double x) { return sdm_atan2(y, x); }

double ker_normalize_angle(double angle)
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

typedef struct { double m[3][3]; } M3;
typedef struct { double x, y, h; } P2;

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

static M3 m3_mul(const M3 *a, const M3 *b)
{
    M3 p;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            p.m[r][c] = a->m[r][0] * b->m[0][c] + a->m[r][1] * b->m[1][c] + a->m[r][2] * b->m[2][c];
    return p;
}

static M3 m3_transpose(const M3 *a)
{
    M3 t;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) t.m[r][c] = a->m[c][r];
    return t;
}

static P2 m3_pose(const M3 *m, P2 p)
{
    P2 o;
    o.x = m->m[0][0] * p.x + m->m[0][1] * p.y + m->m[0][2] * p.h;
    o.y = m->m[1][0] * p.x + m->m[1][1] * p.y + m->m[1][2] * p.h;
    o.h = m->m[2][0] * p.x + m->m[2][1] * p.y + m->m[2][2] * p.h;
    return o;
}

/* 1: inverted; 0: the reference asserts (or the determinant is NaN) */
static int m3_inverse(const M3 *a, M3 *inv)
{
    const double(*m)[3] = a->m;
    inv->m[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    inv->m[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
    inv->m[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    inv->m[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    inv->m[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
    inv->m[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    inv->m[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    inv->m[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
    inv->m[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    double det = m[0][0] * inv->m[0][0] + m[0][1] * inv->m[1][0] + m[0][2] * inv->m[2][0];
    if (!(fabs(det) > 1e-14)) return 0;
    double id = 1.0 / det;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) inv->m[r][c] *= id;
    return 1;
}

static M3 m3_of(const double *v)
{
    M3 r;
    memcpy(r.m, v, sizeof(r.m));
    return r;
}

/* LinkInfo::Update + AddConstraint's matrix */
int ker_link_info(const double *pose1, const double *pose2, const double *cov, double *diff, double *prec)
{
    P2 p1 = {pose1[0], pose1[1], pose1[2]}, p2 = {pose2[0], pose2[1], pose2[2]};
    M3 rot;
    P2 tr;
    if (p1.x == 0.0 && p1.y == 0.0 && p1.h == 0.0) {
        memset(&rot, 0, sizeof(rot));
        rot.m[0][0] = rot.m[1][1] = rot.m[2][2] = 1.0;
        tr.x = tr.y = tr.h = 0.0;
    } else {
        rot = from_axis_angle(0, 0, 1, 0.0 - p1.h);
        if (p1.x != 0.0 || p1.y != 0.0) {
            P2 rp = m3_pose(&rot, p1);
            tr.x = 0.0 - rp.x;
            tr.y = 0.0 - rp.y;
        } else {
            tr.x = 0.0;
            tr.y = 0.0;
        }
        tr.h = 0.0 - p1.h;
    }
    P2 rp2 = m3_pose(&rot, p2);
    double dx = tr.x + rp2.x, dy = tr.y + rp2.y, dh = ker_normalize_angle(p2.h + tr.h);
    M3 r1 = from_axis_angle(0, 0, 1, -p1.h), c = m3_of(cov);
    M3 r1t = m3_transpose(&r1), a = m3_mul(&r1, &c), rc = m3_mul(&a, &r1t), p;
    if (!m3_inverse(&rc, &p)) {
        memset(diff, 0, 3 * sizeof(double));
        memset(prec, 0, 9 * sizeof(double));
        return KE_SINGULAR;
    }
    p.m[1][0] = p.m[0][1];
    p.m[2][0] = p.m[0][2];
    p.m[2][1] = p.m[1][2];
    diff[0] = dx;
    diff[1] = dy;
    diff[2] = dh;
    memcpy(prec, p.m, sizeof(p.m));
    return KE_OK;
}

/* ComputeWeightedMean over n (>= 1) items: KE_OK and out, or KE_SINGULAR */
int ker_weighted_mean(int n, const double *means, const double *covs, double *out)
{
    M3 *inv = (M3 *)malloc(sizeof(M3) * (size_t)n);
    M3 sum, isum;
    int rc = KE_OK;
    memset(&sum, 0, sizeof(sum));
    for (int i = 0; i < n && rc == KE_OK; ++i) {
        M3 c = m3_of(covs + 9 * i);
        if (!m3_inverse(&c, &inv[i])) rc = KE_SINGULAR;
        else
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k) sum.m[r][k] += inv[i].m[r][k];
    }
    if (rc == KE_OK && !m3_inverse(&sum, &isum)) rc = KE_SINGULAR;
    if (rc == KE_OK) {
        P2 acc = {0.0, 0.0, 0.0};
        double tx = 0.0, ty = 0.0;
        for (int i = 0; i < n; ++i) {
            P2 p = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
            tx += sdm_cos(p.h);
            ty += sdm_sin(p.h);
            M3 w = m3_mul(&isum, &inv[i]);
            P2 wp = m3_pose(&w, p);
            acc.x += wp.x;
            acc.y += wp.y;
            acc.h = ker_normalize_angle(acc.h + wp.h);
        }
        tx /= (double)n;
        ty /= (double)n;
        out[0] = acc.x;
        out[1] = acc.y;
        out[2] = sdm_atan2(ty, tx);
    }
    free(inv);
    return rc;
}

static void put_link(ke_link *l, int from, int to, int kind, const double *from_pose, const double *mean, const double *cov)
{
    l->from = from;
    l->to = to;
    l->kind = kind;
    l->status = ker_link_info(from_pose, mean, cov, l->diff, l->precision);
}

/* AddEdges for `count` jobs, sequentially; rows the job does not write are left as they are */
void ker_add_edges(int count, const ke_job *jobs, double *pool, int pool_scans, const kt_result *seq, int n_seq,
                   const kl_closest *running, int n_running, const kt_result *near, const kl_source *src, int n_near,
                   const kl_near_chain *chains, int chain_stride, int n_slots, int flags, double link_min, int max_links,
                   ke_link *links, ke_job_out *out)
{
    const double thr = link_min - KL_TOLERANCE;
    for (int j = 0; j < count; ++j) {
        const ke_job jb = jobs[j];
        ke_job_out *o = &out[j];
        memset(o, 0, sizeof(*o));
        o->graph = jb.graph;
        long long slot = (long long)jb.pool_offset + jb.scan;
        if (jb.scan < 0 || jb.pool_offset < 0 || slot >= pool_scans) {
            o->status = KE_EINVAL;
            continue;
        }
        double *pose = pool + 3 * slot;
        memcpy(o->pose, pose, sizeof(o->pose));
        int bad = jb.running < -1 || jb.running >= n_running || jb.near_count < 0 || jb.near_first < 0 ||
                  (long long)jb.near_first + jb.near_count > n_near;
        if (jb.prev >= 0)
            bad = bad || (long long)jb.pool_offset + jb.prev >= pool_scans || jb.seq_result < 0 || jb.seq_result >= n_seq;
        /* the records, as (from, kind, mean, cov), and the mean list */
        int cap = 2 + (bad ? 0 : jb.near_count), nl = 0, nm = 0;
        int *from = (int *)malloc(sizeof(int) * (size_t)cap), *kind = (int *)malloc(sizeof(int) * (size_t)cap);
        const double **lmean = (const double **)malloc(sizeof(double *) * (size_t)cap);
        const double **lcov = (const double **)malloc(sizeof(double *) * (size_t)cap);
        double *means = (double *)malloc(sizeof(double) * 3 * (size_t)cap), *covs = (double *)malloc(sizeof(double) * 9 * (size_t)cap);
        if (!bad && jb.prev >= 0) {
            const double *rcov = seq[jb.seq_result].covariance;
            from[nl] = jb.prev; kind[nl] = KE_PREV; lmean[nl] = pose; lcov[nl] = rcov; ++nl;
            memcpy(means, pose, 3 * sizeof(double));
            memcpy(covs, rcov, 9 * sizeof(double));
            nm = 1;
            if (jb.running >= 0 && running[jb.running].linked) {
                int cl = running[jb.running].closest;
                if (cl < 0 || (long long)jb.pool_offset + cl >= pool_scans) bad = 1;
                else { from[nl] = cl; kind[nl] = KE_RUNNING; lmean[nl] = pose; lcov[nl] = rcov; ++nl; }
            }
        }
        for (int k = 0; !bad && k < jb.near_count; ++k) {
            const kt_result *r = &near[jb.near_first + k];
            if (!(r->response > thr)) continue;
            memcpy(means + 3 * nm, r->mean, 3 * sizeof(double));
            memcpy(covs + 9 * nm, r->covariance, 9 * sizeof(double));
            ++nm;
            kl_source s = src[jb.near_first + k];
            if (s.slot < 0 || s.slot >= n_slots || s.chain < 0 || s.chain >= chain_stride) { bad = 1; break; }
            kl_near_chain ch = chains[(size_t)s.slot * chain_stride + s.chain];
            if (!(ch.flags & KL_CHAIN_LINKED)) continue;
            if (ch.closest < 0 || (long long)jb.pool_offset + ch.closest >= pool_scans) { bad = 1; break; }
            from[nl] = ch.closest; kind[nl] = KE_NEAR; lmean[nl] = r->mean; lcov[nl] = r->covariance; ++nl;
        }
        if (bad) o->status = KE_EINVAL;
        else if (nl > max_links) o->status = KE_ERANGE;
        else {
            for (int i = 0; i < nl; ++i)
                put_link(&links[(size_t)j * max_links + i], from[i], jb.scan, kind[i],
                         pool + 3 * ((long long)jb.pool_offset + from[i]), lmean[i], lcov[i]);
            o->n_links = nl;
            o->n_means = nm;
            if (nm > 0) {
                double mean[3];
                o->status = ker_weighted_mean(nm, means, covs, mean);
                if (o->status == KE_OK) {
                    memcpy(o->pose, mean, sizeof(mean));
                    if (flags & KE_WRITE_POSE) memcpy(pose, mean, sizeof(mean));
                }
            }
        }
        free(from); free(kind); free((void *)lmean); free((void *)lcov); free(means); free(covs);
    }
}

/* info[2]: accepted before the cut, status bits */
void ker_loop_coarse(int n, const kt_result *coarse, const int *query, const int *bb, const int *bi,
                     const double *pool_ranges, int pool_scans, int n_readings, int tmp_first, int capacity,
                     int base_capacity, double min_coarse, double max_var, int *fq, int *fbb, int *fbi, int *fof,
                     int *n_fine, double *tmp_ranges, double *tmp_poses, int *info)
{
    int accepted = 0, kept = 0, st = 0, open = 1;
    long long bsum = 0;
    fbb[0] = 0;
    for (int m = 0; m < n; ++m) {
        const kt_result *r = &coarse[m];
        if (!(r->response > min_coarse && r->covariance[0] < max_var && r->covariance[4] < max_var)) continue;
        if (query[m] < 0 || query[m] >= pool_scans || bb[m] < 0 || bb[m + 1] < bb[m]) { st |= KE_LOOP_EINVAL; continue; }
        ++accepted;
        int len = bb[m + 1] - bb[m];
        if (!open || kept >= capacity || bsum + len > base_capacity) { open = 0; st |= KE_LOOP_OVERFLOW; continue; }
        int f = kept++;
        fq[f] = tmp_first + f;
        fof[f] = m;
        fbb[f] = (int)bsum;
        memcpy(fbi + bsum, bi + bb[m], sizeof(int) * (size_t)len);
        bsum += len;
        fbb[f + 1] = (int)bsum;
        memcpy(tmp_ranges + (size_t)f * n_readings, pool_ranges + (size_t)query[m] * n_readings, sizeof(double) * (size_t)n_readings);
        memcpy(tmp_poses + 3 * f, r->mean, 3 * sizeof(double));
    }
    for (int f = kept; f < capacity; ++f) {
        for (int i = 0; i < n_readings; ++i) tmp_ranges[(size_t)f * n_readings + i] = INFINITY;
        tmp_poses[3 * f] = tmp_poses[3 * f + 1] = tmp_poses[3 * f + 2] = 0.0;
    }
    *n_fine = kept;
    info[0] = accepted;
    info[1] = st;
}

void ker_loop_fine(int count, int n_fine, const kt_result *fine, const int *fof, int max_matches, const kl_source *source,
                   const int *query, const kl_loop_chain *loop_chains, int chain_stride, double min_fine,
                   ke_closure *closures, double *pool, int pool_scans, int flags)
{
    for (int s = 0; s < count; ++s) {
        ke_closure *c = &closures[s];
        memset(c, 0, sizeof(*c));
        c->chain = c->resume = c->fine = -1;
    }
    for (int f = 0; f < n_fine; ++f) {
        int m = fof[f];
        if (m < 0 || m >= max_matches) continue;
        int s = source[m].slot, chain = source[m].chain;
        if (s < 0 || s >= count || closures[s].chain >= 0) continue;
        if (fine[f].response < min_fine) continue;
        if (chain < 0 || chain >= chain_stride) continue;
        ke_closure *c = &closures[s];
        c->chain = chain;
        c->resume = loop_chains[(size_t)s * chain_stride + chain].resume;
        c->fine = f;
        memcpy(c->pose, fine[f].mean, sizeof(c->pose));
        memcpy(c->covariance, fine[f].covariance, sizeof(c->covariance));
        if ((flags & KE_WRITE_POSE) && query[m] >= 0 && query[m] < pool_scans) memcpy(pool + 3 * (size_t)query[m], c->pose, sizeof(c->pose));
    }
}

void ker_close(int count, const ke_job *jobs, const ke_closure *closures, const kl_closest *closest, const double *pool,
               int pool_scans, int max_links, ke_link *links, ke_job_out *out)
{
    for (int s = 0; s < count; ++s) {
        const ke_job jb = jobs[s];
        ke_job_out *o = &out[s];
        memset(o, 0, sizeof(*o));
        o->graph = jb.graph;
        long long slot = (long long)jb.pool_offset + jb.scan;
        if (jb.scan < 0 || jb.pool_offset < 0 || slot >= pool_scans) { o->status = KE_EINVAL; continue; }
        const ke_closure *c = &closures[s];
        memcpy(o->pose, c->chain >= 0 ? c->pose : pool + 3 * slot, sizeof(o->pose));
        if (c->chain < 0 || !closest[s].linked) continue;
        int cl = closest[s].closest;
        if (cl < 0 || (long long)jb.pool_offset + cl >= pool_scans) { o->status = KE_EINVAL; continue; }
        put_link(&links[(size_t)s * max_links], cl, jb.scan, KE_LOOP, pool + 3 * ((long long)jb.pool_offset + cl), c->pose, c->covariance);
        o->n_links = 1;
    }
}
