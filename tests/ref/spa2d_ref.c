/* tests/ref/spa2d_ref.c -- sequential CPU restatement of SysSPA2d::doSPA in its block-Jacobi PCG mode,
 *   doSPA(niter, sLambda, SBA_BLOCK_JACOBIAN_PCG, initTol, maxCGiters)
 * (lesson6/lib/sparse_bundle_adjustment/src/spa2d.cpp:425-609).  Test infrastructure: the package never loads it.
 *
 * It keeps the reference's loops: setupSparseSys scatters over the constraints into diag / cols / B
 * (spa2d.cpp:351-392), the off-diagonal blocks live in per-column sorted lists as cols[] does
 * (csparse.cpp:472-485), and mMV2 scatters over the column-sorted block list (bpcg/bpcg.h:142-161).  The kernel
 * gathers instead; that the gathers give these bits is what the GPU tests check.
 *
 * Eigen is absent, so its product, inverse and dot orders are unpinned; this file fixes them as
 * include/slam2d/spa.h states (left to right products, (a0*b0 + a1*b1) + a2*b2, cofactor inverse, the 256-lane
 * reduction shape).  sin / cos are csrc/detmath.h's.  Build: gcc -O2 -ffp-contract=off.
 */
#include <stdlib.h>
#include <string.h>

#include "detmath.h"

#define LANES 256

typedef struct spa2d_ref_stats {
    int status, good_iter, lm_iters, rejected, cg_iters, converged;
    double initial_cost, final_cost, lambda;
    int abstol_hits, pad_; /* this file's own: how often abstol raised d0 to the carried residual */
} spa2d_ref_stats;

enum { REF_OK = 0, REF_NO_FIXED = 1, REF_DISCONNECTED = 2 };

static void mul33(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
static void mv3(const double *A, const double *v, double *o)
{
    for (int i = 0; i < 3; ++i) o[i] = (A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2];
}
static void mtv3(const double *A, const double *v, double *o)
{
    for (int j = 0; j < 3; ++j) o[j] = (A[j] * v[0] + A[3 + j] * v[1]) + A[6 + j] * v[2];
}
static void tr33(const double *A, double *T)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * j + i];
}
static double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* Matrix3d::inverse (bpcg.h:282): cofactors over det = (a*c00 + b*c10) + c*c20 */
static void inv33(const double *m, double *o)
{
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
    const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double det = (a * c00 + b * c10) + c * c20;
    o[0] = c00 / det; o[1] = c01 / det; o[2] = c02 / det;
    o[3] = c10 / det; o[4] = c11 / det; o[5] = c12 / det;
    o[6] = c20 / det; o[7] = c21 / det; o[8] = c22 / det;
}

/* The reduction shape: lane t sums terms t, t + 256, ... in ascending order onto +0.0, then the halving tree. */
static double reduce(const double *term, int count)
{
    double s[LANES];
    for (int t = 0; t < LANES; ++t) {
        double acc = 0.0;
        for (int i = t; i < count; i += LANES) acc += term[i];
        s[t] = acc;
    }
    for (int o = LANES / 2; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) s[t] = s[t] + s[t + o];
    return s[0];
}

typedef struct node {
    double trans[3], arot; /* trans(2) = 1 (spa2d.cpp:214) */
    double w2n[6], dRdx[4];
    double oldtrans[3], oldarot;
} node;

typedef struct con {
    int ndr, nd1;
    double tmean[2], amean, prec[9];
    double err[3], J0[9], J0t[9], J1[9], J1t[9];
} con;

/* Node2d::setTransform (spa2d.cpp:63-70) */
static void set_transform(node *nd)
{
    double *w = nd->w2n;
    w[0] = w[4] = sdm_cos(nd->arot);
    w[1] = sdm_sin(nd->arot);
    w[3] = -w[1];
    w[2] = w[5] = 0.0;
    const double c0 = -((w[0] * nd->trans[0] + w[1] * nd->trans[1]) + w[2] * nd->trans[2]);
    const double c1 = -((w[3] * nd->trans[0] + w[4] * nd->trans[1]) + w[5] * nd->trans[2]);
    w[2] = c0;
    w[5] = c1;
}
/* Node2d::setDr (:76-81) */
static void set_dr(node *nd)
{
    nd->dRdx[0] = nd->dRdx[3] = nd->w2n[3];
    nd->dRdx[1] = nd->w2n[0];
    nd->dRdx[2] = -nd->w2n[0];
}
/* Node2d::normArot (spa2d.h:106-110) */
static void norm_arot(node *nd)
{
    if (nd->arot > M_PI) nd->arot -= 2.0 * M_PI;
    if (nd->arot < -M_PI) nd->arot += 2.0 * M_PI;
}

/* Con2dP2::calcErr (:148-159) */
static double calc_err(con *c, const node *nd0, const node *nd1)
{
    const double *w = nd0->w2n, *t1 = nd1->trans;
    c->err[0] = ((w[0] * t1[0] + w[1] * t1[1]) + w[2] * t1[2]) - c->tmean[0];
    c->err[1] = ((w[3] * t1[0] + w[4] * t1[1]) + w[5] * t1[2]) - c->tmean[1];
    double aerr = (nd1->arot - nd0->arot) - c->amean;
    if (aerr > M_PI) aerr -= 2.0 * M_PI;
    if (aerr < -M_PI) aerr += 2.0 * M_PI;
    c->err[2] = aerr;
    double pe[3];
    mv3(c->prec, c->err, pe);
    return dot3(c->err, pe);
}

/* SysSPA2d::calcCost (:173-201), summed in the reduction shape */
static double calc_cost(con *cons, int m, const node *nodes, double *term)
{
    for (int i = 0; i < m; ++i) term[i] = calc_err(&cons[i], &nodes[cons[i].ndr], &nodes[cons[i].nd1]);
    return reduce(term, m);
}

/* Con2dP2::setJacobians (:86-142) */
static void set_jacobians(con *c, const node *nodes)
{
    const node *nr = &nodes[c->ndr], *n1 = &nodes[c->nd1];
    const double *w = nr->w2n;
    const double pwt[2] = {n1->trans[0] - nr->trans[0], n1->trans[1] - nr->trans[1]};
    const double dp0 = nr->dRdx[0] * pwt[0] + nr->dRdx[1] * pwt[1];
    const double dp1 = nr->dRdx[2] * pwt[0] + nr->dRdx[3] * pwt[1];
    const double J0[9] = {-w[0], -w[1], dp0, -w[3], -w[4], dp1, 0.0, 0.0, -1.0};
    const double J1[9] = {w[0], w[1], 0.0, w[3], w[4], 0.0, 0.0, 0.0, 1.0};
    memcpy(c->J0, J0, sizeof(J0));
    memcpy(c->J1, J1, sizeof(J1));
    tr33(c->J0, c->J0t);
    tr33(c->J1, c->J1t);
}

/* cols[] of CSparse2d: per column jj, its blocks keyed by row ii < jj, kept sorted by ii (a std::map). */
typedef struct blk {
    int ri;
    double m[9];
} blk;
typedef struct column {
    blk *b;
    int n, cap;
} column;

/* CSparse2d::addOffdiagBlock (csparse.cpp:472-485) */
static void add_offdiag(column *cols, const double *m, int ii, int jj)
{
    column *col = &cols[jj];
    int pos = 0;
    while (pos < col->n && col->b[pos].ri < ii) ++pos;
    if (pos < col->n && col->b[pos].ri == ii) { /* found it, add */
        for (int q = 0; q < 9; ++q) col->b[pos].m[q] += m[q];
        return;
    }
    if (col->n == col->cap) {
        col->cap = col->cap ? 2 * col->cap : 4;
        col->b = (blk *)realloc(col->b, sizeof(blk) * (size_t)col->cap);
    }
    memmove(&col->b[pos + 1], &col->b[pos], sizeof(blk) * (size_t)(col->n - pos));
    col->b[pos].ri = ii; /* didn't find it: insert a copy */
    memcpy(col->b[pos].m, m, sizeof(double) * 9);
    ++col->n;
}

/* jacobiBPCG<3>::mMV2 (bpcg.h:142-161) over the linear storage vcind / vrind / vcols */
static void mmv2(const double *diag, int nfree, const int *vcind, const int *vrind, const double *vcols, int nblk,
                 const double *vin, double *vout)
{
    for (int i = 0; i < nfree; ++i) mv3(diag + 9 * i, vin + 3 * i, vout + 3 * i);
    for (int i = 0; i < nblk; ++i) {
        const int ri = vrind[i], ii = vcind[i];
        const double *M = vcols + 9 * i;
        double u[3];
        mv3(M, vin + 3 * ii, u);
        for (int q = 0; q < 3; ++q) vout[3 * ri + q] += u[q];
        mtv3(M, vin + 3 * ri, u);
        for (int q = 0; q < 3; ++q) vout[3 * ii + q] += u[q];
    }
}

static double vdot(const double *a, const double *b, int nfree, double *term)
{
    for (int i = 0; i < nfree; ++i) term[i] = dot3(a + 3 * i, b + 3 * i);
    return reduce(term, nfree);
}

/* poses [n][3] in and out; ends [m][2] node indices; means [m][3]; precs [m][9] row-major. */
int spa2d_ref_compute(int n, double *poses, int m, const int *ends, const double *means, const double *precs,
                      int n_fixed, int niter, double sLambda, double initTol, int maxCGiters, spa2d_ref_stats *st)
{
    memset(st, 0, sizeof(*st));
    st->lambda = sLambda;
    /* check for fixed frames (:435-439) */
    if (n_fixed <= 0) {
        st->status = REF_NO_FIXED;
        return 0;
    }
    const int nFixed = n_fixed < n ? n_fixed : n;
    const int nFree = n - nFixed;
    /* a free node without a constraint (dcnt, :407-412): refused here */
    {
        int *dcnt = (int *)calloc((size_t)(nFree > 0 ? nFree : 1), sizeof(int));
        for (int i = 0; i < m; ++i) {
            if (ends[2 * i] >= nFixed) dcnt[ends[2 * i] - nFixed]++;
            if (ends[2 * i + 1] >= nFixed) dcnt[ends[2 * i + 1] - nFixed]++;
        }
        int ndc = 0;
        for (int i = 0; i < nFree; ++i)
            if (dcnt[i] == 0) ndc++;
        free(dcnt);
        if (ndc > 0) {
            st->status = REF_DISCONNECTED;
            return 0;
        }
    }
    const size_t nf = (size_t)(nFree > 0 ? nFree : 1), mm = (size_t)(m > 0 ? m : 1);
    node *nodes = (node *)calloc((size_t)(n > 0 ? n : 1), sizeof(node));
    con *cons = (con *)calloc(mm, sizeof(con));
    double *term = (double *)calloc(nf > mm ? nf : mm, sizeof(double));
    double *diag = (double *)calloc(nf * 9, sizeof(double)), *J = (double *)calloc(nf * 9, sizeof(double));
    double *B = (double *)calloc(nf * 3, sizeof(double)), *x = (double *)calloc(nf * 3, sizeof(double));
    double *r = (double *)calloc(nf * 3, sizeof(double)), *d = (double *)calloc(nf * 3, sizeof(double));
    double *q = (double *)calloc(nf * 3, sizeof(double)), *s = (double *)calloc(nf * 3, sizeof(double));
    column *cols = (column *)calloc(nf, sizeof(column));
    int *vcind = (int *)calloc(mm, sizeof(int)), *vrind = (int *)calloc(mm, sizeof(int));
    double *vcols = (double *)calloc(mm * 9, sizeof(double));

    /* addNode (:207-222) */
    for (int i = 0; i < n; ++i) {
        nodes[i].arot = poses[3 * i + 2];
        nodes[i].trans[0] = poses[3 * i];
        nodes[i].trans[1] = poses[3 * i + 1];
        nodes[i].trans[2] = 1.0;
    }
    /* addConstraint (:243-250) */
    for (int i = 0; i < m; ++i) {
        cons[i].ndr = ends[2 * i];
        cons[i].nd1 = ends[2 * i + 1];
        cons[i].tmean[0] = means[3 * i];
        cons[i].tmean[1] = means[3 * i + 1];
        cons[i].amean = means[3 * i + 2];
        memcpy(cons[i].prec, precs + 9 * i, sizeof(double) * 9);
    }
    /* doSPA :440-449 */
    for (int i = 0; i < n; ++i) {
        set_transform(&nodes[i]);
        set_dr(&nodes[i]);
    }
    double lambda = sLambda; /* :452-453 (sLambda > 0 is the caller's duty) */
    double laminc = 2.0, lamdec = 0.5;
    int iter = 0;
    const double sqMinDelta = 1e-8 * 1e-8;
    double cost = calc_cost(cons, m, nodes, term);
    st->initial_cost = cost;
    int good_iter = 0;
    double residual = 0.0; /* jacobiBPCG::residual */

    for (; iter < niter; iter++) {
        st->lm_iters = iter + 1;
        /* ---- setupSparseSys (:328-413) */
        if (iter == 0) { /* setupBlockStructure(nFree): the columns are emptied (csparse.cpp:431-437) */
            for (int i = 0; i < nFree; ++i) cols[i].n = 0;
        }
        memset(B, 0, sizeof(double) * nf * 3); /* eraseit (:442-460): B, diag and the existing blocks to zero */
        memset(diag, 0, sizeof(double) * nf * 9);
        for (int i = 0; i < nFree; ++i)
            for (int j = 0; j < cols[i].n; ++j) memset(cols[i].b[j].m, 0, sizeof(double) * 9);
        const double lam = 1.0 + lambda;
        for (int pi = 0; pi < m; pi++) {
            con *c = &cons[pi];
            set_jacobians(c, nodes);
            const int i0 = c->ndr - nFixed, i1 = c->nd1 - nFixed;
            double T[9], mblk[9], tp[9], v[3];
            if (i0 >= 0) {
                mul33(c->J0t, c->prec, T);
                mul33(T, c->J0, mblk); /* J0t*prec*J0 (:362) */
                for (int k = 0; k < 9; ++k) diag[9 * i0 + k] += mblk[k];
            }
            if (i1 >= 0) {
                mul33(c->prec, c->J1, tp);  /* :369 */
                mul33(c->J1t, tp, mblk);    /* :370 */
                for (int k = 0; k < 9; ++k) diag[9 * i1 + k] += mblk[k];
                if (i0 >= 0) {
                    double m2[9];
                    mul33(c->J0t, tp, m2); /* :374 */
                    if (i1 < i0) {
                        tr33(m2, mblk);
                        add_offdiag(cols, mblk, i1, i0);
                    } else {
                        add_offdiag(cols, m2, i0, i1);
                    }
                }
            }
            if (i0 >= 0) { /* :388-389 */
                mul33(c->J0t, c->prec, T);
                mv3(T, c->err, v);
                for (int k = 0; k < 3; ++k) B[3 * i0 + k] -= v[k];
            }
            if (i1 >= 0) { /* :390-391 */
                mul33(c->J1t, c->prec, T);
                mv3(T, c->err, v);
                for (int k = 0; k < 3; ++k) B[3 * i1 + k] -= v[k];
            }
        }
        /* incDiagBlocks (csparse.cpp:488-492) */
        for (int i = 0; i < nFree; ++i) {
            diag[9 * i] *= lam;
            diag[9 * i + 4] *= lam;
            diag[9 * i + 8] *= lam;
        }
        /* ---- doBPCG (csparse.cpp:737-749), when B has rows (spa2d.cpp:485) */
        if (nFree > 0) {
            const int abstol = iter > 0;
            memset(x, 0, sizeof(double) * nf * 3);
            /* doBPCG2 (bpcg.h:255-276): the linear storage, columns ascending, rows ascending within */
            int nblk = 0;
            for (int i = 0; i < nFree; ++i)
                for (int j = 0; j < cols[i].n; ++j) {
                    vrind[nblk] = cols[i].b[j].ri;
                    vcind[nblk] = i;
                    memcpy(vcols + 9 * nblk, cols[i].b[j].m, sizeof(double) * 9);
                    ++nblk;
                }
            for (int i = 0; i < nFree; ++i) inv33(diag + 9 * i, J + 9 * i); /* :278-282 */
            memcpy(r, B, sizeof(double) * nf * 3);                            /* r = b */
            for (int i = 0; i < nFree; ++i) mv3(J + 9 * i, r + 3 * i, d + 3 * i); /* mD(J,r,d) */
            double dn = vdot(r, d, nFree, term);
            double d0 = initTol * dn;
            if (abstol) {
                if (residual > d0) {
                    d0 = residual;
                    st->abstol_hits++;
                }
            }
            int i;
            for (i = 0; i < maxCGiters; i++) {
                if (dn < d0) break;
                mmv2(diag, nFree, vcind, vrind, vcols, nblk, d, q);
                const double a = dn / vdot(d, q, nFree, term);
                for (int k = 0; k < 3 * nFree; ++k) x[k] = x[k] + a * d[k];
                for (int k = 0; k < 3 * nFree; ++k) r[k] = r[k] - a * q[k];
                for (int k = 0; k < nFree; ++k) mv3(J + 9 * k, r + 3 * k, s + 3 * k);
                const double dold = dn;
                dn = vdot(r, s, nFree, term);
                const double ba = dn / dold;
                for (int k = 0; k < 3 * nFree; ++k) d[k] = s[k] + ba * d[k];
            }
            residual = dn / 2.0;
            st->cg_iters += i;
            memcpy(B, x, sizeof(double) * nf * 3); /* B = x (csparse.cpp:747) */
        }
        /* ---- convergence (:523-529) */
        const double sqDiff = vdot(B, B, nFree, term);
        if (sqDiff < sqMinDelta) {
            st->converged = 1;
            break;
        }
        /* ---- update the frames (:532-546) */
        int ci = 0;
        for (int i = nFixed; i < n; i++) {
            node *nd = &nodes[i];
            memcpy(nd->oldtrans, nd->trans, sizeof(nd->trans));
            nd->oldarot = nd->arot;
            nd->trans[0] += B[ci];
            nd->trans[1] += B[ci + 1];
            nd->arot += B[ci + 2];
            norm_arot(nd);
            set_transform(nd);
            set_dr(nd);
            ci += 3;
        }
        const double newcost = calc_cost(cons, m, nodes, term);
        if (newcost < cost) { /* :555-561 */
            cost = newcost;
            lambda *= lamdec;
            good_iter++;
        } else { /* :562-582 */
            lambda *= laminc;
            laminc *= 2.0;
            for (int i = nFixed; i < n; i++) {
                node *nd = &nodes[i];
                memcpy(nd->trans, nd->oldtrans, sizeof(nd->trans));
                nd->arot = nd->oldarot;
                set_transform(nd);
                set_dr(nd);
            }
            cost = calc_cost(cons, m, nodes, term);
            st->rejected++;
        }
    }
    st->good_iter = good_iter;
    st->final_cost = cost;
    st->lambda = lambda;
    for (int i = 0; i < n; ++i) {
        poses[3 * i] = nodes[i].trans[0];
        poses[3 * i + 1] = nodes[i].trans[1];
        poses[3 * i + 2] = nodes[i].arot;
    }
    for (int i = 0; i < nFree; ++i) free(cols[i].b);
    free(nodes); free(cons); free(term); free(diag); free(J); free(B); free(x); free(r); free(d); free(q); free(s);
    free(cols); free(vcind); free(vrind); free(vcols);
    return good_iter;
}
