/* tests/ref/spa2d_chol_ref.c -- sequential CPU restatement of SysSPA2d::doSPA with the direct envelope Cholesky
 * solve that include/slam2d/spa.h states ("The direct solve") in place of csp.doChol() (lesson6/lib/
 * sparse_bundle_adjustment/src/spa2d.cpp:501-509).  Test infrastructure: the package never loads it.
 *
 * Everything outside the linear solve is spa2d_ref.c's, included below for its static functions: setTransform,
 * calcErr, setJacobians, the scatter of setupSparseSys into diag / cols / B, incDiagBlocks, the update, the cost and
 * the accept / undo rule.  The solve is written scalar by scalar and row by row (up-looking), the header's
 * sentences one after the other; the kernel factors by block column with a lane per row, and that the two give the
 * same bits is what the GPU tests check.
 *
 * SuiteSparse is absent: cs_cholsol's up-looking reach order, its AMD permutation (csize > 100,
 * csparse.cpp:722-726) and CHOLMOD are unpinned.  Build: gcc -O2 -ffp-contract=off.
 */
#include <math.h>

#include "spa2d_ref.c"

enum { REF_NOT_POSDEF = 3, REF_FACTOR_RANGE = 4 };

/* Scalar row i = 3k + c of the envelope spans the columns 3 first[k] ... i; off[i] is where it starts in the packed
 * array.  Returns the packed length; off has 3 nb + 1 entries. */
static long long env_offsets(int nb, const int *first, long long *off)
{
    long long run = 0;
    for (int k = 0; k < nb; ++k)
        for (int c = 0; c < 3; ++c) {
            off[3 * k + c] = run;
            run += 3 * (long long)(k - first[k]) + c + 1;
        }
    off[3 * nb] = run;
    return run;
}

long long spa2d_chol_env_len(int nb, const int *first)
{
    long long run = 0;
    for (int k = 0; k < nb; ++k) run += 9 * (long long)(k - first[k]) + 6;
    return run;
}

/* The direct solve on nb block rows: env holds A's envelope (packed scalar rows) and receives L; b [3 nb]; x [3 nb].
 * Returns 1, or 0 when a pivot was not > 0 (env then holds the rows factored so far, x is not written). */
int spa2d_chol_solve(int nb, const int *first, double *env, const double *b, double *x)
{
    const int n = 3 * nb;
    long long *off = (long long *)malloc(sizeof(long long) * (size_t)(n + 1));
    double *y = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    int ok = 1;
    env_offsets(nb, first, off);
#define START(i) (3 * first[(i) / 3])
#define EL(i, j) env[off[i] + ((j) - START(i))]
    /* factor A = L L': for row i and column j <= i inside the envelope */
    for (int i = 0; i < n && ok; ++i) {
        const int si = START(i);
        for (int j = si; j <= i; ++j) {
            const int sj = START(j);
            double v = EL(i, j);
            for (int m = si > sj ? si : sj; m < j; ++m) v = v - EL(i, m) * EL(j, m);
            if (j < i) {
                EL(i, j) = v / EL(j, j);
            } else {
                if (!(v > 0.0)) { /* zero, negative or NaN */
                    ok = 0;
                    break;
                }
                EL(i, i) = sqrt(v);
            }
        }
    }
    if (ok) {
        /* forward: y(i) = (b(i) - sum L(i, m) y(m)) / L(i, i), m ascending from start_i */
        for (int i = 0; i < n; ++i) {
            double v = b[i];
            for (int m = START(i); m < i; ++m) v = v - EL(i, m) * y[m];
            y[i] = v / EL(i, i);
        }
        /* backward: x(i) = (y(i) - sum L(m, i) x(m)) / L(i, i), over the rows m > i with start_m <= i, descending */
        for (int i = n - 1; i >= 0; --i) {
            double v = y[i];
            for (int m = n - 1; m > i; --m)
                if (START(m) <= i) v = v - EL(m, i) * x[m];
            x[i] = v / EL(i, i);
        }
    }
#undef EL
#undef START
    free(off);
    free(y);
    return ok;
}

/* first[] over the free nodes (free index k - nFixed): the smallest free neighbour when that is lower, else k. */
void spa2d_chol_first(int n, int m, const int *ends, int n_fixed, int *first)
{
    const int nFixed = n_fixed < n ? n_fixed : n;
    for (int k = 0; k < n - nFixed; ++k) first[k] = k;
    for (int i = 0; i < m; ++i) {
        const int a = ends[2 * i] - nFixed, b = ends[2 * i + 1] - nFixed;
        if (a < 0 || b < 0) continue;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        if (lo < first[hi]) first[hi] = lo;
    }
}

/* As spa2d_ref_compute, with the direct solve.  max_factor_blocks < 0: no capacity check. */
int spa2d_chol_ref_compute(int n, double *poses, int m, const int *ends, const double *means, const double *precs,
                           int n_fixed, int niter, double sLambda, long long max_factor_blocks, spa2d_ref_stats *st)
{
    memset(st, 0, sizeof(*st));
    st->lambda = sLambda;
    if (n_fixed <= 0) { /* :435-439 */
        st->status = REF_NO_FIXED;
        return 0;
    }
    const int nFixed = n_fixed < n ? n_fixed : n;
    const int nFree = n - nFixed;
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
    int *first = (int *)calloc(nf, sizeof(int));
    spa2d_chol_first(n, m, ends, n_fixed, first);
    {
        long long blocks = 0;
        for (int k = 0; k < nFree; ++k) blocks += k - first[k] + 1;
        if (max_factor_blocks >= 0 && blocks > max_factor_blocks) {
            st->status = REF_FACTOR_RANGE;
            free(first);
            return 0;
        }
    }
    long long *off = (long long *)calloc(3 * nf + 1, sizeof(long long));
    const long long env_len = env_offsets(nFree, first, off);
    double *env = (double *)calloc((size_t)(env_len > 0 ? env_len : 1), sizeof(double));
    node *nodes = (node *)calloc((size_t)(n > 0 ? n : 1), sizeof(node));
    con *cons = (con *)calloc(mm, sizeof(con));
    double *term = (double *)calloc(nf > mm ? nf : mm, sizeof(double));
    double *diag = (double *)calloc(nf * 9, sizeof(double));
    double *B = (double *)calloc(nf * 3, sizeof(double)), *x = (double *)calloc(nf * 3, sizeof(double));
    column *cols = (column *)calloc(nf, sizeof(column));

    for (int i = 0; i < n; ++i) { /* addNode (:207-222) */
        nodes[i].arot = poses[3 * i + 2];
        nodes[i].trans[0] = poses[3 * i];
        nodes[i].trans[1] = poses[3 * i + 1];
        nodes[i].trans[2] = 1.0;
    }
    for (int i = 0; i < m; ++i) { /* addConstraint (:243-250) */
        cons[i].ndr = ends[2 * i];
        cons[i].nd1 = ends[2 * i + 1];
        cons[i].tmean[0] = means[3 * i];
        cons[i].tmean[1] = means[3 * i + 1];
        cons[i].amean = means[3 * i + 2];
        memcpy(cons[i].prec, precs + 9 * i, sizeof(double) * 9);
    }
    for (int i = 0; i < n; ++i) { /* doSPA :440-449 */
        set_transform(&nodes[i]);
        set_dr(&nodes[i]);
    }
    double lambda = sLambda;
    double laminc = 2.0, lamdec = 0.5;
    int iter = 0;
    const double sqMinDelta = 1e-8 * 1e-8;
    double cost = calc_cost(cons, m, nodes, term);
    st->initial_cost = cost;
    int good_iter = 0;

    for (; iter < niter; iter++) {
        st->lm_iters = iter + 1;
        /* ---- setupSparseSys (:328-413), as in spa2d_ref.c */
        if (iter == 0)
            for (int i = 0; i < nFree; ++i) cols[i].n = 0;
        memset(B, 0, sizeof(double) * nf * 3);
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
                mul33(T, c->J0, mblk);
                for (int k = 0; k < 9; ++k) diag[9 * i0 + k] += mblk[k];
            }
            if (i1 >= 0) {
                mul33(c->prec, c->J1, tp);
                mul33(c->J1t, tp, mblk);
                for (int k = 0; k < 9; ++k) diag[9 * i1 + k] += mblk[k];
                if (i0 >= 0) {
                    double m2[9];
                    mul33(c->J0t, tp, m2);
                    if (i1 < i0) {
                        tr33(m2, mblk);
                        add_offdiag(cols, mblk, i1, i0);
                    } else {
                        add_offdiag(cols, m2, i0, i1);
                    }
                }
            }
            if (i0 >= 0) {
                mul33(c->J0t, c->prec, T);
                mv3(T, c->err, v);
                for (int k = 0; k < 3; ++k) B[3 * i0 + k] -= v[k];
            }
            if (i1 >= 0) {
                mul33(c->J1t, c->prec, T);
                mv3(T, c->err, v);
                for (int k = 0; k < 3; ++k) B[3 * i1 + k] -= v[k];
            }
        }
        for (int i = 0; i < nFree; ++i) { /* incDiagBlocks (csparse.cpp:488-492, :629) */
            diag[9 * i] *= lam;
            diag[9 * i + 4] *= lam;
            diag[9 * i + 8] *= lam;
        }
        /* ---- the direct solve: the upper triangle of the block system into the lower-triangular envelope */
        if (nFree > 0) {
            memset(env, 0, sizeof(double) * (size_t)env_len);
            for (int k = 0; k < nFree; ++k) {
                for (int c = 0; c < 3; ++c)
                    for (int c2 = 0; c2 <= c; ++c2)
                        env[off[3 * k + c] + (3 * k + c2 - 3 * first[k])] = diag[9 * k + 3 * c2 + c];
                for (int j = 0; j < cols[k].n; ++j) { /* column k: the blocks at (row ri < k, column k) */
                    const blk *bk = &cols[k].b[j];
                    for (int c = 0; c < 3; ++c)
                        for (int c2 = 0; c2 < 3; ++c2)
                            env[off[3 * k + c] + (3 * bk->ri + c2 - 3 * first[k])] = bk->m[3 * c2 + c];
                }
            }
            if (!spa2d_chol_solve(nFree, first, env, B, x)) {
                st->status = REF_NOT_POSDEF;
                break;
            }
            memcpy(B, x, sizeof(double) * nf * 3);
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
    free(first); free(off); free(env); free(nodes); free(cons); free(term); free(diag); free(B); free(x); free(cols);
    return good_iter;
}
