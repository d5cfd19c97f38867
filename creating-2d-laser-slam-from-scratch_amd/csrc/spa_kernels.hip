// spa_kernels.hip -- Karto's pose-graph optimiser on the device: SysSPA2d::doSPA in its block-Jacobi PCG mode
// (lesson6/lib/sparse_bundle_adjustment/src/spa2d.cpp:425-609 with useCSparse = SBA_BLOCK_JACOBIAN_PCG), and, as
// the kernel's second instantiation, with the direct envelope Cholesky solve include/slam2d/spa.h states in
// place of PCG (the node's doSPA(40) solves directly too, csp.doChol() spa2d.cpp:501-509).
//
// One 256-thread workgroup per graph runs the whole LM loop, PCG loops inside, in one launch: no grid-wide
// synchronisation, no cooperative launch, nothing waits on another workgroup.  A graph's working arrays live in
// its slice of the context's scratch (global memory, L2-resident at these sizes); LDS holds the 256 reduction
// lanes and the broadcast header.  Every value a barrier-enclosing branch or loop tests (dn < d0, sqDiff <
// sqMinDelta, newcost < cost, the iteration bounds, the graph's status) is the same on all lanes: it is read
// from LDS (the reduction's lane 0, the header) or computed from such values by the same operations.  NaN makes
// the comparisons false on every lane alike, so the loops end at their bounds.
//
// Arithmetic: IEEE double, -ffp-contract=off, in the orders include/slam2d/spa.h states; tests/ref/spa2d_ref.c
// restates the same sequence with the reference's scatter loops, and the two agree bit for bit; the direct solve
// is restated row by row in tests/ref/spa2d_chol_ref.c.
//
// The direct solve's schedule: the factor goes left-looking by block column j.  Phase A: one lane per row i >= j
// whose envelope reaches column j forms S = A(i, j) - sum over m < j of L(i, m) L(j, m)' (both rows' blocks are
// contiguous); lane 0, which owns row j, turns S(j, j) into L(j, j), solves the forward step y(j) -- the forward
// solve is the factor of the system bordered by b -- and leaves L(j, j) and the pivot flag in LDS.  Phase B: the
// lanes of the rows below divide by L(j, j)'.  Two barriers per block column.  The backward solve goes by block
// row m, descending: every lane forms x(m) from y(m) and L(m, m), then one lane per block of row m subtracts
// L(m, j)' x(m) from y(j); one barrier per row.  Each scalar's subtractions happen in the order spa.h states.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/slam2d/spa.h"
#include "detmath.h"
#include "graph_edit_device.h"

namespace s2d {

constexpr int SPA_THREADS = SPA_REDUCE_LANES;
constexpr int SPA_CON_DOUBLES = 33;  // per constraint: J0'KJ0 [9], J1'(KJ1) [9], the off-diagonal block [9], J0'Ke [3], J1'Ke [3]
// doubles of scratch per node / per constraint (spa_scratch_doubles)
constexpr int SPA_NODE_DOUBLES = 6 + 9 + 9 + 3 * 7;   // w2n, diag, inverse, B x r d q s, saved pose
constexpr int SPA_CONS_DOUBLES = SPA_CON_DOUBLES + 9;  // products, pair block

struct SpaHdr {
    int n_nodes, n_cons, n_pairs;
    int n_fixed;  // SysSPA2d::nFixed of this graph, or SPA_FIXED_FROM_PARAMS
};

// The context's device arrays; graph g owns [g * max_nodes, ...) / [g * max_cons, ...) of each.
struct SpaDev {
    int max_nodes, max_cons;
    const SpaHdr *hdr;        // [G]
    double *poses;            // [G][N][3]: x, y, heading -- persistent
    const int2 *con_nd;       // [G][M]: ndr, nd1 (node indices)
    const double *con_mean;   // [G][M][3]
    const double *con_prec;   // [G][M][9]
    const int *inc_off;       // [G][N + 1]: per node, its incident constraints in constraint order
    const int *inc;           // [G][2M]: constraint * 2 + end (0: the node is ndr, 1: it is nd1)
    const int *nbr_off;       // [G][N + 1]: per node, its off-diagonal neighbours in ascending node index
    const int2 *nbr;          // [G][2M]: neighbour node, pair
    const int *pair_off;      // [G][M + 1]: per unordered node pair, its constraints in constraint order
    const int *pair_con;      // [G][M]
    double *scratch;          // [G][spa_scratch_doubles]
    int max_fac;              // the direct solve's capacity per graph, in 3 x 3 blocks
    double *fac;              // [G][max_fac][9]: the envelope, row after row; block (i, j) row-major
    int *fidx;                // [G][spa_fidx_ints]: first [N], last [N], rowoff [N + 1] over the free nodes
    spa_stats *stats;         // [G]
};

// what the kernels that take their graphs from rows of device memory need besides: the refusals' two words
// (ge_refuse) and the call's number
struct SpaRows {
    unsigned long long *info;
    int max_graphs;
    unsigned seq;
};

__host__ __device__ inline size_t spa_scratch_doubles(int max_nodes, int max_cons)
{
    return (size_t)max_nodes * SPA_NODE_DOUBLES + (size_t)max_cons * SPA_CONS_DOUBLES;
}

__host__ __device__ inline size_t spa_fidx_ints(int max_nodes) { return (size_t)3 * max_nodes + 1; }

// C = A * B, each element (a0*b0 + a1*b1) + a2*b2
__device__ inline void spa_mul33(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ inline void spa_mv3(const double *A, const double *v, double *o)
{
    for (int i = 0; i < 3; ++i) o[i] = (A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2];
}
// o = A' * v
__device__ inline void spa_mtv3(const double *A, const double *v, double *o)
{
    for (int j = 0; j < 3; ++j) o[j] = (A[j] * v[0] + A[3 + j] * v[1]) + A[6 + j] * v[2];
}
__device__ inline void spa_tr33(const double *A, double *T)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * j + i];
}
__device__ inline double spa_dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Matrix3d::inverse (bpcg.h:282), order fixed here: cofactors divided by det = (a*c00 + b*c10) + c*c20
__device__ inline void spa_inv33(const double *m, double *o)
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

// Node2d::setTransform (spa2d.cpp:63-70); setDr (:76-81) is read off w2n: dRdx = [[w10, w00], [-w00, w10]]
__device__ inline void spa_set_transform(const double *pose, double *w)
{
    const double c = sdm_cos(pose[2]), s = sdm_sin(pose[2]);
    w[0] = c; w[1] = s; w[3] = -s; w[4] = c;
    // col(2) = -w2n * trans with col(2) zeroed first, trans = (x, y, 1): (w0*x + w1*y) + w2*t2
    w[2] = -((w[0] * pose[0] + w[1] * pose[1]) + 0.0 * 1.0);
    w[5] = -((w[3] * pose[0] + w[4] * pose[1]) + 0.0 * 1.0);
}

// Con2dP2::calcErr (spa2d.cpp:148-159): err, and the cost term err . (prec * err)
__device__ inline double spa_calc_err(const double *w0, const double *p0, const double *p1, const double *mean,
                                      const double *K, double *err)
{
    err[0] = ((w0[0] * p1[0] + w0[1] * p1[1]) + w0[2] * 1.0) - mean[0];
    err[1] = ((w0[3] * p1[0] + w0[4] * p1[1]) + w0[5] * 1.0) - mean[1];
    double aerr = (p1[2] - p0[2]) - mean[2];
    if (aerr > SDM_PI) aerr -= 2.0 * SDM_PI;
    if (aerr < -SDM_PI) aerr += 2.0 * SDM_PI;
    err[2] = aerr;
    double pe[3];
    spa_mv3(K, err, pe);
    return spa_dot3(err, pe);
}

// The fixed reduction shape (spa.h): the lanes' partial sums, then s[t] += s[t + 128], ..., s[0] += s[1].  Every
// lane returns lane 0's sum, read from LDS.
__device__ inline double spa_reduce(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = SPA_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// calcCost (spa2d.cpp:173-201): the sum over constraints, in the reduction shape
__device__ inline double spa_cost(int m, const int2 *nd, const double *mean, const double *prec, const double *w2n,
                                  const double *poses, double *red)
{
    double acc = 0.0;
    for (int ci = threadIdx.x; ci < m; ci += SPA_THREADS) {
        const int2 e = nd[ci];
        double err[3];
        acc += spa_calc_err(w2n + 6 * e.x, poses + 3 * e.x, poses + 3 * e.y, mean + 3 * ci, prec + 9 * ci, err);
    }
    return spa_reduce(acc, red);
}

// ---- the direct solve (spa.h "The direct solve"); indices are free-node indices f = k - nF

// first[], last[] and the row offsets of graph's envelope, once per compute.  last[j] is the largest row whose
// envelope reaches column j (>= j).  Returns the envelope's blocks, read from LDS: the same on every lane.  When
// they exceed cap, rowoff is not written.
__device__ inline long long spa_chol_setup(int nF, int nfree, int cap, const int *nbr_off, const int2 *nbr, int *first,
                                           int *last, int *rowoff, long long *lscan, int *iscan)
{
    const int t = threadIdx.x;
    for (int f = t; f < nfree; f += SPA_THREADS) {
        const int k = nF + f;
        int fi = f;
        for (int j = nbr_off[k]; j < nbr_off[k + 1]; ++j) {
            const int nb = nbr[j].x;
            if (nb >= nF) {
                if (nb < k) fi = nb - nF;
                break;
            }
        }
        first[f] = fi;
        last[f] = f;
    }
    __syncthreads();
    for (int f = t; f < nfree; f += SPA_THREADS) atomicMax(&last[first[f]], f);
    __syncthreads();
    // prefix sum of the widths and prefix maximum of last[]: lane t scans the segment [lo, hi)
    const int seg = (nfree + SPA_THREADS - 1) / SPA_THREADS;
    const int lo = t * seg < nfree ? t * seg : nfree, hi = lo + seg < nfree ? lo + seg : nfree;
    long long run = 0;
    int rmax = -1;
    for (int f = lo; f < hi; ++f) {
        run += f - first[f] + 1;
        rmax = last[f] > rmax ? last[f] : rmax;
    }
    lscan[t] = run;
    iscan[t] = rmax;
    __syncthreads();
    if (t == 0) {
        run = 0;
        rmax = -1;
        for (int q = 0; q < SPA_THREADS; ++q) {
            const long long v = lscan[q];
            const int w = iscan[q];
            lscan[q] = run;
            iscan[q] = rmax;
            run += v;
            rmax = w > rmax ? w : rmax;
        }
        lscan[SPA_THREADS] = run;
    }
    __syncthreads();
    const long long total = lscan[SPA_THREADS];
    if (total <= cap) {
        run = lscan[t];
        rmax = iscan[t];
        for (int f = lo; f < hi; ++f) {
            rowoff[f] = (int)run;
            run += f - first[f] + 1;
            rmax = last[f] > rmax ? last[f] : rmax;
            last[f] = rmax;
        }
        if (t == 0) rowoff[nfree] = (int)total;
    }
    __syncthreads();
    return total;
}

// The system into the envelope: zeros, then per free node the lower triangle of its diagonal block and the
// transposed pair blocks of its lower free neighbours.  Barriers before (diag, pblk) and after.
__device__ inline void spa_chol_assemble(int nF, int nfree, const int *first, const int *rowoff, const int *nbr_off,
                                         const int2 *nbr, const double *diag, const double *pblk, double *fac)
{
    const int t = threadIdx.x;
    __syncthreads();
    const size_t total = (size_t)9 * rowoff[nfree];
    for (size_t q = t; q < total; q += SPA_THREADS) fac[q] = 0.0;
    __syncthreads();
    for (int f = t; f < nfree; f += SPA_THREADS) {
        const int k = nF + f, fi = first[f];
        double *Lf = fac + (size_t)9 * rowoff[f];
        double *Dg = Lf + (size_t)9 * (f - fi);
        const double *A = diag + 9 * (size_t)k;
        for (int c = 0; c < 3; ++c)
            for (int c2 = 0; c2 <= c; ++c2) Dg[3 * c + c2] = A[3 * c2 + c];
        for (int j = nbr_off[k]; j < nbr_off[k + 1]; ++j) {
            const int2 nb = nbr[j];
            if (nb.x < nF) continue;
            if (nb.x >= k) break;
            double *Bk = Lf + (size_t)9 * (nb.x - nF - fi);
            const double *Pb = pblk + 9 * (size_t)nb.y;
            for (int c = 0; c < 3; ++c)
                for (int c2 = 0; c2 < 3; ++c2) Bk[3 * c + c2] = Pb[3 * c2 + c];
        }
    }
    __syncthreads();
}

// Factor in place, forward solve in place in y, backward solve into x.  ljj [6] (l00 l10 l11 l20 l21 l22) and bad
// are in LDS.  Returns false when a pivot was not > 0: the same on every lane, read from LDS.
__device__ inline bool spa_chol_solve(int nfree, const int *first, const int *last, const int *rowoff, double *fac,
                                      double *y, double *x, double *ljj, int *bad)
{
    const int t = threadIdx.x;
    for (int j = 0; j < nfree; ++j) {
        const int fj = first[j], lastj = last[j];
        const double *Lj = fac + (size_t)9 * rowoff[j];
        // phase A
        for (int i = j + t; i <= lastj; i += SPA_THREADS) {
            const int fi = first[i];
            if (fi > j) continue;
            double *Li = fac + (size_t)9 * rowoff[i];
            double *S = Li + (size_t)9 * (j - fi);
            double s[9];
            for (int q = 0; q < 9; ++q) s[q] = S[q];
            for (int m = fi > fj ? fi : fj; m < j; ++m) {
                const double *a = Li + (size_t)9 * (m - fi), *b = Lj + (size_t)9 * (m - fj);
                for (int c = 0; c < 3; ++c)
                    for (int c2 = 0; c2 < 3; ++c2)
                        for (int q = 0; q < 3; ++q) s[3 * c + c2] = s[3 * c + c2] - a[3 * c + q] * b[3 * c2 + q];
            }
            if (i == j) {  // lane 0: the pivots, then y(j)
                int nb = 0;
                double v = s[0];
                if (!(v > 0.0)) nb = 1;
                const double l00 = sqrt(v);
                const double l10 = s[3] / l00, l20 = s[6] / l00;
                v = s[4] - l10 * l10;
                if (!(v > 0.0)) nb = 1;
                const double l11 = sqrt(v);
                const double l21 = (s[7] - l20 * l10) / l11;
                v = s[8] - l20 * l20;
                v = v - l21 * l21;
                if (!(v > 0.0)) nb = 1;
                const double l22 = sqrt(v);
                double yv[3] = {y[3 * j], y[3 * j + 1], y[3 * j + 2]};
                for (int m = fj; m < j; ++m) {
                    const double *b = Lj + (size_t)9 * (m - fj), *ym = y + 3 * (size_t)m;
                    for (int c = 0; c < 3; ++c)
                        for (int q = 0; q < 3; ++q) yv[c] = yv[c] - b[3 * c + q] * ym[q];
                }
                yv[0] = yv[0] / l00;
                yv[1] = (yv[1] - l10 * yv[0]) / l11;
                yv[2] = ((yv[2] - l20 * yv[0]) - l21 * yv[1]) / l22;
                for (int q = 0; q < 3; ++q) y[3 * j + q] = yv[q];
                s[0] = l00; s[1] = 0.0; s[2] = 0.0;
                s[3] = l10; s[4] = l11; s[5] = 0.0;
                s[6] = l20; s[7] = l21; s[8] = l22;
                ljj[0] = l00; ljj[1] = l10; ljj[2] = l11; ljj[3] = l20; ljj[4] = l21; ljj[5] = l22;
                *bad = nb;
            }
            for (int q = 0; q < 9; ++q) S[q] = s[q];
        }
        __syncthreads();
        if (*bad) return false;
        // phase B: L(i, j) = S(i, j) / L(j, j)'
        const double l00 = ljj[0], l10 = ljj[1], l11 = ljj[2], l20 = ljj[3], l21 = ljj[4], l22 = ljj[5];
        for (int i = j + 1 + t; i <= lastj; i += SPA_THREADS) {
            const int fi = first[i];
            if (fi > j) continue;
            double *S = fac + (size_t)9 * rowoff[i] + (size_t)9 * (j - fi);
            for (int c = 0; c < 3; ++c) {
                const double x0 = S[3 * c] / l00;
                const double x1 = (S[3 * c + 1] - x0 * l10) / l11;
                const double x2 = ((S[3 * c + 2] - x0 * l20) - x1 * l21) / l22;
                S[3 * c] = x0;
                S[3 * c + 1] = x1;
                S[3 * c + 2] = x2;
            }
        }
        __syncthreads();
    }
    for (int m = nfree - 1; m >= 0; --m) {
        const int fm = first[m];
        const double *Lm = fac + (size_t)9 * rowoff[m];
        const double *Dg = Lm + (size_t)9 * (m - fm);
        const double x2 = y[3 * m + 2] / Dg[8];
        const double x1 = (y[3 * m + 1] - Dg[7] * x2) / Dg[4];
        const double x0 = ((y[3 * m] - Dg[6] * x2) - Dg[3] * x1) / Dg[0];
        if (t == 0) {
            x[3 * m] = x0;
            x[3 * m + 1] = x1;
            x[3 * m + 2] = x2;
        }
        for (int j = fm + t; j < m; j += SPA_THREADS) {
            const double *b = Lm + (size_t)9 * (j - fm);
            double *yj = y + 3 * (size_t)j;
            for (int c = 0; c < 3; ++c) yj[c] = ((yj[c] - b[6 + c] * x2) - b[3 + c] * x1) - b[c] * x0;
        }
        __syncthreads();
    }
    return true;
}

// graph_of NULL: workgroup b computes graph g_first + b.  Otherwise it computes graph graph_of[b] (rows of device
// memory, spa_compute_rows_device) unless the row names no graph or an earlier row names the same one
// (graph_edit_device.h's leader rule): such a workgroup leaves before it touches anything, all its lanes alike.
template <int SOLVER>
__global__ __launch_bounds__(SPA_THREADS) void spa_solve_kernel(SpaDev D, int g_first, const int *__restrict__ graph_of,
                                                                 SpaRows R, spa_params P)
{
    __shared__ double red[SPA_THREADS];
    __shared__ int bc[5];
    constexpr bool CHOL = SOLVER == SPA_SOLVER_CHOLESKY;
    __shared__ long long lscan[CHOL ? SPA_THREADS + 1 : 1];
    __shared__ int iscan[CHOL ? SPA_THREADS : 1];
    __shared__ double ljj[CHOL ? 6 : 1];
    const int t = threadIdx.x;
    int g = g_first + blockIdx.x;
    if (graph_of) {
        g = graph_of[blockIdx.x];
        static_assert(SPA_THREADS == GE_THREADS, "ge_is_leader strides by GE_THREADS");
        const bool lead = ge_is_leader(graph_of, sizeof(int), blockIdx.x, g);
        if (g >= R.max_graphs && t == 0) ge_refuse(R.info, R.seq, blockIdx.x, SPA_EINVAL);
        if (g < 0 || g >= R.max_graphs || !lead) return;
    }
    const size_t N = (size_t)D.max_nodes, M = (size_t)D.max_cons;

    if (t == 0) {
        const SpaHdr h = D.hdr[g];
        bc[0] = h.n_nodes;
        bc[1] = h.n_cons;
        bc[2] = h.n_pairs;
        bc[3] = 0;
        bc[4] = h.n_fixed == SPA_FIXED_FROM_PARAMS ? P.n_fixed : h.n_fixed;
    }
    __syncthreads();
    const int n = bc[0], m = bc[1], npairs = bc[2], n_fixed = bc[4];
    const int nF = n_fixed < n ? n_fixed : n;  // nodes [0, nF) are fixed
    const int nfree = n - nF;

    double *poses = D.poses + g * N * 3;
    const int2 *con_nd = D.con_nd + g * M;
    const double *con_mean = D.con_mean + g * M * 3;
    const double *con_prec = D.con_prec + g * M * 9;
    const int *inc_off = D.inc_off + g * (N + 1);
    const int *inc = D.inc + g * 2 * M;
    const int *nbr_off = D.nbr_off + g * (N + 1);
    const int2 *nbr = D.nbr + g * 2 * M;
    const int *pair_off = D.pair_off + g * (M + 1);
    const int *pair_con = D.pair_con + g * M;
    double *sc = D.scratch + g * spa_scratch_doubles(D.max_nodes, D.max_cons);
    double *w2n = sc;            sc += N * 6;
    double *diag = sc;           sc += N * 9;
    double *jinv = sc;           sc += N * 9;
    double *vB = sc;             sc += N * 3;
    double *vx = sc;             sc += N * 3;
    double *vr = sc;             sc += N * 3;
    double *vd = sc;             sc += N * 3;
    double *vq = sc;             sc += N * 3;
    double *vs = sc;             sc += N * 3;
    double *old = sc;            sc += N * 3;
    double *cs = sc;             sc += M * SPA_CON_DOUBLES;
    double *pblk = sc;

    spa_stats st;
    st.status = SPA_OK;
    st.good_iter = st.lm_iters = st.rejected = st.cg_iters = st.converged = 0;
    st.initial_cost = st.final_cost = 0.0;
    st.lambda = P.lambda;

    // "No fixed frames" (spa2d.cpp:435-439): nothing is touched
    if (n_fixed <= 0) {
        st.status = SPA_NO_FIXED;
        if (t == 0) D.stats[g] = st;
        return;
    }
    // a free node without a constraint (the dcnt count of setupSparseSys, spa2d.cpp:407-412): refused
    {
        int lone = 0;
        for (int i = t; i < nfree; i += SPA_THREADS) {
            const int k = nF + i;
            if (inc_off[k + 1] == inc_off[k]) lone = 1;
        }
        if (lone) bc[3] = 1;
        __syncthreads();
        if (bc[3]) {
            st.status = SPA_DISCONNECTED;
            if (t == 0) D.stats[g] = st;
            return;
        }
    }

    // the direct solve's envelope; one that does not fit the context's factor storage is refused
    int *first = D.fidx + g * spa_fidx_ints(D.max_nodes), *last = first + N, *rowoff = last + N;
    double *fac = D.fac + g * (size_t)D.max_fac * 9;
    if constexpr (CHOL) {
        if (spa_chol_setup(nF, nfree, D.max_fac, nbr_off, nbr, first, last, rowoff, lscan, iscan) > D.max_fac) {
            st.status = SPA_FACTOR_RANGE;
            if (t == 0) D.stats[g] = st;
            return;
        }
    }

    // doSPA :440-449: every node's world-to-node transform
    for (int k = t; k < n; k += SPA_THREADS) spa_set_transform(poses + 3 * k, w2n + 6 * k);
    __syncthreads();

    double lambda = P.lambda;  // :452-453
    double laminc = 2.0;       // :455
    const double lamdec = 0.5; // :456
    const double sqMinDelta = 1e-8 * 1e-8;  // :458
    double cost = spa_cost(m, con_nd, con_mean, con_prec, w2n, poses, red);  // :459
    st.initial_cost = cost;
    double residual = 0.0;  // jacobiBPCG::residual; read only when abstol, i.e. after this call has set it

    int iter = 0;
    for (; iter < P.niter; ++iter) {  // :466
        st.lm_iters = iter + 1;
        // ---- setupSparseSys (:328-413), per constraint: setJacobians (:86-142) and the products of :351-392
        for (int ci = t; ci < m; ci += SPA_THREADS) {
            const int2 e = con_nd[ci];
            const int k0 = e.x, k1 = e.y;
            const double *w = w2n + 6 * k0, *p0 = poses + 3 * k0, *p1 = poses + 3 * k1, *K = con_prec + 9 * ci;
            double err[3];
            spa_calc_err(w, p0, p1, con_mean + 3 * ci, K, err);  // con.err as the last calcCost left it
            // pwt = (t1 - tr).head(2); dp = dRdx * pwt
            const double pw0 = p1[0] - p0[0], pw1 = p1[1] - p0[1];
            const double dp0 = w[3] * pw0 + w[0] * pw1;
            const double dp1 = (-w[0]) * pw0 + w[3] * pw1;
            const double J0[9] = {-w[0], -w[1], dp0, -w[3], -w[4], dp1, 0.0, 0.0, -1.0};
            const double J1[9] = {w[0], w[1], 0.0, w[3], w[4], 0.0, 0.0, 0.0, 1.0};
            double J0t[9], J1t[9], T[9], tp[9];
            spa_tr33(J0, J0t);
            spa_tr33(J1, J1t);
            double *o = cs + (size_t)ci * SPA_CON_DOUBLES;
            const bool f0 = k0 >= nF, f1 = k1 >= nF;
            if (f0) {
                spa_mul33(J0t, K, T);      // J0t * prec
                spa_mul33(T, J0, o);       // ... * J0                         (:362)
                spa_mv3(T, err, o + 27);   // J0t * prec * err                 (:389)
            }
            if (f1) {
                spa_mul33(K, J1, tp);      // tp = prec * J1                   (:369)
                spa_mul33(J1t, tp, o + 9); // J1t * tp                         (:370)
                if (f0) {
                    double m2[9];
                    spa_mul33(J0t, tp, m2);  // J0t * tp                       (:374)
                    if (k1 < k0) spa_tr33(m2, o + 18);  // block (i1, i0)      (:375-379)
                    else
                        for (int q = 0; q < 9; ++q) o[18 + q] = m2[q];  // block (i0, i1) (:382)
                }
                spa_mul33(J1t, K, T);
                spa_mv3(T, err, o + 30);   // J1t * prec * err                 (:391)
            }
        }
        __syncthreads();
        // ---- per free node: addDiagBlock / B -= in constraint order (csparse.h:166-167, spa2d.cpp:389-391),
        // incDiagBlocks (csparse.cpp:488-492), the Jacobi preconditioner and PCG's start (bpcg.h:278-287)
        const double lam = 1.0 + lambda;  // :348
        double acc = 0.0;
        for (int i = t; i < nfree; i += SPA_THREADS) {
            const int k = nF + i;
            double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
            for (int j = inc_off[k]; j < inc_off[k + 1]; ++j) {
                const int ci = inc[j] >> 1, end = inc[j] & 1;
                const double *o = cs + (size_t)ci * SPA_CON_DOUBLES;
                for (int q = 0; q < 9; ++q) A[q] += o[9 * end + q];
                for (int q = 0; q < 3; ++q) b[q] -= o[27 + 3 * end + q];
            }
            A[0] *= lam; A[4] *= lam; A[8] *= lam;
            if constexpr (CHOL) {  // the direct solve reads the block and B only
                for (int q = 0; q < 9; ++q) diag[9 * k + q] = A[q];
                for (int q = 0; q < 3; ++q) vB[3 * k + q] = b[q];
                continue;
            }
            double Ji[9], dd[3];
            spa_inv33(A, Ji);
            spa_mv3(Ji, b, dd);  // r = b; mD(J, r, d)
            for (int q = 0; q < 9; ++q) {
                diag[9 * k + q] = A[q];
                jinv[9 * k + q] = Ji[q];
            }
            for (int q = 0; q < 3; ++q) {
                vB[3 * k + q] = b[q];
                vr[3 * k + q] = b[q];
                vd[3 * k + q] = dd[q];
                vx[3 * k + q] = 0.0;
            }
            acc += spa_dot3(b, dd);
        }
        // ---- per node pair with both ends free: addOffdiagBlock (csparse.cpp:472-485).  On a call's first
        // iteration the pair's first constraint is inserted as it is; later the blocks are zeroed (:445-459) and
        // every constraint is added, the first onto +0.0
        for (int p = t; p < npairs; p += SPA_THREADS) {
            const int j0 = pair_off[p], j1 = pair_off[p + 1];
            const int2 e = con_nd[pair_con[j0]];
            if ((e.x < e.y ? e.x : e.y) < nF) continue;
            double Bk[9];
            const double *o = cs + (size_t)pair_con[j0] * SPA_CON_DOUBLES + 18;
            for (int q = 0; q < 9; ++q) Bk[q] = iter == 0 ? o[q] : 0.0 + o[q];
            for (int j = j0 + 1; j < j1; ++j) {
                o = cs + (size_t)pair_con[j] * SPA_CON_DOUBLES + 18;
                for (int q = 0; q < 9; ++q) Bk[q] += o[q];
            }
            for (int q = 0; q < 9; ++q) pblk[9 * (size_t)p + q] = Bk[q];
        }
        if constexpr (CHOL) {
            // ---- the direct solve in place of doChol (spa2d.cpp:501-509): B -> y in place, the step into x; the
            // pivot flag lives in bc[3], free since the disconnected check
            if (nfree > 0) {
                spa_chol_assemble(nF, nfree, first, rowoff, nbr_off, nbr, diag, pblk, fac);
                if (!spa_chol_solve(nfree, first, last, rowoff, fac, vB + 3 * (size_t)nF, vx + 3 * (size_t)nF, ljj, &bc[3])) {
                    st.status = SPA_NOT_POSDEF;
                    break;
                }
            } else {
                __syncthreads();
            }
        } else
        // ---- doBPCG (csparse.cpp:737-749) -> doBPCG2 (bpcg.h:284-315); skipped when B has no rows (:485)
        if (nfree > 0) {
            double dn = spa_reduce(acc, red);  // r.dot(d); its barriers also publish d and the pair blocks
            double d0 = P.init_tol * dn;
            if (iter > 0) {  // abstol (csparse.cpp:743-744)
                if (residual > d0) d0 = residual;
            }
            int i = 0;
            for (; i < P.max_cg_iters; ++i) {
                if (dn < d0) break;
                // mMV2 (bpcg.h:142-161) as a gather: the diagonal block, then the neighbours in ascending index
                acc = 0.0;
                for (int f = t; f < nfree; f += SPA_THREADS) {
                    const int k = nF + f;
                    double q3[3], u[3];
                    spa_mv3(diag + 9 * k, vd + 3 * k, q3);
                    for (int j = nbr_off[k]; j < nbr_off[k + 1]; ++j) {
                        const int2 nb = nbr[j];
                        if (nb.x < nF) continue;
                        if (nb.x < k) spa_mtv3(pblk + 9 * (size_t)nb.y, vd + 3 * nb.x, u);  // vout(ii) += M' vin(ri)
                        else spa_mv3(pblk + 9 * (size_t)nb.y, vd + 3 * nb.x, u);            // vout(ri) += M vin(ii)
                        for (int q = 0; q < 3; ++q) q3[q] += u[q];
                    }
                    for (int q = 0; q < 3; ++q) vq[3 * k + q] = q3[q];
                    acc += spa_dot3(vd + 3 * k, q3);
                }
                const double a = dn / spa_reduce(acc, red);  // :300
                acc = 0.0;
                for (int f = t; f < nfree; f += SPA_THREADS) {
                    const int k = nF + f;
                    double r3[3], s3[3];
                    for (int q = 0; q < 3; ++q) {
                        vx[3 * k + q] = vx[3 * k + q] + a * vd[3 * k + q];  // x += a*d
                        r3[q] = vr[3 * k + q] - a * vq[3 * k + q];          // r -= a*q
                        vr[3 * k + q] = r3[q];
                    }
                    spa_mv3(jinv + 9 * k, r3, s3);  // mD(J, r, s)
                    for (int q = 0; q < 3; ++q) vs[3 * k + q] = s3[q];
                    acc += spa_dot3(r3, s3);
                }
                const double dold = dn;
                dn = spa_reduce(acc, red);  // :306
                const double ba = dn / dold;
                for (int f = t; f < nfree; f += SPA_THREADS) {
                    const int k = nF + f;
                    for (int q = 0; q < 3; ++q) vd[3 * k + q] = vs[3 * k + q] + ba * vd[3 * k + q];  // d = s + ba*d
                }
                __syncthreads();
            }
            residual = dn / 2.0;  // :314
            st.cg_iters += i;
        } else {
            __syncthreads();
        }
        // ---- B = x (csparse.cpp:747); sqDiff = BB.squaredNorm() (:523)
        acc = 0.0;
        for (int f = t; f < nfree; f += SPA_THREADS) {
            const int k = nF + f;
            acc += spa_dot3(vx + 3 * k, vx + 3 * k);
        }
        const double sqDiff = spa_reduce(acc, red);
        if (sqDiff < sqMinDelta) {  // :524-529
            st.converged = 1;
            break;
        }
        // ---- update the frames (:532-546)
        for (int f = t; f < nfree; f += SPA_THREADS) {
            const int k = nF + f;
            double *p = poses + 3 * k;
            for (int q = 0; q < 3; ++q) old[3 * k + q] = p[q];
            p[0] += vx[3 * k];
            p[1] += vx[3 * k + 1];
            double a = p[2] + vx[3 * k + 2];
            if (a > SDM_PI) a -= 2.0 * SDM_PI;  // normArot (spa2d.h:106-110)
            if (a < -SDM_PI) a += 2.0 * SDM_PI;
            p[2] = a;
            spa_set_transform(p, w2n + 6 * k);
        }
        __syncthreads();
        const double newcost = spa_cost(m, con_nd, con_mean, con_prec, w2n, poses, red);  // :549
        if (newcost < cost) {  // :555-561
            cost = newcost;
            lambda *= lamdec;
            st.good_iter++;
        } else {  // :562-582
            lambda *= laminc;
            laminc *= 2.0;
            for (int f = t; f < nfree; f += SPA_THREADS) {
                const int k = nF + f;
                double *p = poses + 3 * k;
                for (int q = 0; q < 3; ++q) p[q] = old[3 * k + q];
                spa_set_transform(p, w2n + 6 * k);
            }
            __syncthreads();
            cost = spa_cost(m, con_nd, con_mean, con_prec, w2n, poses, red);
            st.rejected++;
        }
    }
    st.final_cost = cost;
    st.lambda = lambda;
    if (t == 0) D.stats[g] = st;
}

// =================================================================================================
// spa_edit_nodes_kernel / spa_edit_constraints_kernel: addNode and addConstraint on the device
// (graph_edit_device.h: one workgroup per row, the first row of a graph leads it; its wave 0 applies the graph's rows
// in row order, SpaGraph::find's "last node with the id" as a wave maximum).  New nodes only extend the offset lists.
// New constraints rebuild the six lists to SpaGraph::compile()'s bits:
//   inc      a stable bucket fill of the 2m constraint ends by node;
//   sweep 1  64 nodes at a time, each node's neighbour set as a bit map of max_nodes bits in LDS, set from its
//            incident list: the popcounts give its neighbour count, its count of neighbours above it (the pairs it
//            is the lower end of) and its count of constraints to nodes above it; prefix sums over the nodes give
//            nbr_off, each node's first pair and its first pair_con position ((lo, hi) order);
//   sweep 2  per incident entry whose other end is above the node: the pair is the node's first pair plus the
//            popcount rank of the other end among the bits above the node; pair_con's position is the node's first
//            position plus the entries to lower neighbours above the node plus the earlier entries to the same one,
//            both counted along the incident list, which is in constraint order; pair_off from each pair's first;
//   sweep 3  per incident entry: nbr[nbr_off + popcount rank of the other end] = (other end, the constraint's pair).
// The per-constraint pair and the three per-node counts live in the graph's slice of the solver's scratch, which no
// compute expects to survive.  LDS: max(max_nodes + 1 ints, 64 rows of ceil(max_nodes / 32) words and as many
// uint16 word prefixes) + a few hundred ints.
// =================================================================================================
constexpr int SPA_EDIT_TILE = 64;

struct SpaEdit {
    SpaHdr *hdr;
    double *poses;
    int *ids;  // [G][max_nodes]
    int2 *con_nd;
    double *con_mean, *con_prec;
    int *inc_off, *inc, *nbr_off;
    int2 *nbr;
    int *pair_off, *pair_con;
    double *scratch;
    unsigned long long *info;  // ge_refuse
    int N, M, G;
    unsigned seq;
};

__host__ __device__ inline int spa_edit_words(int max_nodes) { return (max_nodes + 31) / 32; }
__host__ __device__ inline size_t spa_edit_lds(int max_nodes)
{
    const size_t tile = (size_t)SPA_EDIT_TILE * spa_edit_words(max_nodes) * 6, fill = sizeof(int) * ((size_t)max_nodes + 1);
    return ((tile > fill ? tile : fill) + 15) / 16 * 16 + sizeof(int) * (GE_THREADS + GE_WAVES + SPA_EDIT_TILE + 4);
}

__device__ __forceinline__ int spa_wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// bits of row `bm` below bit j
__device__ __forceinline__ int spa_edit_rank(const unsigned *bm, const unsigned short *pre, int j)
{
    return (int)pre[j >> 5] + __popc(bm[j >> 5] & ((1u << (j & 31)) - 1u));
}

// One sweep over the nodes, SPA_EDIT_TILE at a time: the tile's bit maps (and word prefixes when PREFIX), then
// per_tile(k0, k1) by all lanes and per_entry(node, row, other end, position in inc) for every incident entry.
template <bool PREFIX, class PerTile, class PerEntry>
__device__ inline void spa_edit_sweep(int n, int W, const int *inc_off, const int *inc, const int2 *con_nd, unsigned *bm,
                                      unsigned short *pre, PerTile per_tile, PerEntry per_entry)
{
    const int t = threadIdx.x;
    for (int k0 = 0; k0 < n; k0 += SPA_EDIT_TILE) {
        const int k1 = min(k0 + SPA_EDIT_TILE, n);
        for (int i = t; i < SPA_EDIT_TILE * W; i += GE_THREADS) bm[i] = 0;
        __syncthreads();
        const int x0 = inc_off[k0], x1 = inc_off[k1];
        int k = 0, o = 0;
        // an entry's node: the last k with inc_off[k] <= x
        auto locate = [&](int x) {
            int lo = k0, hi = k1;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (inc_off[mid] <= x) lo = mid;
                else hi = mid;
            }
            k = lo;
            const int e = inc[x];
            const int2 c = con_nd[e >> 1];
            o = (e & 1) ? c.x : c.y;
        };
        for (int x = x0 + t; x < x1; x += GE_THREADS) {
            locate(x);
            atomicOr(&bm[(k - k0) * W + (o >> 5)], 1u << (o & 31));
        }
        __syncthreads();
        if (PREFIX) {
            if (t < k1 - k0) {
                int run = 0;
                for (int w = 0; w < W; ++w) {
                    pre[t * W + w] = (unsigned short)run;
                    run += __popc(bm[t * W + w]);
                }
            }
            __syncthreads();
        }
        per_tile(k0, k1);
        for (int x = x0 + t; x < x1; x += GE_THREADS) {
            locate(x);
            per_entry(k, k - k0, o, x);
        }
        __syncthreads();
    }
}

// all lanes of the leader: graph g's six lists from its n nodes and m constraints
__device__ inline void spa_edit_rebuild(const SpaEdit &E, int g, int n, int m, unsigned char *smem)
{
    const int t = threadIdx.x;
    const size_t N = (size_t)E.N, M = (size_t)E.M;
    const int W = spa_edit_words(E.N);
    const size_t tile = (size_t)SPA_EDIT_TILE * W * 6, fill = sizeof(int) * (N + 1);
    int *cur = (int *)smem;
    unsigned *bm = (unsigned *)smem;
    unsigned short *pre = (unsigned short *)(smem + (size_t)SPA_EDIT_TILE * W * 4);
    int *s_b = (int *)(smem + ((tile > fill ? tile : fill) + 15) / 16 * 16), *sw = s_b + GE_THREADS, *s_cnt = sw + GE_WAVES;
    const int2 *con_nd = E.con_nd + g * M;
    int *inc_off = E.inc_off + g * (N + 1), *inc = E.inc + g * 2 * M, *nbr_off = E.nbr_off + g * (N + 1);
    int2 *nbr = E.nbr + g * 2 * M;
    int *pair_off = E.pair_off + g * (M + 1), *pair_con = E.pair_con + g * M;
    int *pairidx = (int *)(E.scratch + g * spa_scratch_doubles(E.N, E.M));
    int *pb = pairidx + M, *cb = pb + (N + 1);

    ge_bucket_fill(
        n, 2 * m, cur, s_b, sw, inc_off,
        [&](int x) {
            const int2 c = con_nd[x >> 1];
            return (x & 1) ? c.y : c.x;
        },
        [&](int x, int pos) { inc[pos] = x; });
    __threadfence_block();
    __syncthreads();

    // sweep 1: the counts
    spa_edit_sweep<false>(
        n, W, inc_off, inc, con_nd, bm, pre,
        [&](int k0, int k1) {
            if (t < k1 - k0) {
                const int k = k0 + t;
                int total = 0, above = 0;
                for (int w = 0; w < W; ++w) {
                    const unsigned b = bm[t * W + w];
                    total += __popc(b);
                    if (w > (k >> 5)) above += __popc(b);
                    else if (w == (k >> 5)) above += __popc(b & ~((2u << (k & 31)) - 1u));
                }
                nbr_off[k] = total;
                pb[k] = above;
            }
        },
        [&](int, int, int, int) {});
    // and each node's constraints to nodes above it, counted over the incident entries
    for (int k0 = 0; k0 < n; k0 += SPA_EDIT_TILE) {
        const int k1 = min(k0 + SPA_EDIT_TILE, n);
        if (t < SPA_EDIT_TILE) s_cnt[t] = 0;
        __syncthreads();
        for (int x = inc_off[k0] + t; x < inc_off[k1]; x += GE_THREADS) {
            int lo = k0, hi = k1;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (inc_off[mid] <= x) lo = mid;
                else hi = mid;
            }
            const int e = inc[x];
            const int2 c = con_nd[e >> 1];
            if (((e & 1) ? c.x : c.y) > lo) atomicAdd(&s_cnt[lo - k0], 1);
        }
        __syncthreads();
        if (t < k1 - k0) cb[k0 + t] = s_cnt[t];
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    ge_exscan_array(nbr_off, n, sw);
    const int n_pairs = ge_exscan_array(pb, n, sw);
    ge_exscan_array(cb, n, sw);

    // sweep 2: pairs and pair_con
    spa_edit_sweep<true>(
        n, W, inc_off, inc, con_nd, bm, pre, [&](int, int) {},
        [&](int k, int row, int o, int x) {
            if (o <= k) return;
            const unsigned *b = bm + row * W;
            const unsigned short *p = pre + row * W;
            const int pair = pb[k] + spa_edit_rank(b, p, o) - spa_edit_rank(b, p, k + 1);
            int before = 0, same = 0;
            for (int y = inc_off[k]; y < inc_off[k + 1]; ++y) {
                const int e = inc[y];
                const int2 c = con_nd[e >> 1];
                const int oo = (e & 1) ? c.x : c.y;
                before += oo > k && oo < o;
                same += y < x && oo == o;
            }
            const int ci = inc[x] >> 1;
            pair_con[cb[k] + before + same] = ci;
            if (same == 0) pair_off[pair] = cb[k] + before;
            pairidx[ci] = pair;
        });
    if (t == 0) pair_off[n_pairs] = m;
    __threadfence_block();
    __syncthreads();

    // sweep 3: the neighbour lists
    spa_edit_sweep<true>(
        n, W, inc_off, inc, con_nd, bm, pre, [&](int, int) {},
        [&](int k, int row, int o, int x) {
            nbr[nbr_off[k] + spa_edit_rank(bm + row * W, pre + row * W, o)] = make_int2(o, pairidx[inc[x] >> 1]);
        });
    if (t == 0) {
        SpaHdr h = E.hdr[g];
        h.n_nodes = n;
        h.n_cons = m;
        h.n_pairs = n_pairs;
        E.hdr[g] = h;
    }
}

// a row that names no graph of the context: true when the workgroup is done with it
__device__ inline bool spa_edit_bad_row(const SpaEdit &E, int row, int g, int *added_out, int *status_out)
{
    if (g >= 0 && g < E.G) return false;
    if (threadIdx.x == 0) {
        if (added_out) added_out[row] = 0;
        if (status_out) status_out[row] = g < 0 ? SPA_OK : SPA_EINVAL;
        if (g >= 0) ge_refuse(E.info, E.seq, row, SPA_EINVAL);
    }
    return true;
}

__global__ void __launch_bounds__(GE_THREADS)
spa_edit_nodes_kernel(SpaEdit E, int count, const spa_node_row *__restrict__ rows, const int *__restrict__ mask,
                      int *__restrict__ status_out)
{
    const int row = blockIdx.x, lane = threadIdx.x & 63;
    const int g = rows[row].graph;
    if (spa_edit_bad_row(E, row, g, nullptr, status_out)) return;
    if (!ge_is_leader(rows, sizeof(spa_node_row), row, g)) return;
    if (threadIdx.x >= 64) return;  // wave 0 alone from here: no workgroup barrier below
    const size_t N = (size_t)E.N, M = (size_t)E.M;
    const int n0 = E.hdr[g].n_nodes;
    int n = n0;
    for (int base = row; base < count; base += 64) {
        const int j = base + lane;
        unsigned long long todo = __ballot(j < count && rows[j].graph == g);
        while (todo) {
            const int r = base + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            int st = SPA_OK;
            if (!mask || mask[r] == 1) {
                if (n >= E.N) {
                    st = SPA_ERANGE;
                } else {
                    if (lane == 0) E.ids[g * N + n] = rows[r].id;
                    if (lane < 3) E.poses[(g * N + n) * 3 + lane] = rows[r].pose[lane];
                    ++n;
                }
            }
            if (lane == 0) {
                if (status_out) status_out[r] = st;
                if (st != SPA_OK) ge_refuse(E.info, E.seq, r, st);
            }
        }
    }
    if (n == n0) return;
    // the new nodes have no constraint: their lists are empty
    int *inc_off = E.inc_off + g * (N + 1), *nbr_off = E.nbr_off + g * (N + 1);
    const int ie = n0 > 0 ? inc_off[n0] : 0, ne = n0 > 0 ? nbr_off[n0] : 0;
    for (int k = (n0 > 0 ? n0 + 1 : 0) + lane; k <= n; k += 64) {
        inc_off[k] = ie;
        nbr_off[k] = ne;
    }
    if (lane == 0) {
        if (n0 == 0) E.pair_off[g * (M + 1)] = 0;
        E.hdr[g].n_nodes = n;
    }
}

__global__ void __launch_bounds__(GE_THREADS)
spa_edit_constraints_kernel(SpaEdit E, int count, const spa_con_row *__restrict__ rows, const int *__restrict__ mask,
                            int *__restrict__ added_out, int *__restrict__ status_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char spa_edit_smem[];
    __shared__ int s_m;
    const int row = blockIdx.x, lane = threadIdx.x & 63;
    const int g = rows[row].graph;
    if (spa_edit_bad_row(E, row, g, added_out, status_out)) return;
    if (!ge_is_leader(rows, sizeof(spa_con_row), row, g)) return;
    const size_t N = (size_t)E.N, M = (size_t)E.M;
    const SpaHdr h = E.hdr[g];
    const int n = h.n_nodes, m0 = h.n_cons;
    if (threadIdx.x < 64) {
        const int *ids = E.ids + g * N;
        int m = m0;
        for (int base = row; base < count; base += 64) {
            const int j = base + lane;
            unsigned long long todo = __ballot(j < count && rows[j].graph == g);
            while (todo) {
                const int r = base + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                int st = SPA_OK, added = 0;
                if (!mask || mask[r] == 1) {
                    const int id0 = rows[r].id0, id1 = rows[r].id1;
                    if (id0 == id1) {
                        st = SPA_EINVAL;
                    } else {
                        int ni0 = -1, ni1 = -1;  // the LAST node with the id
                        for (int k = lane; k < n; k += 64) {
                            const int id = ids[k];
                            if (id == id0) ni0 = k;
                            if (id == id1) ni1 = k;
                        }
                        ni0 = spa_wave_max(ni0);
                        ni1 = spa_wave_max(ni1);
                        if (ni0 >= 0 && ni1 >= 0) {
                            if (ni0 == ni1) {
                                st = SPA_EINVAL;
                            } else if (m >= E.M) {
                                st = SPA_ERANGE;
                            } else {
                                if (lane == 0) E.con_nd[g * M + m] = make_int2(ni0, ni1);
                                if (lane < 3) E.con_mean[(g * M + m) * 3 + lane] = rows[r].mean[lane];
                                if (lane < 9) E.con_prec[(g * M + m) * 9 + lane] = rows[r].prec[lane];
                                ++m;
                                added = 1;
                            }
                        }
                    }
                }
                if (lane == 0) {
                    if (added_out) added_out[r] = added;
                    if (status_out) status_out[r] = st;
                    if (st != SPA_OK) ge_refuse(E.info, E.seq, r, st);
                }
            }
        }
        if (lane == 0) s_m = m;
    }
    __threadfence_block();
    __syncthreads();
    const int m = s_m;
    if (m == m0) return;
    spa_edit_rebuild(E, g, n, m, spa_edit_smem);
}

// =================================================================================================
// spa_export_kernel: the loop of MapperGraph::CorrectPoses (Mapper.cpp:1404-1411) for the graphs rows name
// =================================================================================================
// One workgroup per row.  For the nodes k = 0 .. n - 1 of graph g in node order, pool[offset[g] + id[k]] = pose[k], the
// three doubles moved as 64-bit words.  Ids that increase strictly (Karto's: a scan's id is its index) name every
// slot once, so all lanes copy; otherwise lane 0 copies in node order and a later node with an id wins.  An id < 0
// or a slot outside [0, pool_scans) is skipped and counted.
__global__ void __launch_bounds__(GE_THREADS)
spa_export_kernel(SpaDev D, SpaRows R, const int *__restrict__ ids, const int *__restrict__ graph_of,
                  const int *__restrict__ pool_offset, unsigned long long *__restrict__ pool, int pool_scans)
{
    const int t = threadIdx.x, row = blockIdx.x;
    const int g = graph_of[row];
    if (g < 0) return;
    if (g >= R.max_graphs) {
        if (t == 0) ge_refuse(R.info, R.seq, row, SPA_EINVAL);
        return;
    }
    const size_t N = (size_t)D.max_nodes;
    const int n = min(max(D.hdr[g].n_nodes, 0), D.max_nodes);
    const int *id = ids + g * N;
    const unsigned long long *src = (const unsigned long long *)(D.poses + g * N * 3);
    const long long off = pool_offset[g];
    int ordered = 1;
    for (int k = t; k + 1 < n; k += GE_THREADS) ordered &= id[k] < id[k + 1];
    ordered = __syncthreads_and(ordered);
    const auto copy = [&](int k) {
        const long long slot = off + id[k];
        if (id[k] < 0 || slot < 0 || slot >= pool_scans) {
            ge_refuse(R.info, R.seq, row, SPA_ERANGE);
            return;
        }
        for (int q = 0; q < 3; ++q) pool[3 * slot + q] = src[3 * (size_t)k + q];
    };
    if (ordered) {
        for (int k = t; k < n; k += GE_THREADS) copy(k);
    } else if (t == 0) {
        for (int k = 0; k < n; ++k) copy(k);
    }
}

}  // namespace s2d
