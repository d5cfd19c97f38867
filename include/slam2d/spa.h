/* include/slam2d/spa.h -- C-ABI of the MI355X Karto pose-graph optimiser (lesson6, config 5): SPA in its
 * block-Jacobi PCG mode, for a fleet of independent graphs.
 *
 * Reference: MapperGraph::CorrectPoses (lesson6/lib/open_karto/src/Mapper.cpp:1397-1414) calls
 * SpaSolver::Compute (lesson6/src/spa_solver/spa_solver.cc:43-61), which calls SysSPA2d::doSPA
 * (lesson6/lib/sparse_bundle_adjustment/src/spa2d.cpp:425-609).  This library runs
 *
 *     doSPA(niter, sLambda, SBA_BLOCK_JACOBIAN_PCG, initTol, maxCGiters)
 *
 * the mode whose arithmetic is all in the reference's own text (setupSparseSys spa2d.cpp:328-413,
 * CSparse2d::incDiagBlocks / doBPCG csparse.cpp:488-492, :737-749, jacobiBPCG<3>::doBPCG2 / mMV2
 * bpcg/bpcg.h:142-161, :237-316).  The node itself calls doSPA(40), whose default linear solver is sparse
 * Cholesky through CSparse / CHOLMOD, libraries outside the reference tree: that mode is NOT built.  Both
 * modes minimise the same cost; their iterates differ.
 *
 *   spa_add_node        SysSPA2d::addNode (spa2d.cpp:207-222)
 *   spa_add_constraint  SysSPA2d::addConstraint (spa2d.cpp:230-252)
 *   spa_compute[_device] doSPA for graphs [g_first, g_first + count), one workgroup per graph, one launch
 *   spa_get_nodes       what SpaSolver::Compute returns (spa_solver.cc:55-60): id, x, y, heading per node
 *
 * Eigen, SuiteSparse and boost are absent from this image, so the library is checked against the CPU
 * restatement tests/ref/spa2d_ref.c and parity with the compiled reference is UNPINNED, as for the matcher
 * (karto.h) and the grid (karto_grid.h).  The restatement fixes what Eigen leaves open, and the kernel
 * follows it bit for bit:
 *   - all arithmetic is IEEE double without FMA contraction; sin / cos are csrc/detmath.h's;
 *   - matrix products go left to right as the reference writes them; a 3-term dot is (a0*b0 + a1*b1) + a2*b2;
 *   - the 3 x 3 inverse is the cofactor matrix divided by det = (m00*c00 + m01*c10) + m02*c20;
 *   - every vector reduction (r.d, d.q, r.s, the step's squared norm, the cost) has ONE shape, SPA_REDUCE_LANES
 *     = 256 lanes: lane t adds the terms of free node (or constraint) t, t + 256, ... in ascending order onto
 *     +0.0, a node's term being its 3-term dot; then s[t] += s[t + 128], s[t] += s[t + 64], ..., s[0] += s[1].
 *
 * Conventions as in karto_grid.h: plain C types, int status (SPA_OK / negative), spa_last_error().  A pose
 * is double[3] = x, y, heading (rad); a precision matrix is double[9], row-major.
 */
#ifndef SLAM2D_SPA_H
#define SLAM2D_SPA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPA_OK 0
#define SPA_EINVAL (-1)
#define SPA_EHIP (-2)
#define SPA_ENOMEM (-3)
#define SPA_ENODEV (-4)
#define SPA_ERANGE (-5) /* more nodes or constraints than the context was created for */

/* per-graph status of a compute (spa_stats.status); the other graphs of the launch still run */
#define SPA_NOT_RUN (-100)   /* no compute has covered this graph yet */
#define SPA_NO_FIXED 1       /* n_fixed <= 0 (spa2d.cpp:435-439): 0 iterations, poses untouched */
#define SPA_DISCONNECTED 2   /* a free node has no constraint: refused, poses untouched (the reference prints
                                "disconnected nodes" and inverts a zero block) */

#define SPA_REDUCE_LANES 256
#define SPA_FIXED_FROM_PARAMS (-2147483647 - 1)
#define SPA_MAX_NITER 1000
#define SPA_MAX_CG_ITERS 65536
#define SPA_MAX_ITER_PRODUCT 1048576 /* niter * max_cg_iters: the kernel's run time is their product */

typedef struct spa_params {
    int niter;        /* LM iterations at most: 40 (spa_solver.cc:51) */
    int max_cg_iters; /* PCG iterations per LM iteration at most: 50 (spa2d.h:249) */
    int n_fixed;      /* the first n_fixed nodes stay put: 1 (spa2d.h:198) */
    int pad_;
    double lambda;    /* LM diagonal augmentation, re-initialised by every compute: 1e-4; must be > 0 */
    double init_tol;  /* PCG relative tolerance: 1e-8 */
} spa_params;

typedef struct spa_stats {
    int status;      /* SPA_OK, SPA_NO_FIXED, SPA_DISCONNECTED or SPA_NOT_RUN */
    int good_iter;   /* doSPA's return value: accepted steps */
    int lm_iters;    /* LM iterations begun (linear systems set up), the converging one included */
    int rejected;    /* steps undone because the cost did not fall */
    int cg_iters;    /* PCG iterations, all LM iterations together */
    int converged;   /* 1: ended by sqDiff < sqMinDelta (spa2d.cpp:523-529); 0: by niter */
    double initial_cost, final_cost; /* calcCost (spa2d.cpp:173-201) before the first and after the last step */
    double lambda;   /* the final lambda */
} spa_stats;

typedef struct spa_ctx spa_ctx;

const char *spa_last_error(void);
const char *spa_version(void);
void spa_default_params(spa_params *params);

/* A fleet of max_graphs graphs of up to max_nodes nodes and max_constraints constraints each, all device
 * resident.  Every graph starts empty. */
int spa_create(spa_ctx **out, int max_graphs, int max_nodes, int max_constraints);
int spa_destroy(spa_ctx *ctx);

/* addNode: appends a node; its index is the count before.  Ids need not be unique. */
int spa_add_node(spa_ctx *ctx, int g, int id, const double *pose);
/* addConstraint: looks both ids up over all nodes, the LAST node with an id winning.  *added = 1 when the
 * constraint was appended, 0 when an id is unknown (nothing added, still SPA_OK): the reference's bool.
 * id0 == id1 is SPA_EINVAL (Karto never makes one; added may be NULL). */
int spa_add_constraint(spa_ctx *ctx, int g, int id0, int id1, const double *mean, const double *prec, int *added);
/* Bulk form: replaces graph g by n_nodes nodes (ids, poses[n][3]) and n_cons constraints given by node INDEX
 * (ends int[n_cons][2], means[n_cons][3], precs[n_cons][9]). */
int spa_set_graph(spa_ctx *ctx, int g, int n_nodes, const int *ids, const double *poses, int n_cons, const int *ends, const double *means, const double *precs);
/* Empties graph g. */
int spa_clear_graph(spa_ctx *ctx, int g);
/* SysSPA2d::nFixed is a member of the system: graph g's own value, used instead of params->n_fixed by every
 * later compute.  SPA_FIXED_FROM_PARAMS (the initial state) goes back to params->n_fixed. */
int spa_set_n_fixed(spa_ctx *ctx, int g, int n_fixed);
int spa_get_counts(spa_ctx *ctx, int g, int *n_nodes, int *n_cons);

/* doSPA on graphs [g_first, g_first + count).  Poses persist: a later compute starts from the optimised
 * poses, as m_Spa does.  No solver state crosses calls (lambda is re-initialised, spa2d.cpp:452-453; abstol
 * is false on a call's first LM iteration, csparse.cpp:743-744).
 * spa_compute waits for the result.  spa_compute_device enqueues on hip_stream (NULL: the context's) and
 * returns: one kernel launch, no host synchronisation.  Only a graph edited since its last compute costs
 * more: it is uploaded first, which waits for the context's previous device work. */
int spa_compute(spa_ctx *ctx, int g_first, int count, const spa_params *params);
int spa_compute_device(spa_ctx *ctx, int g_first, int count, const spa_params *params, void *hip_stream);

/* ids_out int[n], poses_out double[n][3] in node order; either may be NULL.  Waits for the last compute. */
int spa_get_nodes(spa_ctx *ctx, int g, int *ids_out, double *poses_out);
/* The same poses on the device, double[n][3]: the d_poses layout kg_build_device and kt_set_scans_device
 * take.  Valid after the compute's stream work, until the graph is edited or the context destroyed. */
int spa_device_poses(spa_ctx *ctx, int g, const double **d_poses, int *n);
int spa_get_stats(spa_ctx *ctx, int g, spa_stats *stats);

/* Test hook: fills the working arrays of every graph (not the poses or the graph itself) with byte. */
int spa_poison_scratch(spa_ctx *ctx, int byte);

#ifdef __cplusplus
}
#endif

#endif
