/* include/slam2d/spa.h -- C-ABI of the MI355X Karto pose-graph optimiser (lesson6, config 5): SPA with its
 * block-Jacobi PCG solve or a direct envelope Cholesky solve, for a fleet of independent graphs.
 *
 * Reference: MapperGraph::CorrectPoses (lesson6/lib/open_karto/src/Mapper.cpp:1397-1414) calls
 * SpaSolver::Compute (lesson6/src/spa_solver/spa_solver.cc:43-61), which calls SysSPA2d::doSPA
 * (lesson6/lib/sparse_bundle_adjustment/src/spa2d.cpp:425-609).  This library runs
 *
 *     doSPA(niter, sLambda, SBA_BLOCK_JACOBIAN_PCG, initTol, maxCGiters)
 *
 * the mode whose arithmetic is all in the reference's own text (setupSparseSys spa2d.cpp:328-413,
 * CSparse2d::incDiagBlocks / doBPCG csparse.cpp:488-492, :737-749, jacobiBPCG<3>::doBPCG2 / mMV2
 * bpcg/bpcg.h:142-161, :237-316), when spa_params.solver is SPA_SOLVER_PCG (the default).  The node itself calls
 * doSPA(40), whose default linear solver is the direct sparse Cholesky solve csp.doChol() (spa2d.cpp:501-509)
 * through CSparse's cs_cholsol / CHOLMOD, libraries outside the reference tree.  SPA_SOLVER_CHOLESKY selects a
 * direct solve as well, in an evaluation order of this library's own, stated below ("The direct solve"); an
 * ordering changes only the rounding of a Cholesky solve, not its solution.  Everything in doSPA outside the
 * linear solve is the same in both modes.  Both minimise the same cost; their iterates differ.
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
 * The direct solve (SPA_SOLVER_CHOLESKY).  tests/ref/spa2d_chol_ref.c restates it row by row; the kernel's
 * parallel schedule gives the same bits.  nF is the number of fixed nodes, node indices below are free-node
 * indices k - nF, and free node k owns the scalar rows 3k + c, c = 0, 1, 2.
 *   System.  Only the upper triangle of the block system enters, as in setupCSstructure (csparse.cpp:553-631).
 *     The working matrix A is lower triangular: for c' <= c, A(3k + c, 3k + c') = diag_k[c'][c], diag_k being the
 *     node's diagonal block after incDiagBlocks (its three diagonal elements times 1 + lambda, csparse.cpp:629);
 *     for a pair of free nodes j < k with a constraint, A(3k + c, 3j + c') = pblk_(j,k)[c'][c], pblk_(j,k) being
 *     the block addOffdiagBlock keeps at (row j, column k).
 *   Envelope, natural order (the order cs_cholsol itself uses up to csize = 100, csparse.cpp:722-726).  first[k]
 *     is the smallest free neighbour of k when that is < k, else k.  Scalar row 3k + c spans the columns
 *     start = 3 first[k] ... 3k + c; structural zeros inside the span are ordinary +0.0 entries.  A graph's
 *     envelope has sum over free k of (k - first[k] + 1) blocks of 3 x 3 (spa_envelope_blocks).
 *   Factor A = L L'.  For row i and column j <= i inside the envelope: v = A(i, j); for m ascending from
 *     max(start_i, start_j) to j - 1, v = v - L(i, m) * L(j, m), one subtraction at a time; then L(i, j) =
 *     v / L(j, j) for j < i and L(i, i) = sqrt(v) (IEEE, correctly rounded).  Any schedule that yields these
 *     bits is allowed.
 *   Solve.  Forward: y(i) = (b(i) - sum L(i, m) * y(m)) / L(i, i), m ascending from start_i, subtracted one at a
 *     time.  Backward: x(i) = (y(i) - sum L(m, i) * x(m)) / L(i, i) over the rows m > i with start_m <= i, in
 *     descending m, subtracted one at a time.  x is the step BB holds at spa2d.cpp:519.
 *   Failure.  A pivot with !(v > 0) -- zero, negative or NaN -- ends that graph's compute with the status
 *     SPA_NOT_POSDEF: the poses are as the last completed LM iteration left them, the stats those to date
 *     (lm_iters counts the iteration whose factor failed).  The reference prints "Sparse Cholesky failed!" and
 *     steps by the untouched right-hand side; this library refuses instead.
 *   cg_iters stays 0 in this mode.
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
#define SPA_NOT_POSDEF 3     /* SPA_SOLVER_CHOLESKY: a pivot was not > 0 (zero, negative or NaN).  Poses as the last
                                completed LM iteration left them, stats to date (the reference prints "Sparse
                                Cholesky failed!" and steps by the right-hand side) */
#define SPA_FACTOR_RANGE 4   /* SPA_SOLVER_CHOLESKY: the graph's envelope has more blocks than the context's
                                max_factor_blocks: refused, poses untouched */

#define SPA_SOLVER_PCG 0      /* block-Jacobi preconditioned conjugate gradients (SBA_BLOCK_JACOBIAN_PCG) */
#define SPA_SOLVER_CHOLESKY 1 /* direct envelope Cholesky in natural order ("The direct solve" above) */

#define SPA_REDUCE_LANES 256
#define SPA_FIXED_FROM_PARAMS (-2147483647 - 1)
#define SPA_MAX_NITER 1000
#define SPA_MAX_CG_ITERS 65536
#define SPA_MAX_ITER_PRODUCT 1048576 /* niter * max_cg_iters: the kernel's run time is their product */

typedef struct spa_params {
    int niter;        /* LM iterations at most: 40 (spa_solver.cc:51) */
    int max_cg_iters; /* PCG iterations per LM iteration at most: 50 (spa2d.h:249) */
    int n_fixed;      /* the first n_fixed nodes stay put: 1 (spa2d.h:198) */
    int solver;       /* SPA_SOLVER_PCG (0, the default) or SPA_SOLVER_CHOLESKY; anything else is SPA_EINVAL */
    double lambda;    /* LM diagonal augmentation, re-initialised by every compute: 1e-4; must be > 0 */
    double init_tol;  /* PCG relative tolerance: 1e-8 */
} spa_params;

typedef struct spa_stats {
    int status;      /* SPA_OK, SPA_NO_FIXED, SPA_DISCONNECTED, SPA_NOT_POSDEF, SPA_FACTOR_RANGE or SPA_NOT_RUN */
    int good_iter;   /* doSPA's return value: accepted steps */
    int lm_iters;    /* LM iterations begun (linear systems set up), the converging one included */
    int rejected;    /* steps undone because the cost did not fall */
    int cg_iters;    /* PCG iterations, all LM iterations together; 0 with SPA_SOLVER_CHOLESKY */
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
/* The same with room for the direct solve's factor: max_factor_blocks 3 x 3 blocks per graph (0 .. 2^27), the
 * sum over a graph's free nodes of k - first[k] + 1.  spa_create means 0: every SPA_SOLVER_CHOLESKY compute of a
 * graph with a free node then ends with SPA_FACTOR_RANGE.  The factor costs about the sum of the squared row
 * widths (k - first[k] + 1) in 3 x 3 products per LM iteration. */
int spa_create_ex(spa_ctx **out, int max_graphs, int max_nodes, int max_constraints, int max_factor_blocks);
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
/* The blocks of graph g's envelope when its first n_fixed nodes are fixed (n_fixed as a compute would use it: the
 * graph's own value or params->n_fixed; <= 0 gives 0 blocks): counted on the host from the neighbour lists, to size
 * a context or to predict SPA_FACTOR_RANGE. */
int spa_envelope_blocks(spa_ctx *ctx, int g, int n_fixed, long long *blocks);

/* doSPA on graphs [g_first, g_first + count).  Poses persist: a later compute starts from the optimised
 * poses, as m_Spa does.  No solver state crosses calls (lambda is re-initialised, spa2d.cpp:452-453; abstol
 * is false on a call's first LM iteration, csparse.cpp:743-744).
 * spa_compute waits for the result.  spa_compute_device enqueues on hip_stream (NULL: the context's) and
 * returns: one kernel launch, no host synchronisation.  Only a graph edited since its last compute costs
 * more: it is uploaded first, which waits for the context's previous device work. */
int spa_compute(spa_ctx *ctx, int g_first, int count, const spa_params *params);
int spa_compute_device(spa_ctx *ctx, int g_first, int count, const spa_params *params, void *hip_stream);

/* GRAPHS NAMED BY ROWS OF DEVICE MEMORY, so that the host needs to know neither which graphs are computed nor their
 * node counts.  Both calls enqueue one launch on hip_stream (NULL: the context's) and return, with no host
 * synchronisation and no copy -- unless a graph (any graph: a row may name it) has pending HOST edits, which are
 * uploaded first (the only case in which they wait).
 *
 * spa_compute_rows_device: workgroup i runs doSPA on graph d_graph[i] exactly as spa_compute_device would.  A row is
 * passed over when its entry is negative or when an earlier row names the same graph; an entry >= max_graphs is
 * refused (SPA_EINVAL, counted).  Poses and spa_stats of graphs that are not computed are untouched.
 *
 * spa_export_poses_device: the loop of MapperGraph::CorrectPoses (Mapper.cpp:1404-1411).  For row i's graph g =
 * d_graph[i] (negative: passed over; >= max_graphs: refused, SPA_EINVAL) and its nodes k = 0 .. n_nodes - 1 in node
 * order, d_pool_poses[d_pool_offset[g] + id[k]] = pose[k], the three doubles copied as bits; d_pool_offset is
 * int[max_graphs], d_pool_poses double[pool_scans][3].  A later node with the same id overwrites an earlier one.  A
 * node whose id is < 0 or whose slot lies outside [0, pool_scans) is skipped and counted (SPA_ERANGE, under its
 * row).  n_nodes is the DEVICE header's.
 *
 * spa_get_rows_info: rows (export: nodes) these two calls refused since the last call of this function, and the
 * status of the first of them in (call, row) order (SPA_OK: none).  Waits. */
int spa_compute_rows_device(spa_ctx *ctx, int n_rows, const int *d_graph, const spa_params *params, void *hip_stream);
int spa_export_poses_device(spa_ctx *ctx, int n_rows, const int *d_graph, const int *d_pool_offset,
                            double *d_pool_poses, int pool_scans, void *hip_stream);
int spa_get_rows_info(spa_ctx *ctx, int *n_refused, int *first_status);

/* ids_out int[n], poses_out double[n][3] in node order; either may be NULL.  Waits for the last compute. */
int spa_get_nodes(spa_ctx *ctx, int g, int *ids_out, double *poses_out);
/* The same poses on the device, double[n][3]: the d_poses layout kg_build_device and kt_set_scans_device
 * take.  The POINTER is fixed for the context's life (graph g owns rows [g * max_nodes, (g + 1) * max_nodes) of
 * one array), so it may be fetched once; the contents are valid after the compute's stream work.  *n is the
 * graph's node count, for which the call pulls a graph edited on the device back (it then waits). */
int spa_device_poses(spa_ctx *ctx, int g, const double **d_poses, int *n);
int spa_get_stats(spa_ctx *ctx, int g, spa_stats *stats);

/* GRAPH EDITS ON THE DEVICE.  The same edits as spa_add_node / spa_add_constraint, applied by kernels,
 * stream-ordered, with no host synchronisation and no copy -- unless a graph has pending HOST edits, which are
 * uploaded first (the only case in which these calls wait; every graph of a fresh context counts as edited once).
 * They leave the context's device arrays (header, ids, constraints and the six index lists) as host edits followed
 * by the upload would have.  Row arrays are device memory; d_mask and the output arrays may be NULL.  One workgroup
 * per row; the first row that names a graph leads it and applies all its rows in row order, so rows of several
 * graphs may be interleaved.  A negative graph skips the row; with d_mask a row is applied only where
 * d_mask[i] == 1 (else status SPA_OK, added 0).  A refused row changes nothing; later rows are still applied.
 *
 * Limits: device edits need max_nodes <= SPA_EDIT_MAX_NODES (a node's neighbour set is kept as a bit map in
 * LDS); a larger context is refused at the call with SPA_ERANGE.  The constraints have no cap of their own: no
 * list of them is kept in LDS.
 *
 * A device edit leaves the host's copy of the graphs behind.  spa_add_node, spa_add_constraint, spa_get_counts,
 * spa_get_nodes, spa_envelope_blocks, spa_set_n_fixed and spa_device_poses then first pull their graph back (they
 * wait and copy its header, ids, poses and constraints); spa_set_graph and spa_clear_graph overwrite it.
 *
 * spa_edit_nodes_device: appends node (id, pose) and writes the pose into the device poses; the other nodes'
 * optimised poses persist.  A full graph refuses the row with SPA_ERANGE.
 * spa_edit_constraints_device: spa_add_constraint's semantics: an unknown id gives added 0 and SPA_OK; id0 == id1,
 * or both ids resolving to one node, SPA_EINVAL; max_constraints reached, SPA_ERANGE. */
#define SPA_EDIT_MAX_NODES 4096

typedef struct spa_node_row {
    int graph, id;
    double pose[3];
} spa_node_row;

typedef struct spa_con_row {
    int graph, id0, id1, pad_;
    double mean[3];
    double prec[9];
} spa_con_row;

int spa_edit_nodes_device(spa_ctx *ctx, int count, const spa_node_row *d_rows, const int *d_mask, int *d_status_out,
                          void *hip_stream);
int spa_edit_constraints_device(spa_ctx *ctx, int count, const spa_con_row *d_rows, const int *d_mask,
                                int *d_added_out, int *d_status_out, void *hip_stream);
/* Rows the device edits refused since the last call of this function, and the status of the first of them in
 * (call, row) order (SPA_OK: none).  Waits. */
int spa_get_edit_info(spa_ctx *ctx, int *n_refused, int *first_status);
/* Inspection: uploads graph g's pending host edits, waits, and copies its DEVICE arrays back: ids int[n_nodes],
 * ends int[n_cons][2], means double[n_cons][3], precs double[n_cons][9], inc_off int[n_nodes + 1], inc int[2
 * n_cons], nbr_off int[n_nodes + 1], nbr int[nbr_off[n_nodes]][2], pair_off int[n_pairs + 1], pair_con
 * int[n_cons].  Any output may be NULL. */
int spa_download_graph(spa_ctx *ctx, int g, int *n_nodes, int *n_cons, int *n_pairs, int *ids_out, int *ends_out,
                       double *means_out, double *precs_out, int *inc_off_out, int *inc_out, int *nbr_off_out,
                       int *nbr_out, int *pair_off_out, int *pair_con_out);

/* Test hook: fills the working arrays of every graph (not the poses or the graph itself) with byte. */
int spa_poison_scratch(spa_ctx *ctx, int byte);

#ifdef __cplusplus
}
#endif

#endif
