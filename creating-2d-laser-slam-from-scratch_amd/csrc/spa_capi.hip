// spa_capi.hip -- host runtime + extern "C" boundary (include/slam2d/spa.h) of the pose-graph optimiser.
// The optimisation runs in spa_kernels.hip; the host keeps each graph's nodes and constraints (spa_graph.h) and
// uploads an edited graph before its next compute.  Without a usable HIP device spa_create fails with SPA_ENODEV
// (no CPU fallback).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "stage_runtime.h"
#include "karto_graph_mirror.h"
#include "spa_graph.h"
#include "spa_kernels.hip"

using namespace s2d;

namespace {
thread_local StageError spa_err;
S2D_ASSERT_STATUS_CODES(SPA);

constexpr int SPA_MAX_GRAPHS = 1 << 16;
constexpr int SPA_MAX_NODES = 1 << 20;
constexpr int SPA_MAX_CONS = 1 << 22;
constexpr int SPA_MAX_FACTOR_BLOCKS = 1 << 27;
}  // namespace

struct spa_ctx {
    int G = 0, N = 0, M = 0;
    std::vector<SpaGraph> graphs;
    std::vector<int> uploaded_nodes;  // per graph: nodes [0, uploaded) have their pose on the device
    std::vector<char> dirty;          // per graph: edited since the last upload
    std::vector<int> n_fixed;         // per graph: SysSPA2d::nFixed, or SPA_FIXED_FROM_PARAMS
    DeviceEditEpoch edit;  // device edits: which host copies are behind
    DeviceEditEpoch rows;  // the row-indexed compute and export: their refusals' words and call numbers only
    int *d_ids = nullptr;
    SpaDev dev{};
    SpaHdr *d_hdr = nullptr;
    int2 *d_con_nd = nullptr, *d_nbr = nullptr;
    double *d_con_mean = nullptr, *d_con_prec = nullptr;
    int *d_inc_off = nullptr, *d_inc = nullptr, *d_nbr_off = nullptr, *d_pair_off = nullptr, *d_pair_con = nullptr;
    size_t scratch_bytes = 0, fac_bytes = 0, fidx_bytes = 0;
    StreamOrder order;
    DeviceBuffers mem;
};

namespace {

int check_graph(const spa_ctx *c, int g)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    if (g < 0 || g >= c->G) return spa_err.fail(SPA_EINVAL, "graph index out of range");
    return SPA_OK;
}

// An edited graph: its index lists, constraints and the poses of the nodes added since the last upload.  The
// copies are synchronous and follow the context's previous device work.
int upload_graph(spa_ctx *c, int g)
{
    SpaGraph &gr = c->graphs[g];
    int rc = c->order.wait_last(spa_err);
    if (rc != SPA_OK) return rc;
    gr.compile();
    const size_t N = (size_t)c->N, M = (size_t)c->M;
    const int n = gr.n_nodes(), m = gr.n_cons();
    const SpaHdr h{n, m, gr.n_pairs(), c->n_fixed[g]};
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_hdr + g, &h, sizeof(h), hipMemcpyHostToDevice));
    const int up = c->uploaded_nodes[g];
    if (n > up)
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->dev.poses + (g * N + up) * 3, gr.poses.data() + (size_t)up * 3, sizeof(double) * 3 * (n - up),
                       hipMemcpyHostToDevice));
    c->uploaded_nodes[g] = n;
    if (n > 0) S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_ids + g * N, gr.ids.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    if (m > 0) {
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_con_nd + g * M, gr.ends.data(), sizeof(int) * 2 * m, hipMemcpyHostToDevice));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_con_mean + g * M * 3, gr.means.data(), sizeof(double) * 3 * m, hipMemcpyHostToDevice));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_con_prec + g * M * 9, gr.precs.data(), sizeof(double) * 9 * m, hipMemcpyHostToDevice));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_inc + g * 2 * M, gr.inc.data(), sizeof(int) * gr.inc.size(), hipMemcpyHostToDevice));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_pair_con + g * M, gr.pair_con.data(), sizeof(int) * m, hipMemcpyHostToDevice));
        if (!gr.nbr.empty())
            S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_nbr + g * 2 * M, gr.nbr.data(), sizeof(int) * 2 * gr.nbr.size(), hipMemcpyHostToDevice));
    }
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_inc_off + g * (N + 1), gr.inc_off.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice));
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_nbr_off + g * (N + 1), gr.nbr_off.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice));
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(c->d_pair_off + g * (M + 1), gr.pair_off.data(), sizeof(int) * gr.pair_off.size(),
                   hipMemcpyHostToDevice));
    c->dirty[g] = 0;
    return SPA_OK;
}

// The host copy of graph g, current again after device edits: waits, and copies the header, the nodes and the
// constraints back.  The poses of the copy are the device's current ones, and all of them count as uploaded.
int pull_graph(spa_ctx *c, int g)
{
    if (c->edit.current(g)) return SPA_OK;
    int rc = c->order.wait_last(spa_err);
    if (rc != SPA_OK) return rc;
    const size_t N = (size_t)c->N, M = (size_t)c->M;
    SpaHdr h{};
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(&h, c->d_hdr + g, sizeof(h), hipMemcpyDeviceToHost));
    if (h.n_nodes < 0 || h.n_nodes > c->N || h.n_cons < 0 || h.n_cons > c->M)
        return spa_err.fail(SPA_EHIP, "the device header of the graph is out of range");
    const size_t n = (size_t)h.n_nodes, m = (size_t)h.n_cons;
    std::vector<int> ids(n), ends(2 * m);
    std::vector<double> poses(3 * n), means(3 * m), precs(9 * m);
    if (n > 0) {
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(ids.data(), c->d_ids + g * N, sizeof(int) * n, hipMemcpyDeviceToHost));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(poses.data(), c->dev.poses + g * N * 3, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
    }
    if (m > 0) {
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(ends.data(), c->d_con_nd + g * M, sizeof(int) * 2 * m, hipMemcpyDeviceToHost));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(means.data(), c->d_con_mean + g * M * 3, sizeof(double) * 3 * m, hipMemcpyDeviceToHost));
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(precs.data(), c->d_con_prec + g * M * 9, sizeof(double) * 9 * m, hipMemcpyDeviceToHost));
    }
    if (!spa_mirror_rebuild(c->graphs[g], h.n_nodes, ids.data(), poses.data(), h.n_cons, ends.data(), means.data(),
                            precs.data()))
        return spa_err.fail(SPA_EHIP, "the device constraint list of the graph is not a graph's");
    c->graphs[g].compile();  // spa_envelope_blocks reads the lists of a graph that is not dirty
    c->uploaded_nodes[g] = h.n_nodes;
    c->edit.mark_current(g);
    return SPA_OK;
}

SpaEdit edit_args(spa_ctx *c)
{
    return SpaEdit{c->d_hdr,   c->dev.poses, c->d_ids,      c->d_con_nd,   c->d_con_mean,    c->d_con_prec,
                   c->d_inc_off, c->d_inc,   c->d_nbr_off,  c->d_nbr,      c->d_pair_off,    c->d_pair_con,
                   c->dev.scratch, c->edit.d_info, c->N,    c->M,          c->G,             c->edit.seq};
}

// before a device edit: the context's sizes, then pending host edits go up (the only wait); afterwards every host
// copy is behind
int begin_edit(spa_ctx *c, StreamCall &call)
{
    if (c->N > SPA_EDIT_MAX_NODES) return spa_err.fail(SPA_ERANGE, "device edits need max_nodes <= SPA_EDIT_MAX_NODES (4096)");
    int rc;
    for (int g = 0; g < c->G; ++g)
        if (c->dirty[g] && (rc = upload_graph(c, g)) != SPA_OK) return rc;
    c->edit.bump();
    return call.begin();
}

// after a launch: its error, then the call's end
int end_launch(StreamCall &call)
{
    S2D_CHK(spa_err, SPA_EHIP, hipGetLastError());
    return call.done();
}

int check_params(const spa_params *p)
{
    if (!p) return spa_err.fail(SPA_EINVAL, "params is NULL");
    if (p->niter < 0 || p->niter > SPA_MAX_NITER) return spa_err.fail(SPA_EINVAL, "niter must be in [0, SPA_MAX_NITER]");
    if (p->max_cg_iters < 0 || p->max_cg_iters > SPA_MAX_CG_ITERS)
        return spa_err.fail(SPA_EINVAL, "max_cg_iters must be in [0, SPA_MAX_CG_ITERS]");
    if ((long long)p->niter * p->max_cg_iters > SPA_MAX_ITER_PRODUCT)
        return spa_err.fail(SPA_EINVAL, "niter * max_cg_iters exceeds SPA_MAX_ITER_PRODUCT");
    if (!(p->lambda > 0) || !std::isfinite(p->lambda)) return spa_err.fail(SPA_EINVAL, "lambda must be > 0 and finite");
    if (!(p->init_tol >= 0)) return spa_err.fail(SPA_EINVAL, "init_tol must be >= 0");
    if (p->solver != SPA_SOLVER_PCG && p->solver != SPA_SOLVER_CHOLESKY)
        return spa_err.fail(SPA_EINVAL, "solver must be SPA_SOLVER_PCG or SPA_SOLVER_CHOLESKY");
    return SPA_OK;
}

// doSPA, one workgroup per graph: graphs [g_first, g_first + count), or those the `count` rows of graph_of name
void launch_solve(spa_ctx *c, int count, int g_first, const int *graph_of, const SpaRows &rows, const spa_params *p,
                  StreamCall &call)
{
    if (p->solver == SPA_SOLVER_CHOLESKY)
        hipLaunchKernelGGL(spa_solve_kernel<SPA_SOLVER_CHOLESKY>, dim3((unsigned)count), dim3(SPA_THREADS), 0, call.s,
                           c->dev, g_first, graph_of, rows, *p);
    else
        hipLaunchKernelGGL(spa_solve_kernel<SPA_SOLVER_PCG>, dim3((unsigned)count), dim3(SPA_THREADS), 0, call.s, c->dev,
                           g_first, graph_of, rows, *p);
}

int run(spa_ctx *c, int g_first, int count, const spa_params *p, StreamCall &call)
{
    int rc = check_params(p);
    if (rc != SPA_OK) return rc;
    if (g_first < 0 || count < 0 || g_first > c->G - count) return spa_err.fail(SPA_EINVAL, "graph range out of bounds");
    if (count == 0) return SPA_OK;
    for (int g = g_first; g < g_first + count; ++g)
        if (c->dirty[g] && (rc = upload_graph(c, g)) != SPA_OK) return rc;
    // order after the context's previous device work, whichever stream it ran on (DESIGN.md "Streams")
    if ((rc = call.begin()) != SPA_OK) return rc;
    launch_solve(c, count, g_first, nullptr, SpaRows{}, p, call);
    return end_launch(call);
}

// before a call whose graphs are rows of device memory: any graph may be named, so every pending host edit goes up
// (the only wait); the call gets the next number of the refusals' order
int begin_rows(spa_ctx *c, StreamCall &call)
{
    int rc;
    for (int g = 0; g < c->G; ++g)
        if (c->dirty[g] && (rc = upload_graph(c, g)) != SPA_OK) return rc;
    c->rows.bump();
    return call.begin();
}

SpaRows rows_args(spa_ctx *c) { return SpaRows{c->rows.d_info, c->G, c->rows.seq}; }

}  // namespace

extern "C" {

const char *spa_last_error(void) { return spa_err.c_str(); }
const char *spa_version(void) { return "slam2d-spa 2 (gfx950, block-Jacobi PCG, envelope Cholesky)"; }

void spa_default_params(spa_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->niter = 40;          // spa_solver.cc:51
    p->max_cg_iters = 50;   // spa2d.h:249
    p->n_fixed = 1;         // spa2d.h:198
    p->lambda = 1.0e-4;     // spa2d.h:249
    p->init_tol = 1.0e-8;   // spa2d.h:249
}

int spa_create(spa_ctx **out, int max_graphs, int max_nodes, int max_constraints)
{
    return spa_create_ex(out, max_graphs, max_nodes, max_constraints, 0);
}

int spa_create_ex(spa_ctx **out, int max_graphs, int max_nodes, int max_constraints, int max_factor_blocks)
{
    if (!out) return spa_err.fail(SPA_EINVAL, "out is NULL");
    *out = nullptr;
    if (max_factor_blocks < 0 || max_factor_blocks > SPA_MAX_FACTOR_BLOCKS)
        return spa_err.fail(SPA_EINVAL, "need 0 <= max_factor_blocks <= 2^27");
    if (max_graphs < 1 || max_graphs > SPA_MAX_GRAPHS || max_nodes < 1 || max_nodes > SPA_MAX_NODES ||
        max_constraints < 1 || max_constraints > SPA_MAX_CONS)
        return spa_err.fail(SPA_EINVAL, "need 1 <= max_graphs <= 2^16, 1 <= max_nodes <= 2^20, 1 <= max_constraints <= 2^22");
    if (!device_present()) return spa_err.fail(SPA_ENODEV, "no HIP device");
    spa_ctx *c = new spa_ctx;
    c->G = max_graphs;
    c->N = max_nodes;
    c->M = max_constraints;
    c->graphs.resize((size_t)max_graphs);
    c->uploaded_nodes.assign((size_t)max_graphs, 0);
    c->dirty.assign((size_t)max_graphs, 1);
    c->edit.synced.assign((size_t)max_graphs, 0);
    c->n_fixed.assign((size_t)max_graphs, SPA_FIXED_FROM_PARAMS);
    const size_t G = (size_t)max_graphs, N = (size_t)max_nodes, M = (size_t)max_constraints;
    c->scratch_bytes = sizeof(double) * G * spa_scratch_doubles(max_nodes, max_constraints);
    c->fac_bytes = sizeof(double) * G * (size_t)max_factor_blocks * 9;
    c->fidx_bytes = sizeof(int) * G * spa_fidx_ints(max_nodes);
    hipError_t e;
    if ((e = c->order.create()) != hipSuccess) {
        spa_destroy(c);
        return spa_err.fail(SPA_EHIP, "hipStreamCreate", e);
    }
    DeviceBuffers &m = c->mem;
    m.alloc(c->d_hdr, sizeof(SpaHdr) * G);
    m.alloc(c->dev.poses, sizeof(double) * G * N * 3);
    m.alloc(c->d_ids, sizeof(int) * G * N);
    m.alloc(c->edit.d_info, sizeof(unsigned long long) * 2);
    m.alloc(c->rows.d_info, sizeof(unsigned long long) * 2);
    m.alloc(c->d_con_nd, sizeof(int2) * G * M);
    m.alloc(c->d_con_mean, sizeof(double) * G * M * 3);
    m.alloc(c->d_con_prec, sizeof(double) * G * M * 9);
    m.alloc(c->d_inc_off, sizeof(int) * G * (N + 1));
    m.alloc(c->d_inc, sizeof(int) * G * 2 * M);
    m.alloc(c->d_nbr_off, sizeof(int) * G * (N + 1));
    m.alloc(c->d_nbr, sizeof(int2) * G * 2 * M);
    m.alloc(c->d_pair_off, sizeof(int) * G * (M + 1));
    m.alloc(c->d_pair_con, sizeof(int) * G * M);
    m.alloc(c->dev.scratch, c->scratch_bytes);
    if (c->fac_bytes > 0) m.alloc(c->dev.fac, c->fac_bytes);
    m.alloc(c->dev.fidx, c->fidx_bytes);
    m.alloc(c->dev.stats, sizeof(spa_stats) * G);
    if ((e = m.error) != hipSuccess) {
        spa_destroy(c);
        return spa_err.fail(SPA_ENOMEM, "hipMalloc", e);
    }
    c->dev.max_nodes = max_nodes;
    c->dev.max_cons = max_constraints;
    c->dev.max_fac = max_factor_blocks;
    c->dev.hdr = c->d_hdr;
    c->dev.con_nd = c->d_con_nd;
    c->dev.con_mean = c->d_con_mean;
    c->dev.con_prec = c->d_con_prec;
    c->dev.inc_off = c->d_inc_off;
    c->dev.inc = c->d_inc;
    c->dev.nbr_off = c->d_nbr_off;
    c->dev.nbr = c->d_nbr;
    c->dev.pair_off = c->d_pair_off;
    c->dev.pair_con = c->d_pair_con;
    std::vector<spa_stats> st(G);
    for (auto &x : st) {
        memset(&x, 0, sizeof(x));
        x.status = SPA_NOT_RUN;
    }
    if ((e = hipMemcpy(c->dev.stats, st.data(), sizeof(spa_stats) * G, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(c->dev.poses, 0, sizeof(double) * G * N * 3)) != hipSuccess ||
        (e = c->edit.reset_async(c->order.stream)) != hipSuccess ||
        (e = c->rows.reset_async(c->order.stream)) != hipSuccess ||
        (e = hipEventRecord(c->order.ev_last, c->order.stream)) != hipSuccess) {
        spa_destroy(c);
        return spa_err.fail(SPA_EHIP, "initialising the context", e);
    }
    *out = c;
    return SPA_OK;
}

int spa_destroy(spa_ctx *c)
{
    if (!c) return SPA_OK;
    c->order.destroy();
    c->mem.free_all();
    delete c;
    return SPA_OK;
}

int spa_add_node(spa_ctx *c, int g, int id, const double *pose)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    if (!pose) return spa_err.fail(SPA_EINVAL, "pose is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;
    if (c->graphs[g].n_nodes() >= c->N) return spa_err.fail(SPA_ERANGE, "the graph already has max_nodes nodes");
    c->graphs[g].add_node(id, pose);
    c->dirty[g] = 1;
    return SPA_OK;
}

int spa_add_constraint(spa_ctx *c, int g, int id0, int id1, const double *mean, const double *prec, int *added)
{
    if (added) *added = 0;
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    if (!mean || !prec) return spa_err.fail(SPA_EINVAL, "NULL argument");
    if (id0 == id1) return spa_err.fail(SPA_EINVAL, "a constraint from a node to itself");
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;
    SpaGraph &gr = c->graphs[g];
    const int ni0 = gr.find(id0), ni1 = gr.find(id1);
    if (ni0 < 0 || ni1 < 0) return SPA_OK;  // addConstraint returns false (:241)
    if (ni0 == ni1) return spa_err.fail(SPA_EINVAL, "a constraint from a node to itself");
    if (gr.n_cons() >= c->M) return spa_err.fail(SPA_ERANGE, "the graph already has max_constraints constraints");
    gr.add_constraint_by_index(ni0, ni1, mean, prec);
    c->dirty[g] = 1;
    if (added) *added = 1;
    return SPA_OK;
}

int spa_set_graph(spa_ctx *c, int g, int n_nodes, const int *ids, const double *poses, int n_cons, const int *ends,
                  const double *means, const double *precs)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    if (n_nodes < 0 || n_cons < 0) return spa_err.fail(SPA_EINVAL, "negative count");
    if (n_nodes > c->N || n_cons > c->M) return spa_err.fail(SPA_ERANGE, "more nodes or constraints than the context holds");
    if ((n_nodes > 0 && (!ids || !poses)) || (n_cons > 0 && (!ends || !means || !precs)))
        return spa_err.fail(SPA_EINVAL, "NULL argument");
    for (int ci = 0; ci < n_cons; ++ci) {
        const int a = ends[2 * ci], b = ends[2 * ci + 1];
        if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) return spa_err.fail(SPA_EINVAL, "constraint end out of range");
        if (a == b) return spa_err.fail(SPA_EINVAL, "a constraint from a node to itself");
    }
    std::lock_guard<std::mutex> lock(c->order.mu);
    SpaGraph &gr = c->graphs[g];
    gr.clear();
    for (int k = 0; k < n_nodes; ++k) gr.add_node(ids[k], poses + 3 * k);
    for (int ci = 0; ci < n_cons; ++ci) gr.add_constraint_by_index(ends[2 * ci], ends[2 * ci + 1], means + 3 * ci, precs + 9 * ci);
    c->uploaded_nodes[g] = 0;
    c->edit.mark_current(g);
    c->dirty[g] = 1;
    return SPA_OK;
}

int spa_clear_graph(spa_ctx *c, int g)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    c->graphs[g].clear();
    c->uploaded_nodes[g] = 0;
    c->edit.mark_current(g);
    c->dirty[g] = 1;
    return SPA_OK;
}

int spa_set_n_fixed(spa_ctx *c, int g, int n_fixed)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;  // the upload that follows rewrites the whole graph
    c->n_fixed[g] = n_fixed;
    c->dirty[g] = 1;
    return SPA_OK;
}

int spa_get_counts(spa_ctx *c, int g, int *n_nodes, int *n_cons)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;
    if (n_nodes) *n_nodes = c->graphs[g].n_nodes();
    if (n_cons) *n_cons = c->graphs[g].n_cons();
    return SPA_OK;
}

int spa_envelope_blocks(spa_ctx *c, int g, int n_fixed, long long *blocks)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    if (!blocks) return spa_err.fail(SPA_EINVAL, "blocks is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;
    SpaGraph &gr = c->graphs[g];
    if (c->dirty[g]) gr.compile();  // the lists only; the upload stays with the next compute
    *blocks = gr.envelope_blocks(n_fixed);
    return SPA_OK;
}

int spa_compute_device(spa_ctx *c, int g_first, int count, const spa_params *params, void *hip_stream)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    StreamCall call(c->order, spa_err, hip_stream);
    return run(c, g_first, count, params, call);
}

int spa_compute(spa_ctx *c, int g_first, int count, const spa_params *params)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    StreamCall call(c->order, spa_err, nullptr);
    int rc = run(c, g_first, count, params, call);
    if (rc != SPA_OK) return rc;
    S2D_CHK(spa_err, SPA_EHIP, hipStreamSynchronize(c->order.stream));
    return SPA_OK;
}

int spa_compute_rows_device(spa_ctx *c, int n_rows, const int *d_graph, const spa_params *params, void *hip_stream)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    int rc = check_params(params);
    if (rc != SPA_OK) return rc;
    if (n_rows < 0) return spa_err.fail(SPA_EINVAL, "negative count");
    if (n_rows == 0) return SPA_OK;
    if (!d_graph) return spa_err.fail(SPA_EINVAL, "d_graph is NULL");
    StreamCall call(c->order, spa_err, hip_stream);
    if ((rc = begin_rows(c, call)) != SPA_OK) return rc;
    launch_solve(c, n_rows, 0, d_graph, rows_args(c), params, call);
    return end_launch(call);
}

int spa_export_poses_device(spa_ctx *c, int n_rows, const int *d_graph, const int *d_pool_offset, double *d_pool_poses,
                            int pool_scans, void *hip_stream)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    if (n_rows < 0 || pool_scans < 0) return spa_err.fail(SPA_EINVAL, "negative count");
    if (n_rows == 0) return SPA_OK;
    if (!d_graph || !d_pool_offset || !d_pool_poses) return spa_err.fail(SPA_EINVAL, "NULL argument");
    StreamCall call(c->order, spa_err, hip_stream);
    int rc = begin_rows(c, call);
    if (rc != SPA_OK) return rc;
    hipLaunchKernelGGL(spa_export_kernel, dim3((unsigned)n_rows), dim3(GE_THREADS), 0, call.s, c->dev, rows_args(c), c->d_ids,
                       d_graph, d_pool_offset, (unsigned long long *)d_pool_poses, pool_scans);
    return end_launch(call);
}

int spa_get_rows_info(spa_ctx *c, int *n_refused, int *first_status)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    const int rc = c->order.wait_last(spa_err);
    return rc != SPA_OK ? rc : c->rows.read_and_reset(spa_err, n_refused, first_status);
}

int spa_get_nodes(spa_ctx *c, int g, int *ids_out, double *poses_out)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = c->order.wait_last(spa_err)) != SPA_OK) return rc;
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;
    const SpaGraph &gr = c->graphs[g];
    const int n = gr.n_nodes(), up = c->uploaded_nodes[g];
    if (ids_out)
        for (int k = 0; k < n; ++k) ids_out[k] = gr.ids[k];
    if (poses_out) {
        if (up > 0)
            S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(poses_out, c->dev.poses + (size_t)g * c->N * 3, sizeof(double) * 3 * up, hipMemcpyDeviceToHost));
        for (int k = up; k < n; ++k)
            for (int q = 0; q < 3; ++q) poses_out[3 * k + q] = gr.poses[(size_t)3 * k + q];
    }
    return SPA_OK;
}

int spa_device_poses(spa_ctx *c, int g, const double **d_poses, int *n)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = pull_graph(c, g)) != SPA_OK) return rc;
    if (c->dirty[g] && (rc = upload_graph(c, g)) != SPA_OK) return rc;  // nodes added since the last compute
    if (d_poses) *d_poses = c->dev.poses + (size_t)g * c->N * 3;
    if (n) *n = c->graphs[g].n_nodes();
    return SPA_OK;
}

int spa_get_stats(spa_ctx *c, int g, spa_stats *stats)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    if (!stats) return spa_err.fail(SPA_EINVAL, "stats is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    if ((rc = c->order.wait_last(spa_err)) != SPA_OK) return rc;
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(stats, c->dev.stats + g, sizeof(*stats), hipMemcpyDeviceToHost));
    return SPA_OK;
}

int spa_edit_nodes_device(spa_ctx *c, int count, const spa_node_row *d_rows, const int *d_mask, int *d_status_out,
                          void *hip_stream)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    if (count < 0) return spa_err.fail(SPA_EINVAL, "negative count");
    StreamCall call(c->order, spa_err, hip_stream);
    if (c->N > SPA_EDIT_MAX_NODES) return spa_err.fail(SPA_ERANGE, "device edits need max_nodes <= SPA_EDIT_MAX_NODES (4096)");
    if (count == 0) return SPA_OK;
    if (!d_rows) return spa_err.fail(SPA_EINVAL, "d_rows is NULL");
    int rc = begin_edit(c, call);
    if (rc != SPA_OK) return rc;
    hipLaunchKernelGGL(spa_edit_nodes_kernel, dim3((unsigned)count), dim3(GE_THREADS), 0, call.s, edit_args(c), count,
                       d_rows, d_mask, d_status_out);
    return end_launch(call);
}

int spa_edit_constraints_device(spa_ctx *c, int count, const spa_con_row *d_rows, const int *d_mask, int *d_added_out,
                                int *d_status_out, void *hip_stream)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    if (count < 0) return spa_err.fail(SPA_EINVAL, "negative count");
    StreamCall call(c->order, spa_err, hip_stream);
    if (c->N > SPA_EDIT_MAX_NODES) return spa_err.fail(SPA_ERANGE, "device edits need max_nodes <= SPA_EDIT_MAX_NODES (4096)");
    if (count == 0) return SPA_OK;
    if (!d_rows) return spa_err.fail(SPA_EINVAL, "d_rows is NULL");
    int rc = begin_edit(c, call);
    if (rc != SPA_OK) return rc;
    hipLaunchKernelGGL(spa_edit_constraints_kernel, dim3((unsigned)count), dim3(GE_THREADS), spa_edit_lds(c->N), call.s,
                       edit_args(c), count, d_rows, d_mask, d_added_out, d_status_out);
    return end_launch(call);
}

int spa_get_edit_info(spa_ctx *c, int *n_refused, int *first_status)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    const int rc = c->order.wait_last(spa_err);
    return rc != SPA_OK ? rc : c->edit.read_and_reset(spa_err, n_refused, first_status);
}

int spa_download_graph(spa_ctx *c, int g, int *n_nodes, int *n_cons, int *n_pairs, int *ids_out, int *ends_out,
                       double *means_out, double *precs_out, int *inc_off_out, int *inc_out, int *nbr_off_out,
                       int *nbr_out, int *pair_off_out, int *pair_con_out)
{
    int rc = check_graph(c, g);
    if (rc != SPA_OK) return rc;
    std::lock_guard<std::mutex> lock(c->order.mu);
    if (c->dirty[g] && (rc = upload_graph(c, g)) != SPA_OK) return rc;
    if ((rc = c->order.wait_last(spa_err)) != SPA_OK) return rc;
    const size_t N = (size_t)c->N, M = (size_t)c->M;
    SpaHdr h{};
    S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(&h, c->d_hdr + g, sizeof(h), hipMemcpyDeviceToHost));
    if (h.n_nodes < 0 || h.n_nodes > c->N || h.n_cons < 0 || h.n_cons > c->M || h.n_pairs < 0 || h.n_pairs > h.n_cons)
        return spa_err.fail(SPA_EHIP, "the device header of the graph is out of range");
    if (n_nodes) *n_nodes = h.n_nodes;
    if (n_cons) *n_cons = h.n_cons;
    if (n_pairs) *n_pairs = h.n_pairs;
    const size_t n = (size_t)h.n_nodes, m = (size_t)h.n_cons;
#define SPA_DOWN(out, src, bytes) \
    if ((out) && (bytes) > 0) S2D_CHK(spa_err, SPA_EHIP, hipMemcpy((out), (src), (bytes), hipMemcpyDeviceToHost))
    SPA_DOWN(ids_out, c->d_ids + g * N, sizeof(int) * n);
    SPA_DOWN(ends_out, c->d_con_nd + g * M, sizeof(int2) * m);
    SPA_DOWN(means_out, c->d_con_mean + g * M * 3, sizeof(double) * 3 * m);
    SPA_DOWN(precs_out, c->d_con_prec + g * M * 9, sizeof(double) * 9 * m);
    SPA_DOWN(inc_off_out, c->d_inc_off + g * (N + 1), sizeof(int) * (n + 1));
    SPA_DOWN(inc_out, c->d_inc + g * 2 * M, sizeof(int) * 2 * m);
    SPA_DOWN(nbr_off_out, c->d_nbr_off + g * (N + 1), sizeof(int) * (n + 1));
    SPA_DOWN(pair_off_out, c->d_pair_off + g * (M + 1), sizeof(int) * ((size_t)h.n_pairs + 1));
    SPA_DOWN(pair_con_out, c->d_pair_con + g * M, sizeof(int) * m);
    if (nbr_out && m > 0) {
        int total = 0;
        S2D_CHK(spa_err, SPA_EHIP, hipMemcpy(&total, c->d_nbr_off + g * (N + 1) + n, sizeof(int), hipMemcpyDeviceToHost));
        if (total < 0 || (size_t)total > 2 * m) return spa_err.fail(SPA_EHIP, "the device neighbour offsets of the graph are out of range");
        SPA_DOWN(nbr_out, c->d_nbr + g * 2 * M, sizeof(int2) * (size_t)total);
    }
#undef SPA_DOWN
    return SPA_OK;
}

int spa_poison_scratch(spa_ctx *c, int byte)
{
    if (!c) return spa_err.fail(SPA_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->order.mu);
    int rc = c->order.wait_last(spa_err);
    if (rc != SPA_OK) return rc;
    S2D_CHK(spa_err, SPA_EHIP, hipMemset(c->dev.scratch, byte, c->scratch_bytes));
    if (c->fac_bytes > 0) S2D_CHK(spa_err, SPA_EHIP, hipMemset(c->dev.fac, byte, c->fac_bytes));
    S2D_CHK(spa_err, SPA_EHIP, hipMemset(c->dev.fidx, byte, c->fidx_bytes));
    S2D_CHK(spa_err, SPA_EHIP, hipDeviceSynchronize());
    return SPA_OK;
}

}  // extern "C"
