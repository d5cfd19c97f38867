// karto_edit_kernels.hip -- HIP kernels of the Karto graph-edit stage (gfx950; the C-ABI is
// include/slam2d/karto_edit.h).  The edits themselves run in the graph contexts' kernels (karto_loop_kernels.hip
// kl_edit_*, spa_kernels.hip spa_edit_*); these turn the stages' device records into their rows.
//   kd_flatten_vertices_kernel  one lane per kp_intake record: the vertex row's graph and expected id, the node row.
//   kd_flatten_edges_kernel     one lane per (job, link record): the edge row and the constraint row; a record that
//                               is not committed gets graph -1, which both edit kernels skip.
//   kd_tally_kernel             after an edit call: the node mask from the vertex ids, and the stage's totals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slam2d/karto_edit.h"

namespace s2d {

constexpr int KD_THREADS = 256;

__global__ void __launch_bounds__(KD_THREADS)
kd_flatten_vertices_kernel(const kp_intake *__restrict__ intake, int g_first, int count, int *__restrict__ graph,
                           int *__restrict__ expect, spa_node_row *__restrict__ nodes)
{
    const int i = blockIdx.x * KD_THREADS + threadIdx.x;
    if (i >= count) return;
    const kp_intake r = intake[i];
    const bool use = r.accepted && r.status == KP_OK;  // kp_plan_vertices
    graph[i] = use ? g_first + i : -1;
    expect[i] = r.scan;
    spa_node_row n;
    n.graph = use ? g_first + i : -1;
    n.id = r.scan;
    for (int q = 0; q < 3; ++q) n.pose[q] = r.corrected[q];
    nodes[i] = n;
}

__global__ void __launch_bounds__(KD_THREADS)
kd_flatten_edges_kernel(const ke_job_out *__restrict__ jobs, const ke_link *__restrict__ links, int max_links,
                        int first_job, int count, kl_edge_row *__restrict__ edges, spa_con_row *__restrict__ cons)
{
    const int i = blockIdx.x * KD_THREADS + threadIdx.x;
    if (i >= count * max_links) return;
    const int j = first_job + i / max_links, r = i % max_links;
    const ke_job_out jo = jobs[j];
    const ke_link l = links[(size_t)j * max_links + r];
    // ke_plan_commit
    const bool use = (jo.status == KE_OK || jo.status == KE_SINGULAR) && r < jo.n_links && l.status == KE_OK;
    const int g = use ? jo.graph : -1;
    edges[i] = kl_edge_row{g, l.from, l.to, 0};
    spa_con_row c;
    c.graph = g;
    c.id0 = l.from;
    c.id1 = l.to;
    c.pad_ = 0;
    for (int q = 0; q < 3; ++q) c.mean[q] = l.diff[q];
    for (int q = 0; q < 9; ++q) c.prec[q] = l.precision[q];
    cons[i] = c;
}

// val NULL: only the refusals of `status` are counted.  which 0: val is a vertex id (>= 0: added) and mask_out gets
// 1 where the vertex was added; which 1: val is an is_new flag.  info: vertices, new edges, refused rows.
__global__ void __launch_bounds__(KD_THREADS)
kd_tally_kernel(int count, const int *__restrict__ val, int which, const int *__restrict__ status, int *__restrict__ mask_out,
                int *__restrict__ info)
{
    const int i = blockIdx.x * KD_THREADS + threadIdx.x;
    int ok = 0, bad = 0;
    if (i < count) {
        if (val) ok = which == 0 ? val[i] >= 0 : val[i] == 1;
        if (mask_out) mask_out[i] = ok;
        bad = status[i] != 0;
    }
    // counts only: integer sums are the same in any order
    const int oks = __popcll(__ballot(ok)), bads = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (oks) atomicAdd(&info[which], oks);
        if (bads) atomicAdd(&info[2], bads);
    }
}

}  // namespace s2d
