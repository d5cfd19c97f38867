// karto_graph_mirror.h -- the host mirrors of the two pose graphs (KlGraph of karto_loop_graph.h, SpaGraph of
// spa_graph.h): the epoch that tells which of them device-side edits have left behind (EditEpoch), and a mirror
// rebuilt from a graph's device arrays after such edits: the header's counts and the edge / constraint arrays in
// insertion order are all a mirror needs, since every other list is compile()'s function of them.  Plain C++, no
// HIP above the __HIPCC__ line: karto_capi.hip, karto_loop_capi.hip and spa_capi.hip include it, and so do the
// stand-alone checks tests/cpp/karto_graph_mirror_check.cpp and tests/cpp/stage_runtime_check.cpp (built with
// -fsanitize=address,undefined).  Below that line: the epoch's device words (DeviceEditEpoch), for those three.
#pragma once
#include <cstddef>
#include <vector>

#include "karto_loop_graph.h"
#include "spa_graph.h"

namespace s2d {

// Which mirrors are behind the device: every device edit call bumps the epoch, and graph g's host copy is current
// only while synced[g] equals it.  seq numbers the edit calls since the last *_get_edit_info (ge_refuse's order).
struct EditEpoch {
    unsigned epoch = 0, seq = 0;
    std::vector<unsigned> synced;  // per graph, 0 at first: a fresh context is current

    void bump()
    {
        ++epoch;
        ++seq;
    }
    bool current(int g) const { return synced[(size_t)g] == epoch; }
    void mark_current(int g) { synced[(size_t)g] = epoch; }
};

// ends int[n_edges][2]: source, target.  false (the graph is left empty) when an end is no vertex or an edge joins a
// vertex to itself -- arrays no sequence of AddVertex / AddEdge calls leaves.
inline bool kl_mirror_rebuild(KlGraph &gr, int n_scans, int n_edges, const int *ends)
{
    gr.clear();
    if (n_scans < 0 || n_edges < 0) return false;
    for (int e = 0; e < n_edges; ++e) {
        const int a = ends[2 * e], b = ends[2 * e + 1];
        if (a < 0 || a >= n_scans || b < 0 || b >= n_scans || a == b) return false;
    }
    for (int k = 0; k < n_scans; ++k) gr.add_vertex();
    for (int e = 0; e < n_edges; ++e) gr.append_edge(ends[2 * e], ends[2 * e + 1]);
    return true;
}

// ids int[n_nodes], poses double[n_nodes][3] (the device's current poses), ends int[n_cons][2] (node indices),
// means double[n_cons][3], precs double[n_cons][9].  false (the graph is left empty) when an end is no node or a
// constraint joins a node to itself.
inline bool spa_mirror_rebuild(SpaGraph &gr, int n_nodes, const int *ids, const double *poses, int n_cons, const int *ends,
                               const double *means, const double *precs)
{
    gr.clear();
    if (n_nodes < 0 || n_cons < 0) return false;
    for (int c = 0; c < n_cons; ++c) {
        const int a = ends[2 * c], b = ends[2 * c + 1];
        if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes || a == b) return false;
    }
    for (int k = 0; k < n_nodes; ++k) gr.add_node(ids[k], poses + (size_t)3 * k);
    for (int c = 0; c < n_cons; ++c)
        gr.add_constraint_by_index(ends[2 * c], ends[2 * c + 1], means + (size_t)3 * c, precs + (size_t)9 * c);
    return true;
}

}  // namespace s2d

#if defined(__HIPCC__)
#include "stage_runtime.h"

namespace s2d __attribute__((visibility("hidden"))) {

// EditEpoch with the device words the edit kernels refuse into (ge_refuse of graph_edit_device.h): the count of
// refused rows and the packed (sequence, row, status) of the first, {0, ~0} when nothing was refused.
struct DeviceEditEpoch : EditEpoch {
    unsigned long long *d_info = nullptr;

    hipError_t reset_async(hipStream_t s)
    {
        const hipError_t e = hipMemsetAsync(d_info, 0, sizeof(unsigned long long), s);
        return e != hipSuccess ? e : hipMemsetAsync(d_info + 1, 0xff, sizeof(unsigned long long), s);
    }

    // *_get_edit_info, after the caller's wait_last
    int read_and_reset(StageError &err, int *n_refused, int *first_status)
    {
        unsigned long long info[2] = {0, 0};
        hipError_t e = hipMemcpy(info, d_info, sizeof(info), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return err.fail(S2D_EHIP, "hipMemcpy(info, c->d_edit_info, sizeof(info), hipMemcpyDeviceToHost)", e);
        if (n_refused) *n_refused = (int)info[0];
        if (first_status) *first_status = info[0] ? -(int)(info[1] & 0xff) : S2D_OK;
        const unsigned long long fresh[2] = {0, ~0ull};
        if ((e = hipMemcpy(d_info, fresh, sizeof(fresh), hipMemcpyHostToDevice)) != hipSuccess)
            return err.fail(S2D_EHIP, "hipMemcpy(c->d_edit_info, fresh, sizeof(fresh), hipMemcpyHostToDevice)", e);
        seq = 0;
        return S2D_OK;
    }
};

}  // namespace s2d
#endif  // __HIPCC__
