// karto_process_commit.h -- host side of the Karto scan-intake stage (include/slam2d/karto_process.h): the create-time
// parameter rules with the two thresholds, kp_set_state's rule, and the intake records of a call turned into the
// ordered AddVertex / AddNode calls of Mapper::Process (Mapper.cpp:2053).  Plain C++, no HIP: karto_process_capi.hip
// includes it, and so does the stand-alone check tests/cpp/karto_process_check.cpp (built with
// -fsanitize=address,undefined).
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/slam2d/karto_process.h"

namespace s2d {

struct KpPlan {
    double thr_travel = 0;  // Square(minimum_travel_distance) - KT_TOLERANCE   (Mapper.cpp:2114)
    double thr_buffer = 0;  // Square(scan_buffer_maximum_scan_distance) - KT_TOLERANCE   (Mapper.h:1376)
    int window_max = 0;     // the longest running window a graph can hold: min(scan_buffer_size, max_scans)
};

// nullptr when the context can be created, else what is wrong
inline const char *kp_check_create(const kp_params &p, int n_graphs, int n_readings, int max_scans, const int *pool_offset,
                                   KpPlan &plan)
{
    if (n_graphs < 1 || n_graphs > (1 << 20)) return "need 1 <= n_graphs <= 2^20";
    if (n_readings < 1 || n_readings > 4096) return "need 1 <= n_readings <= 4096";
    if (max_scans < 1 || max_scans > KL_MAX_SCANS) return "need 1 <= max_scans <= KL_MAX_SCANS (4096)";
    if (p.scan_buffer_size < 1) return "need scan_buffer_size >= 1";
    if (p.minimum_time_interval != p.minimum_time_interval || p.minimum_travel_distance != p.minimum_travel_distance ||
        p.minimum_travel_heading != p.minimum_travel_heading)
        return "a parameter is NaN";
    if (p.inverted != 0 && p.inverted != 1) return "inverted must be 0 or 1";
    plan.thr_travel = p.minimum_travel_distance * p.minimum_travel_distance - KL_TOLERANCE;
    plan.thr_buffer = p.scan_buffer_maximum_scan_distance * p.scan_buffer_maximum_scan_distance - KL_TOLERANCE;
    // d2(back, back) = 0 > thr would erase the new scan itself: the reference then calls front() on an empty vector
    if (!(plan.thr_buffer >= 0.0)) return "need Square(scan_buffer_maximum_scan_distance) - KT_TOLERANCE >= 0";
    plan.window_max = p.scan_buffer_size < max_scans ? p.scan_buffer_size : max_scans;
    if (pool_offset)
        for (int g = 0; g < n_graphs; ++g)
            if (pool_offset[g] < 0 || pool_offset[g] > INT32_MAX - max_scans) return "a pool offset is out of range";
    if (!pool_offset && (long long)n_graphs * max_scans > INT32_MAX) return "the default pool offsets exceed an int";
    return nullptr;
}

// kp_set_state's rule: the running scans are a non-empty contiguous tail of a non-empty graph's scans
inline bool kp_state_valid(const kp_state &s, int max_scans, int scan_buffer_size)
{
    if (s.n_scans < 0 || s.n_scans > max_scans) return false;
    if (s.n_scans == 0) return s.run_length == 0 && s.run_begin == 0;
    if (s.run_length < 1 || s.run_length > scan_buffer_size || s.run_length > s.n_scans) return false;
    return s.run_begin == s.n_scans - s.run_length;
}

// Per accepted record in order: add_vertex(graph, id) (AddVertex; id = the scan count before), then, the id being
// the record's scan index, add_node(graph, scan, corrected) (AddNode).  Returns the number of vertices added, or
// -(1 + that number) at the first failure: a callback returning false, or an id other than the scan index.
template <class AddVertex, class AddNode>
int kp_plan_vertices(const kp_intake *recs, int count, int g_first, AddVertex add_vertex, AddNode add_node, bool *id_mismatch)
{
    int added = 0;
    if (id_mismatch) *id_mismatch = false;
    for (int i = 0; i < count; ++i) {
        const kp_intake &r = recs[i];
        if (!r.accepted || r.status != KP_OK) continue;
        int id = -1;
        if (!add_vertex(g_first + i, id)) return -(1 + added);
        ++added;
        if (id != r.scan) {
            if (id_mismatch) *id_mismatch = true;
            return -(1 + added);
        }
        if (!add_node(g_first + i, r.scan, r.corrected)) return -(1 + added);
    }
    return added;
}

}  // namespace s2d
