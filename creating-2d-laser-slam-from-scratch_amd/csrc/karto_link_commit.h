// karto_link_commit.h -- host side of the Karto graph-linking stage: the link records of a stage (ke_link rows and
// their ke_job_out, include/slam2d/karto_link.h) turned into the ordered graph edits of LinkScans (Mapper.cpp:1104-
// 1121): AddEdge per record, and AddConstraint only where the edge is new.  Plain C++, no HIP: karto_link_capi.hip
// includes it, and so does the stand-alone check tests/cpp/karto_link_commit_check.cpp (built with
// -fsanitize=address,undefined).
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/slam2d/karto_link.h"

namespace s2d {

// One AddEdge call of the commit, in call order; constraint: the edge was new, so AddConstraint follows with the
// record's diff and precision (record `record` of job row `job`).
struct KeAction {
    int job, record, graph, from, to;
    bool constraint;
};

// Rows jobs[count] and links[count][max_links].  A job with a status other than KE_OK and KE_SINGULAR has no
// records; a record with a status other than KE_OK (KE_SINGULAR) is skipped.  add_edge(graph, from, to, is_new) is
// the graph's AddEdge with its dedupe rule; it returns false to end the commit (the actions so far stay in out).
template <class AddEdge>
bool ke_plan_commit(const ke_job_out *jobs, const ke_link *links, int count, int max_links, AddEdge add_edge,
                    std::vector<KeAction> &out)
{
    for (int j = 0; j < count; ++j) {
        const ke_job_out &jo = jobs[j];
        if (jo.status != KE_OK && jo.status != KE_SINGULAR) continue;
        const int n = jo.n_links < max_links ? jo.n_links : max_links;
        for (int r = 0; r < n; ++r) {
            const ke_link &l = links[(size_t)j * max_links + r];
            if (l.status != KE_OK) continue;
            bool is_new = false;
            if (!add_edge(jo.graph, l.from, l.to, is_new)) return false;
            out.push_back(KeAction{j, r, jo.graph, l.from, l.to, is_new});
        }
    }
    return true;
}

}  // namespace s2d
