// karto_link_commit_check.cpp -- stand-alone host of csrc/karto_link_commit.h: the link records of a stage turned into
// LinkScans' ordered graph edits (AddEdge per record, AddConstraint only where the edge is new, Mapper.cpp:1104-1121),
// with csrc/karto_loop_graph.h's AddEdge as the dedupe callback.  Built by tests/test_karto_link_cpu.py with
// -fsanitize=address,undefined; no GPU, no Python in the process.
//
// stdin:  n_graphs n_vertices count max_links, then per job: status graph n_links, then per record of the row
//         (max_links of them, written or not): from to status
// stdout: {"ok": 1, "actions": [[job, record, graph, from, to, constraint], ...], "edges": [[[s, t], ...] per graph]}
//         ok = 0: the callback refused an edge (an end that is no vertex, or from == to) and the plan ended there
#include <cstdio>
#include <vector>

#include "karto_link_commit.h"
#include "karto_loop_graph.h"

int main()
{
    int G = 0, V = 0, count = 0, K = 0;
    if (scanf("%d %d %d %d", &G, &V, &count, &K) != 4 || G < 1 || V < 0 || count < 0 || K < 1) return 2;
    std::vector<s2d::KlGraph> graphs((size_t)G);
    for (auto &g : graphs)
        for (int v = 0; v < V; ++v) g.add_vertex();
    std::vector<ke_job_out> jobs((size_t)count);
    std::vector<ke_link> links((size_t)count * K);
    for (int j = 0; j < count; ++j) {
        ke_job_out &o = jobs[(size_t)j];
        o = ke_job_out{};
        if (scanf("%d %d %d", &o.status, &o.graph, &o.n_links) != 3) return 2;
        for (int r = 0; r < K; ++r) {
            ke_link &l = links[(size_t)j * K + r];
            l = ke_link{};
            if (scanf("%d %d %d", &l.from, &l.to, &l.status) != 3) return 2;
            l.diff[0] = j;
            l.diff[1] = r;
        }
    }
    std::vector<s2d::KeAction> actions;
    const bool ok = s2d::ke_plan_commit(jobs.data(), links.data(), count, K,
        [&](int g, int from, int to, bool &is_new) {
            if (g < 0 || g >= G || from < 0 || from >= V || to < 0 || to >= V || from == to) return false;
            graphs[(size_t)g].add_edge(from, to, is_new);
            return true;
        },
        actions);
    printf("{\"ok\": %d, \"actions\": [", ok ? 1 : 0);
    for (size_t k = 0; k < actions.size(); ++k) {
        const s2d::KeAction &a = actions[k];
        printf("%s[%d, %d, %d, %d, %d, %d]", k ? ", " : "", a.job, a.record, a.graph, a.from, a.to, a.constraint ? 1 : 0);
    }
    printf("], \"edges\": [");
    for (int g = 0; g < G; ++g) {
        printf("%s[", g ? ", " : "");
        const std::vector<int> &e = graphs[(size_t)g].ends;
        for (size_t k = 0; k < e.size() / 2; ++k) printf("%s[%d, %d]", k ? ", " : "", e[2 * k], e[2 * k + 1]);
        printf("]");
    }
    printf("]}\n");
    return 0;
}
