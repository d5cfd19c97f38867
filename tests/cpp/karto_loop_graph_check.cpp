// karto_loop_graph_check.cpp -- stand-alone host of csrc/karto_loop_graph.h: MapperGraph::AddEdge's dedupe rule
// (Mapper.cpp:1075-1101) and the adjacency order of compile() against a brute-force recount over the accepted edges.
// Built by tests/test_karto_loop_cpu.py with -fsanitize=address,undefined; no GPU, no Python in the process.
//
// stdin:  n m  s_0 t_0 ... s_{m-1} t_{m-1}      (m AddEdge calls on n vertices)
// stdout: {"ok": 1, "is_new": [...], "ends": [[s, t], ...], "adj_off": [...], "adj": [[other, edge], ...]}
#include <cstdio>
#include <vector>

#include "karto_loop_graph.h"

int main()
{
    int n = 0, m = 0;
    if (scanf("%d %d", &n, &m) != 2 || n < 0 || m < 0) return 2;
    s2d::KlGraph g;
    for (int v = 0; v < n; ++v)
        if (g.add_vertex() != v) return 3;
    std::vector<int> is_new, want_new;
    std::vector<int> acc;  // accepted edges: source, target
    for (int k = 0; k < m; ++k) {
        int s, t;
        if (scanf("%d %d", &s, &t) != 2 || s < 0 || s >= n || t < 0 || t >= n || s == t) return 2;
        // brute force: old only if an accepted edge runs from s to t (t -> s does not count)
        bool old = false;
        for (size_t e = 0; e < acc.size() / 2; ++e) old = old || (acc[2 * e] == s && acc[2 * e + 1] == t);
        want_new.push_back(old ? 0 : 1);
        if (!old) {
            acc.push_back(s);
            acc.push_back(t);
        }
        bool fresh = false;
        const int e = g.add_edge(s, t, fresh);
        is_new.push_back(fresh ? 1 : 0);
        if (g.ends[(size_t)2 * e] != s || g.ends[(size_t)2 * e + 1] != t) return 4;
    }
    g.compile();
    // brute force: vertex v's list is every accepted edge that touches v, in insertion order, as (other end, edge)
    std::vector<int> want_off(1, 0), want_adj;
    for (int v = 0; v < n; ++v) {
        for (size_t e = 0; e < acc.size() / 2; ++e) {
            if (acc[2 * e] == v) {
                want_adj.push_back(acc[2 * e + 1]);
                want_adj.push_back((int)e);
            } else if (acc[2 * e + 1] == v) {
                want_adj.push_back(acc[2 * e]);
                want_adj.push_back((int)e);
            }
        }
        want_off.push_back((int)(want_adj.size() / 2));
    }
    const bool ok = is_new == want_new && g.ends == acc && g.adj_off == want_off && g.adj == want_adj &&
                    g.n_edges() == (int)(acc.size() / 2) && g.n_scans() == n;
    printf("{\"ok\": %d, \"is_new\": [", ok ? 1 : 0);
    for (size_t k = 0; k < is_new.size(); ++k) printf("%s%d", k ? ", " : "", is_new[k]);
    printf("], \"ends\": [");
    for (size_t e = 0; e < g.ends.size() / 2; ++e) printf("%s[%d, %d]", e ? ", " : "", g.ends[2 * e], g.ends[2 * e + 1]);
    printf("], \"adj_off\": [");
    for (size_t k = 0; k < g.adj_off.size(); ++k) printf("%s%d", k ? ", " : "", g.adj_off[k]);
    printf("], \"adj\": [");
    for (size_t k = 0; k < g.adj.size() / 2; ++k) printf("%s[%d, %d]", k ? ", " : "", g.adj[2 * k], g.adj[2 * k + 1]);
    printf("]}\n");
    g.clear();
    return ok ? 0 : 1;
}
