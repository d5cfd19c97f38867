// karto_loop_graph.h -- host side of the loop-closure search: one graph's vertices and edge lists as MapperGraph
// keeps them (AddVertex, AddEdge Mapper.cpp:1075-1101, the Edge constructor Mapper.h:304-309) and their compilation
// into the adjacency offsets kl_search_kernel reads through.  Plain C++, no HIP: karto_loop_capi.hip includes it,
// and so does the stand-alone check tests/cpp/karto_loop_graph_check.cpp (built with -fsanitize=address,undefined).
#pragma once
#include <cstddef>
#include <vector>

namespace s2d {

struct KlGraph {
    int n = 0;                            // vertices: a scan's state id is its index
    std::vector<int> ends;                // [m][2]: source, target, in insertion order
    std::vector<std::vector<int>> edges;  // per vertex: Vertex::m_Edges as edge indices, in insertion order

    // compile()'s results
    std::vector<int> adj_off;             // [n + 1]
    std::vector<int> adj;                 // [2m][2]: the other end of the edge (GetAdjacentVertices), the edge index

    int n_scans() const { return n; }
    int n_edges() const { return (int)(ends.size() / 2); }

    void clear()
    {
        n = 0;
        ends.clear(); edges.clear(); adj_off.clear(); adj.clear();
    }

    int add_vertex()
    {
        edges.emplace_back();
        return n++;
    }

    // The loop of AddEdge (:1086-1095) over the source's edge list: the index of an edge whose target is `target`,
    // or -1.  An edge of the source's list that ends in another vertex than the source starts at the source.
    int find_edge(int source, int target) const
    {
        for (int e : edges[(size_t)source])
            if (ends[(size_t)2 * e + 1] == target) return e;
        return -1;
    }

    // new Edge(v1, v2): appended to the source's list, then to the target's
    int append_edge(int source, int target)
    {
        const int e = n_edges();
        ends.push_back(source);
        ends.push_back(target);
        edges[(size_t)source].push_back(e);
        edges[(size_t)target].push_back(e);
        return e;
    }

    // AddEdge: the existing edge's index with is_new = false, or the appended edge's with is_new = true
    int add_edge(int source, int target, bool &is_new)
    {
        const int old = find_edge(source, target);
        is_new = old < 0;
        return is_new ? append_edge(source, target) : old;
    }

    void compile()
    {
        adj_off.assign((size_t)n + 1, 0);
        adj.clear();
        adj.reserve(ends.size() * 2);
        for (int v = 0; v < n; ++v) {
            for (int e : edges[(size_t)v]) {
                const int s = ends[(size_t)2 * e], t = ends[(size_t)2 * e + 1];
                adj.push_back(s != v ? s : t);
                adj.push_back(e);
            }
            adj_off[(size_t)v + 1] = (int)(adj.size() / 2);
        }
    }
};

}  // namespace s2d
