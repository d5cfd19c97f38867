// spa_graph.h -- host side of the pose-graph optimiser: one graph's nodes and constraints as SysSPA2d keeps them
// (addNode spa2d.cpp:207-222, addConstraint :230-252) and their compilation into the index lists
// spa_solve_kernel gathers through.  Plain C++, no HIP: spa_capi.hip includes it, and so does the stand-alone
// check tests/cpp/spa_graph_check.cpp (built with -fsanitize=address,undefined).
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <vector>

namespace s2d {

struct SpaGraph {
    std::vector<int> ids;        // [n]
    std::vector<double> poses;   // [n][3]: the poses as added (the optimised ones live on the device)
    std::vector<int> ends;       // [m][2]: ndr, nd1 (node indices)
    std::vector<double> means;   // [m][3]
    std::vector<double> precs;   // [m][9]

    // compile()'s results
    std::vector<int> inc_off, inc;            // [n + 1], [2m]: constraint * 2 + end, in constraint order
    std::vector<int> nbr_off;                 // [n + 1]
    std::vector<std::array<int, 2>> nbr;      // [<= 2m]: neighbour node (ascending per node), pair
    std::vector<int> pair_off, pair_con;      // [pairs + 1], [m]: constraints per unordered pair, in constraint order

    int n_nodes() const { return (int)ids.size(); }
    int n_cons() const { return (int)(ends.size() / 2); }
    int n_pairs() const { return pair_off.empty() ? 0 : (int)pair_off.size() - 1; }

    void clear()
    {
        ids.clear(); poses.clear(); ends.clear(); means.clear(); precs.clear();
        inc_off.clear(); inc.clear(); nbr_off.clear(); nbr.clear(); pair_off.clear(); pair_con.clear();
    }

    int add_node(int id, const double *pose)
    {
        ids.push_back(id);
        poses.insert(poses.end(), pose, pose + 3);
        return n_nodes() - 1;
    }

    // The lookup loop of addConstraint (:233-241): every node is visited, so the LAST one with an id wins.
    int find(int id) const
    {
        int ni = -1;
        for (int i = 0; i < n_nodes(); ++i)
            if (ids[i] == id) ni = i;
        return ni;
    }

    void add_constraint_by_index(int ni0, int ni1, const double *mean, const double *prec)
    {
        ends.push_back(ni0);
        ends.push_back(ni1);
        means.insert(means.end(), mean, mean + 3);
        precs.insert(precs.end(), prec, prec + 9);
    }

    void compile()
    {
        const int n = n_nodes(), m = n_cons();
        // per node, its incident constraints in constraint order (counting sort keeps the order)
        inc_off.assign((size_t)n + 1, 0);
        for (int ci = 0; ci < m; ++ci) {
            ++inc_off[(size_t)ends[2 * ci] + 1];
            ++inc_off[(size_t)ends[2 * ci + 1] + 1];
        }
        for (int k = 0; k < n; ++k) inc_off[(size_t)k + 1] += inc_off[k];
        inc.assign((size_t)2 * m, 0);
        std::vector<int> fill(inc_off.begin(), inc_off.end() - 1);
        for (int ci = 0; ci < m; ++ci)
            for (int end = 0; end < 2; ++end) inc[(size_t)fill[ends[2 * ci + end]]++] = ci * 2 + end;
        // unordered pairs: constraints sorted by (lo, hi), stably, so each pair keeps the constraint order
        std::vector<std::array<int, 3>> key((size_t)m);
        for (int ci = 0; ci < m; ++ci) {
            const int a = ends[2 * ci], b = ends[2 * ci + 1];
            key[ci] = {std::min(a, b), std::max(a, b), ci};
        }
        std::stable_sort(key.begin(), key.end(), [](const std::array<int, 3> &x, const std::array<int, 3> &y) {
            return x[0] != y[0] ? x[0] < y[0] : x[1] < y[1];
        });
        pair_off.clear();
        pair_con.assign((size_t)m, 0);
        std::vector<std::array<int, 3>> half;  // node, neighbour, pair -- both directions
        for (int j = 0; j < m; ++j) {
            if (j == 0 || key[j][0] != key[j - 1][0] || key[j][1] != key[j - 1][1]) {
                const int p = (int)pair_off.size();
                pair_off.push_back(j);
                half.push_back({key[j][0], key[j][1], p});
                half.push_back({key[j][1], key[j][0], p});
            }
            pair_con[j] = key[j][2];
        }
        pair_off.push_back(m);
        // per node, its neighbours in ascending node index
        std::sort(half.begin(), half.end());
        nbr_off.assign((size_t)n + 1, 0);
        nbr.assign(half.size(), {0, 0});
        for (size_t j = 0; j < half.size(); ++j) {
            ++nbr_off[(size_t)half[j][0] + 1];
            nbr[j] = {half[j][1], half[j][2]};
        }
        for (int k = 0; k < n; ++k) nbr_off[(size_t)k + 1] += nbr_off[k];
    }

    // The direct solve's envelope (spa.h "The direct solve"), from compile()'s neighbour lists: first[k] of node
    // k >= n_fixed is the first entry >= n_fixed of its ascending neighbour list when that is < k, else k.
    int envelope_first(int k, int n_fixed) const
    {
        for (int j = nbr_off[k]; j < nbr_off[(size_t)k + 1]; ++j) {
            const int nb = nbr[j][0];
            if (nb >= n_fixed) return nb < k ? nb : k;
        }
        return k;
    }

    // The envelope's 3 x 3 blocks: the sum over the free nodes of k - first[k] + 1; 0 when nothing is fixed (such
    // a compute is refused).  n_fixed beyond the node count leaves no free node.
    long long envelope_blocks(int n_fixed) const
    {
        if (n_fixed <= 0) return 0;
        long long blocks = 0;
        for (int k = n_fixed; k < n_nodes(); ++k) blocks += (long long)(k - envelope_first(k, n_fixed)) + 1;
        return blocks;
    }
};

}  // namespace s2d
