// karto_graph_mirror_check.cpp -- stand-alone check of csrc/karto_graph_mirror.h (built with
// -fsanitize=address,undefined by tests/test_karto_edit_cpu.py): a graph built by calls and compiled equals the graph
// rebuilt from the first one's counts and edge / constraint arrays -- what a pull-back after device edits copies --
// and compiled.
//
// stdin, one case:
//   kl  n  k  (source target) * k                 n vertices, then k AddEdge calls with the dedupe rule
//   spa n  id * n  k  (id0 id1) * k               n nodes with these ids, then k addConstraint calls by id
// stdout: one JSON object; exit status 0 when the two graphs agree in every array.
#include <cstdio>
#include <cstring>
#include <vector>

#include "karto_graph_mirror.h"

using namespace s2d;

static void print_ints(const char *name, const std::vector<int> &v, bool last = false)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}

static int run_kl()
{
    int n = 0, k = 0;
    if (scanf("%d %d", &n, &k) != 2 || n < 0 || k < 0) return 2;
    KlGraph a;
    for (int i = 0; i < n; ++i) a.add_vertex();
    std::vector<int> is_new;
    for (int i = 0; i < k; ++i) {
        int s, t;
        if (scanf("%d %d", &s, &t) != 2 || s < 0 || s >= n || t < 0 || t >= n || s == t) return 2;
        bool nw = false;
        a.add_edge(s, t, nw);
        is_new.push_back(nw);
    }
    a.compile();
    KlGraph b;
    const bool built = kl_mirror_rebuild(b, a.n_scans(), a.n_edges(), a.ends.data());
    b.compile();
    const bool same = built && b.n == a.n && b.ends == a.ends && b.edges == a.edges && b.adj_off == a.adj_off && b.adj == a.adj;
    // arrays no graph has are refused and leave the mirror empty
    KlGraph c;
    const int bad[2] = {0, n};
    const bool refused = !kl_mirror_rebuild(c, n, 1, bad) && c.n_scans() == 0 && c.n_edges() == 0;
    printf("{\"ok\": %d, \"refused\": %d, ", same ? 1 : 0, refused ? 1 : 0);
    print_ints("is_new", is_new);
    print_ints("ends", b.ends);
    print_ints("adj_off", b.adj_off);
    print_ints("adj", b.adj, true);
    printf("}\n");
    return same && refused ? 0 : 1;
}

static int run_spa()
{
    int n = 0, k = 0;
    if (scanf("%d", &n) != 1 || n < 0) return 2;
    SpaGraph a;
    for (int i = 0; i < n; ++i) {
        int id;
        if (scanf("%d", &id) != 1) return 2;
        const double pose[3] = {0.5 * i, -0.25 * i, 0.01 * i};
        a.add_node(id, pose);
    }
    if (scanf("%d", &k) != 1 || k < 0) return 2;
    std::vector<int> added;
    for (int i = 0; i < k; ++i) {
        int id0, id1;
        if (scanf("%d %d", &id0, &id1) != 2) return 2;
        const int ni0 = a.find(id0), ni1 = a.find(id1);
        const bool ok = ni0 >= 0 && ni1 >= 0 && ni0 != ni1;
        if (ok) {
            double mean[3], prec[9];
            for (int q = 0; q < 3; ++q) mean[q] = i + 0.1 * q;
            for (int q = 0; q < 9; ++q) prec[q] = 10.0 * i + q;
            a.add_constraint_by_index(ni0, ni1, mean, prec);
        }
        added.push_back(ok);
    }
    a.compile();
    SpaGraph b;
    const bool built = spa_mirror_rebuild(b, a.n_nodes(), a.ids.data(), a.poses.data(), a.n_cons(), a.ends.data(),
                                          a.means.data(), a.precs.data());
    b.compile();
    const bool same = built && b.ids == a.ids && b.poses == a.poses && b.ends == a.ends && b.means == a.means &&
                      b.precs == a.precs && b.inc_off == a.inc_off && b.inc == a.inc && b.nbr_off == a.nbr_off &&
                      b.nbr == a.nbr && b.pair_off == a.pair_off && b.pair_con == a.pair_con;
    SpaGraph c;
    const int bad[2] = {0, 0};
    const double z[9] = {0};
    const int one_id = 7;
    const bool refused = !spa_mirror_rebuild(c, 1, &one_id, z, 1, bad, z, z) && c.n_nodes() == 0 && c.n_cons() == 0;
    std::vector<int> nbr;
    for (const auto &e : b.nbr) {
        nbr.push_back(e[0]);
        nbr.push_back(e[1]);
    }
    printf("{\"ok\": %d, \"refused\": %d, ", same ? 1 : 0, refused ? 1 : 0);
    print_ints("added", added);
    print_ints("ends", b.ends);
    print_ints("inc_off", b.inc_off);
    print_ints("inc", b.inc);
    print_ints("nbr_off", b.nbr_off);
    print_ints("nbr", nbr);
    print_ints("pair_off", b.pair_off);
    print_ints("pair_con", b.pair_con, true);
    printf("}\n");
    return same && refused ? 0 : 1;
}

int main()
{
    char mode[8] = {0};
    if (scanf("%7s", mode) != 1) return 2;
    if (!strcmp(mode, "kl")) return run_kl();
    if (!strcmp(mode, "spa")) return run_spa();
    return 2;
}
