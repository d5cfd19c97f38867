// karto_process_check.cpp -- stand-alone host of csrc/karto_process_commit.h: kp_create's parameter rules with the two
// thresholds, kp_set_state's rule, and the intake records of a call turned into Mapper::Process' ordered AddVertex /
// AddNode calls, with csrc/karto_loop_graph.h's AddVertex as the callback.  Built by tests/test_karto_process_cpu.py
// with -fsanitize=address,undefined; no GPU, no Python in the process.
//
// stdin, one command:
//   create  min_time min_dist min_heading buffer_dist buffer_size inverted n_graphs n_readings max_scans
//           -> {"ok": 0 or 1, "why": "...", "thr_travel": hex double, "thr_buffer": hex double, "window_max": n}
//   state   n_scans run_begin run_length max_scans buffer_size -> {"ok": 0 or 1}
//   commit  n_graphs g_first count fail_node, then per graph its scan count, then per record: status accepted scan
//           -> {"added": n, "ok": 0 or 1, "mismatch": 0 or 1, "vertices": [[g, id], ...], "nodes": [[g, scan, x], ...],
//               "counts": [per graph]}; fail_node: the AddNode call (counted from 0) that refuses, or -1
#include <cstdio>
#include <cstring>
#include <vector>

#include "karto_loop_graph.h"
#include "karto_process_commit.h"

int main()
{
    char cmd[16] = {0};
    if (scanf("%15s", cmd) != 1) return 2;
    if (!strcmp(cmd, "create")) {
        kp_params p{};
        int G = 0, nr = 0, ms = 0;
        if (scanf("%lf %lf %lf %lf %d %d %d %d %d", &p.minimum_time_interval, &p.minimum_travel_distance, &p.minimum_travel_heading,
                  &p.scan_buffer_maximum_scan_distance, &p.scan_buffer_size, &p.inverted, &G, &nr, &ms) != 9)
            return 2;
        s2d::KpPlan plan;
        const char *why = s2d::kp_check_create(p, G, nr, ms, nullptr, plan);
        printf("{\"ok\": %d, \"why\": \"%s\", \"thr_travel\": \"%a\", \"thr_buffer\": \"%a\", \"window_max\": %d}\n", why ? 0 : 1,
               why ? why : "", plan.thr_travel, plan.thr_buffer, plan.window_max);
        return 0;
    }
    if (!strcmp(cmd, "state")) {
        kp_state s{};
        int ms = 0, size = 0;
        if (scanf("%d %d %d %d %d", &s.n_scans, &s.run_begin, &s.run_length, &ms, &size) != 5) return 2;
        printf("{\"ok\": %d}\n", s2d::kp_state_valid(s, ms, size) ? 1 : 0);
        return 0;
    }
    if (strcmp(cmd, "commit")) return 2;
    int G = 0, g_first = 0, count = 0, fail_node = -1;
    if (scanf("%d %d %d %d", &G, &g_first, &count, &fail_node) != 4 || G < 1 || count < 0 || g_first < 0 || g_first + count > G) return 2;
    std::vector<s2d::KlGraph> graphs((size_t)G);
    for (auto &g : graphs) {
        int n = 0;
        if (scanf("%d", &n) != 1 || n < 0) return 2;
        for (int v = 0; v < n; ++v) g.add_vertex();
    }
    std::vector<kp_intake> recs((size_t)count);
    for (int i = 0; i < count; ++i) {
        kp_intake &r = recs[(size_t)i];
        r = kp_intake{};
        if (scanf("%d %d %d", &r.status, &r.accepted, &r.scan) != 3) return 2;
        r.corrected[0] = 100.0 * (g_first + i) + r.scan;
    }
    std::vector<int> vertices, nodes;
    std::vector<double> node_x;
    bool mismatch = false;
    int node_calls = 0;
    const int n = s2d::kp_plan_vertices(
        recs.data(), count, g_first,
        [&](int g, int &id) {
            if (g < 0 || g >= G) return false;
            id = graphs[(size_t)g].add_vertex();
            vertices.push_back(g);
            vertices.push_back(id);
            return true;
        },
        [&](int g, int scan, const double *pose) {
            if (node_calls++ == fail_node) return false;
            nodes.push_back(g);
            nodes.push_back(scan);
            node_x.push_back(pose[0]);
            return true;
        },
        &mismatch);
    printf("{\"added\": %d, \"ok\": %d, \"mismatch\": %d, \"vertices\": [", n >= 0 ? n : -(n + 1), n >= 0 ? 1 : 0, mismatch ? 1 : 0);
    for (size_t k = 0; k < vertices.size() / 2; ++k) printf("%s[%d, %d]", k ? ", " : "", vertices[2 * k], vertices[2 * k + 1]);
    printf("], \"nodes\": [");
    for (size_t k = 0; k < nodes.size() / 2; ++k) printf("%s[%d, %d, %.17g]", k ? ", " : "", nodes[2 * k], nodes[2 * k + 1], node_x[k]);
    printf("], \"counts\": [");
    for (int g = 0; g < G; ++g) printf("%s%d", g ? ", " : "", graphs[(size_t)g].n_scans());
    printf("]}\n");
    return 0;
}
