// Stand-alone driver of the Hector host launch policy (csrc/hector_internal.h: parse_options, plan_step,
// plan_pipeline, plan_fused_ingest) for tests/test_hector_launch_cpu.py.  g++ only: no HIP, no library.  Also meant
// for a sanitizer build on a CPU: `make -C tests/cpp asan` builds it with -fsanitize=address,undefined and runs it
// over the lines the CPU test sent.
//
// Without arguments it reads lines from stdin,
//   KNOB=value ... | B levels max_points sx sy ncu reduce_order count mode [big [ingest_n]]
// (values hold no blanks; "KNOB=" is the empty string, a knob not named is unset) and prints one line of JSON per
// input line: the parsed options and the plan, or {"error": message} when the parser refuses.  With the argument
// "constants" it prints the header's sizes that the Python test plans restate.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "hector_internal.h"

using namespace s2d;

static std::map<std::string, std::string> g_env;
static const char *lookup(const char *name)
{
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

static void print_list(const char *name, const int *v)
{
    std::printf("\"%s\": [", name);
    for (int l = 0; l < MAX_LEVELS; ++l) std::printf("%s%d", l ? ", " : "", v[l]);
    std::printf("], ");
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "constants") == 0) {
        std::printf("{\"MAX_LEVELS\": %d, \"MAX_PARTS\": %d, \"ORD_SWEEP_MAX\": %d, \"REG_POINTS\": %d, \"UPD_FIXED_WORDS\": %d, "
                    "\"UPD_THREADS\": %d, \"MAX_BIN_TILES\": %d, \"CW_MAXN\": %d, \"MATCH_REG_POINTS\": %d}\n",
                    MAX_LEVELS, MAX_PARTS, ORD_SWEEP_MAX, UPD_RREG * UPD_THREADS, UPD_FIXED_WORDS, UPD_THREADS, MAX_BIN_TILES,
                    CW_MAXN, MATCH_THREADS * MATCH_REG_PTS);
        return 0;
    }
    for (std::string line; std::getline(std::cin, line);) {
        const size_t bar = line.find('|');
        if (bar == std::string::npos) continue;
        g_env.clear();
        std::istringstream knobs(line.substr(0, bar)), nums(line.substr(bar + 1));
        for (std::string kv; knobs >> kv;) {
            const size_t eq = kv.find('=');
            if (eq != std::string::npos) g_env[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        HsShape sh{};
        int reduce_order = 0, count = 0, mode = 0, big = 0;
        if (!(nums >> sh.B >> sh.levels >> sh.max_points >> sh.sx >> sh.sy >> sh.ncu >> reduce_order >> count >> mode) ||
            sh.levels < 1 || sh.levels > MAX_LEVELS) {
            std::printf("{\"error\": \"bad shape\"}\n");
            continue;
        }
        if (nums >> big) nums >> sh.ingest_n;
        sh.big = big != 0;
        HsOptions o;
        if (const char *refused = parse_options(o, lookup)) {
            std::printf("{\"error\": \"%s\"}\n", refused);
            continue;
        }
        const StepPlan p = plan_step(o, sh, reduce_order, count, mode);
        std::printf("{\"stream_pad_words\": %zu, \"tile_wg_set\": %d, \"tile_wg_per_cu\": %d, \"pipeline\": %d, "
                    "\"reduce_order\": %d, \"fuse_ingest\": %d, \"ord_interval\": %d, \"nparts\": %d, \"nq\": %d, "
                    "\"update_single\": %d, \"upd_ring\": %d, \"upd_rays_lds\": %d, \"upd_parts_fixed\": %d, ",
                    o.stream_pad_words, o.tile_wg_set, o.tile_wg_per_cu, o.pipeline, o.reduce_order, o.fuse_ingest,
                    o.ord_interval, o.nparts, o.nq, o.update_single, o.upd_ring, o.upd_rays_lds, o.upd_parts_fixed);
        print_list("upd_parts", o.upd_parts);
        print_list("upd_minp", o.upd_minp);
        std::printf("\"seg_cap_set\": %d, \"seg_cap\": %u, \"item_cap_set\": %d, \"item_cap\": %u, ", o.seg_cap_set, o.seg_cap,
                    o.item_cap_set, o.item_cap);
        std::printf("\"seq\": %d, \"regs\": %d, \"big\": %d, \"upd\": %d, \"use_list\": %d, \"blocks\": %d, \"shmem\": %zu, "
                    "\"pipelined\": %d, \"fused_ingest\": %d}\n",
                    p.seq, p.regs, p.big, (int)p.upd, p.use_list, p.blocks, p.shmem, plan_pipeline(o, sh),
                    plan_fused_ingest(o, sh));
    }
    return 0;
}
