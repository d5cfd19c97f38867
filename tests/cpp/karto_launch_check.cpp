// Stand-alone driver of the Karto host policy (csrc/karto_internal.h: kt_parse_options, kt_geometry, kt_slots,
// kt_plan_chunk, kt_plan_coarse, kg_parse_options, kg_split_rule) for tests/test_karto_launch_cpu.py.  g++ only: no
// HIP, no library.  Also meant for a sanitizer build on a CPU: `make -C tests/cpp asan` builds it with
// -fsanitize=address,undefined and runs it over the lines the CPU test sent.
//
// Without arguments it reads lines from stdin, of two forms,
//   KNOB=value ... | laser(5 numbers) params(11 numbers) max_matches max_base count pass
//   KNOB=value ... | split num_cus ntiles count
// (values hold no blanks; "KNOB=" is the empty string, a knob not named is unset; laser and params in the order of
// kt_laser / kt_params without the pads) and prints one line of JSON per input line: the parsed options, the
// geometry's integer fields, kt_get_grid_info's words, the smear kernel as hex and the plans -- or the workgroups per
// tile -- or {"error": message} on a refusal.  With the argument "constants" it prints the header's sizes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "karto_internal.h"

using namespace s2d;

static std::map<std::string, std::string> g_env;
static const char *lookup(const char *name)
{
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

static void print_list(const char *name, const int *v, int n, const char *tail)
{
    std::printf("\"%s\": [", name);
    for (int i = 0; i < n; ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]%s", tail);
}

static void split_line(std::istringstream &nums)
{
    int num_cus = 0, ntiles = 0, count = 0, force = 0;
    if (!(nums >> num_cus >> ntiles >> count) || num_cus < 1 || ntiles < 1 || count < 1) {
        std::printf("{\"error\": \"bad shape\"}\n");
        return;
    }
    if (const char *refused = kg_parse_options(force, lookup)) {
        std::printf("{\"error\": \"%s\"}\n", refused);
        return;
    }
    std::printf("{\"force_split\": %d, \"split\": %d}\n", force, kg_split_rule(force, num_cus, ntiles, count));
}

static void match_line(const std::vector<double> &v)
{
    kt_laser L{v[0], v[1], v[2], v[3], (int)v[4], 0};
    kt_params p{v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14], (int)v[15], 0};
    const int max_matches = (int)v[16], max_base = (int)v[17], count = (int)v[18], pass = (int)v[19];
    KtOptions o;
    const char *refused = kt_parse_options(o, lookup);
    KtGeom g;
    std::vector<unsigned char> kernel;
    if (refused || kt_geometry(L, p, o, g, kernel, refused) != KT_OK) {
        std::printf("{\"error\": \"%s\"}\n", refused);
        return;
    }
    if (max_matches < 1 || max_base < 0 || count < 1 || pass < 0 || pass >= g.npass) {
        std::printf("{\"error\": \"bad shape\"}\n");
        return;
    }
    std::printf("{\"tile_w\": %d, \"angle_group\": %d, \"slots_knob\": %d, \"build\": %d, \"poison\": %d, ", o.tile_w,
                o.angle_group, o.slots, (int)o.build, o.poison);
    std::printf("\"grid_size\": %d, \"border\": %d, \"width\": %d, \"height\": %d, \"ws\": %d, \"data_size\": %d, \"side\": %d, "
                "\"probs_ws\": %d, \"half\": %d, \"ksize\": %d, \"n\": %d, \"nxy\": %d, \"ctx\": %d, \"cty\": %d, \"clw\": %d, "
                "\"npass\": %d, \"fn\": %d, \"fnang\": %d, \"use_expansion\": %d, \"max_poses\": %d, \"grid_stride\": %zu, "
                "\"tiles_x\": %d, \"tiles_y\": %d, \"ntiles\": %d, ",
                g.grid_size, g.border, g.width, g.height, g.ws, g.data_size, g.side, g.probs_ws, g.half, g.ksize, g.n, g.nxy,
                g.ctx, g.cty, g.clw, g.npass, g.fn, g.fnang, g.use_expansion, g.max_poses, g.grid_stride, g.tiles_x,
                g.tiles_y, g.ntiles);
    print_list("nang", g.nang, 4, ", ");
    int info[10];
    kt_grid_info_words(g, info);
    print_list("grid_info", info, 10, ", ");
    std::printf("\"kernel\": \"");
    for (unsigned char b : kernel) std::printf("%02x", b);
    std::printf("\", ");
    const KtChunkPlan c = kt_plan_chunk(o, g, max_base, count);
    const KtCoarsePlan k = kt_plan_coarse(o, g, count, pass);
    std::printf("\"slots\": %d, \"binned_eligible\": %d, \"add\": %d, \"add_grid\": %d, \"add_block\": %d, \"clear\": %d, "
                "\"clear_grid_x\": %d, \"clear_grid_y\": %d, \"select_threads\": %d, \"fine_grid\": %d, \"fine_block\": %d, "
                "\"prepare_lds\": %zu, \"prepare_attr\": %d, \"coarse_ag\": %d, \"coarse_blocks\": %lld, \"coarse_refused\": ",
                kt_slots(o, max_matches), kt_binned_eligible(o, g, max_base), (int)c.add, c.add_grid, c.add_block,
                (int)c.clear, c.clear_grid_x, c.clear_grid_y, c.select_threads, c.fine_grid, c.fine_block, c.prepare_lds,
                c.prepare_attr, k.angle_group, k.blocks);
    if (k.refused) std::printf("\"%s\"}\n", k.refused);
    else std::printf("null}\n");
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "constants") == 0) {
        std::printf("{\"KT_THREADS\": %d, \"KT_MAX_READINGS\": %d, \"KT_FINE_MAX_ANG\": %d, \"KT_MAX_NXY\": %d, \"KT_OCC\": %d, "
                    "\"KT_AS_WAVES\": %d, \"KT_AS_MAX_TILES\": %d, \"KT_AS_MAX_BASE\": %d, \"KT_FINE_THREADS\": %d, "
                    "\"KG_MAX_SPLIT\": %d, \"sizeof_KtGeom\": %zu}\n",
                    KT_THREADS, KT_MAX_READINGS, KT_FINE_MAX_ANG, KT_MAX_NXY, KT_OCC, KT_AS_WAVES, KT_AS_MAX_TILES,
                    KT_AS_MAX_BASE, KT_FINE_THREADS, KG_MAX_SPLIT, sizeof(KtGeom));
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
        std::string word;
        std::vector<double> v;
        bool split = false, bad = false;
        while (nums >> word) {
            if (v.empty() && word == "split") {
                split = true;
                break;
            }
            char *end = nullptr;
            v.push_back(std::strtod(word.c_str(), &end));  // (the test sends repr(): strtod reads it back exactly)
            bad |= *end != '\0';
        }
        if (split) split_line(nums);
        else if (bad || v.size() != 20) std::printf("{\"error\": \"bad shape\"}\n");
        else match_line(v);
    }
    return 0;
}
