// scan_refresh_plan_check.cpp -- TEST INFRASTRUCTURE: drives the host policy of the record-indexed scan refresh
// (csrc/scan_refresh_plan.h: the SLAM2D_REFRESH_WG knob and the launch size) on a CPU.  A stand-alone program, built
// by tests/test_karto_correct_cpu.py with g++ -fsanitize=address,undefined and run directly; no HIP, no library.
//
//   scan_refresh_plan_check constants
//   scan_refresh_plan_check grid <num_cus> <bound> [knob value]      (the knob unset when the value is absent)
//   scan_refresh_plan_check bound <n_rows> <max_scans>
// Each prints one JSON object.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "scan_refresh_plan.h"

namespace {
const char *g_knob = nullptr;  // SLAM2D_REFRESH_WG's value, or NULL: unset

const char *lookup(const char *name) { return strcmp(name, "SLAM2D_REFRESH_WG") == 0 ? g_knob : nullptr; }
}  // namespace

int main(int argc, char **argv)
{
    using namespace s2d;
    if (argc >= 2 && !strcmp(argv[1], "constants")) {
        printf("{\"REFRESH_MAX_ROWS\": %d, \"REFRESH_WAVES\": %d, \"REFRESH_WG_PER_CU\": %d}\n", REFRESH_MAX_ROWS,
               REFRESH_WAVES, REFRESH_WG_PER_CU);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "bound")) {
        printf("{\"bound\": %d}\n", refresh_bound(atoi(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "grid")) {
        g_knob = argc >= 5 ? argv[4] : nullptr;
        RefreshOptions o;
        if (const char *refused = refresh_parse_options(o, lookup)) {
            printf("{\"error\": \"%s\"}\n", refused);
            return 0;
        }
        printf("{\"max_wg\": %d, \"grid\": %d}\n", o.max_wg, refresh_grid(o, atoi(argv[2]), atoi(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: %s constants | grid <num_cus> <bound> [knob] | bound <n_rows> <max_scans>\n", argv[0]);
    return 2;
}
