// scan_refresh_plan.h -- the host policy of the record-indexed scan refresh (kl_refresh_device of karto_loop.h): its
// knob and the size of its one launch.  The kernel takes its scans from a list it builds on the device (a prefix sum
// over the rows' resolved counts) by a grid-stride loop, so the grid only has to be large enough to fill the GPU and
// never depends on a number the host would have to read back.  No HIP type, no context, no global: it compiles as
// plain C++17 too (tests/cpp/scan_refresh_plan_check.cpp, tests/test_karto_correct_cpu.py).
#pragma once
#include <limits.h>

#include "knob_int.h"  // parse_knob_int

namespace s2d {

constexpr int REFRESH_MAX_ROWS = 4096;  // the prefix sum lives in one workgroup's LDS (KL_REFRESH_MAX_ROWS)
constexpr int REFRESH_WAVES = 4;        // scans a workgroup of 256 lanes has in flight, one per wave
constexpr int REFRESH_WG_PER_CU = 8;

struct RefreshOptions {
    int max_wg = 0;  // SLAM2D_REFRESH_WG: > 0 caps the launch at that many workgroups (tests, A/B); <= 0 or unset: no cap
};

// The knob, through get (the library: getenv).  NULL, or the refusal's text (the create call then fails with EINVAL):
// a value that is not one whole decimal integer.
inline const char *refresh_parse_options(RefreshOptions &o, const char *(*get)(const char *))
{
    o = RefreshOptions{};
    if (const char *v = get("SLAM2D_REFRESH_WG"))
        if (!parse_knob_int(v, o.max_wg)) return "SLAM2D_REFRESH_WG must be an integer";
    return nullptr;
}

// What the host knows of a call's scans without reading a row: every row names at most max_scans of them.
inline int refresh_bound(int n_rows, int max_scans)
{
    const long long b = (long long)(n_rows < 0 ? 0 : n_rows) * (max_scans < 0 ? 0 : max_scans);
    return b > INT_MAX ? INT_MAX : (int)b;
}

// Workgroups of the launch for at most `bound` scans: one wave per scan until every CU holds REFRESH_WG_PER_CU
// workgroups, the grid-stride loop beyond that.  0 for no scans (nothing is launched).
inline int refresh_grid(const RefreshOptions &o, int num_cus, int bound)
{
    if (bound <= 0) return 0;
    const int by_scans = (bound - 1) / REFRESH_WAVES + 1;
    const int fill = (num_cus < 1 ? 1 : num_cus) * REFRESH_WG_PER_CU;
    int grid = by_scans < fill ? by_scans : fill;
    if (o.max_wg > 0 && o.max_wg < grid) grid = o.max_wg;
    return grid;
}

}  // namespace s2d
