// knob_int.h -- how every family's host reads an integer knob from the environment.  Plain C++17, no HIP, no
// family's types: karto_internal.h, scan_refresh_plan.h and stage_runtime.h include it.
#pragma once
#include <errno.h>
#include <limits.h>
#include <stdlib.h>

namespace s2d {

// a knob's whole value as one decimal integer ("12", "-3": no commas, no suffix, not empty) that fits an int.  One
// out-of-line copy serves every knob of every context (the library has always carried it as a weak symbol).
__attribute__((noinline)) inline bool parse_knob_int(const char *v, int &out)
{
    char *end = nullptr;
    errno = 0;
    const long long x = strtoll(v, &end, 10);
    if (end == v || *end != '\0' || errno != 0 || x < INT_MIN || x > INT_MAX) return false;
    out = (int)x;
    return true;
}

}  // namespace s2d
