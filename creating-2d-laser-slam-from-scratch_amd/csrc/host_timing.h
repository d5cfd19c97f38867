// host_timing.h -- per-kernel device timing of a context's launches (host only): a pool of hipEvent pairs around each
// launch and the accumulated milliseconds / launch counts per kernel.  Used by every context that times its kernels
// (hs_, gm_, pl_ and the Karto stages) through stage_runtime.h, which holds the *_set_timing / *_get_kernel_times
// entry points' common part.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace s2d {

struct KernelTimer {
    static constexpr int MAX_KERNELS = 8;
    using Pair = std::pair<hipEvent_t, hipEvent_t>;
    bool on = false;                             // *_set_timing
    std::vector<Pair> idle;                      // events are created lazily, only while timing is on
    std::vector<std::pair<int, Pair>> used;      // (kernel, events) of the launches not yet collected
    Pair cur{};                                  // the launch between begin and end
    double acc_ms[MAX_KERNELS] = {};
    int64_t acc_n[MAX_KERNELS] = {};

    hipError_t begin(hipStream_t s)
    {
        if (!on) return hipSuccess;
        hipError_t e;
        if (!idle.empty()) {
            cur = idle.back();
            idle.pop_back();
        } else if ((e = hipEventCreate(&cur.first)) != hipSuccess || (e = hipEventCreate(&cur.second)) != hipSuccess) {
            return e;
        }
        return hipEventRecord(cur.first, s);
    }

    // after the launch: its error, timing or not
    hipError_t end(hipStream_t s, int which)
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || !on) return e;
        if ((e = hipEventRecord(cur.second, s)) != hipSuccess) return e;
        used.push_back({which, cur});
        return hipSuccess;
    }

    // the caller has synchronised the device: add the finished launches up and report kernels [0, n)
    hipError_t collect(double *ms_out, int64_t *launches_out, int reset, int n)
    {
        for (auto &u : used) {
            float ms = 0;
            const hipError_t e = hipEventElapsedTime(&ms, u.second.first, u.second.second);
            if (e != hipSuccess) return e;
            acc_ms[u.first] += ms;
            acc_n[u.first] += 1;
            idle.push_back(u.second);
        }
        used.clear();
        for (int i = 0; i < n; ++i) {
            if (ms_out) ms_out[i] = acc_ms[i];
            if (launches_out) launches_out[i] = acc_n[i];
            if (reset) {
                acc_ms[i] = 0;
                acc_n[i] = 0;
            }
        }
        return hipSuccess;
    }

    void destroy()
    {
        for (auto &u : used) idle.push_back(u.second);
        for (auto &p : idle) {
            hipEventDestroy(p.first);
            hipEventDestroy(p.second);
        }
        used.clear();
        idle.clear();
    }
};

// One kernel launch of a context's function: `fail(code, what, hipError_t)` is the file's error return, `ehip` its
// code for a HIP error.  hipGetLastError is checked after every launch.
#define S2D_TIMED_LAUNCH(timer, fail, ehip, stream, which, ...)                      \
    do {                                                                             \
        hipError_t _e = (timer).begin(stream);                                       \
        if (_e != hipSuccess) return fail(ehip, "hipEventRecord (kernel timing)", _e); \
        hipLaunchKernelGGL(__VA_ARGS__);                                             \
        if ((_e = (timer).end(stream, which)) != hipSuccess) return fail(ehip, "hipGetLastError()", _e); \
    } while (0)

}  // namespace s2d
