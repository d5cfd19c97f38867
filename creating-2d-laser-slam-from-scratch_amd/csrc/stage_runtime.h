// stage_runtime.h -- the host runtime every context of the library shares (hs_, gm_, pl_, ud_ and the Karto stages
// kt_, kg_, spa_, kl_, ke_, kp_, kd_, kc_): status codes, the module's error text, stream ordering between calls
// (DESIGN.md "Streams"), creation helpers and the timing entry points.  Host only, and no family's types.  The part
// above the __HIPCC__ line names no HIP symbol and compiles as plain C++17 (tests/cpp/stage_runtime_check.cpp).
#pragma once
#include <stdlib.h>

#include "knob_int.h"  // parse_knob_int

namespace s2d {

// The status codes of the public headers; each capi file asserts that its own XX_* equal them.  The four oldest
// headers (hector.h, gmapping.h, plicp.h, undistort.h) have the first five only: HS_ESTATE is hector.h's own -5.
enum : int { S2D_OK = 0, S2D_EINVAL = -1, S2D_EHIP = -2, S2D_ENOMEM = -3, S2D_ENODEV = -4, S2D_ERANGE = -5 };
#define S2D_ASSERT_COMMON_CODES(XX)                                                                          \
    static_assert(XX##_OK == s2d::S2D_OK && XX##_EINVAL == s2d::S2D_EINVAL && XX##_EHIP == s2d::S2D_EHIP &&   \
                      XX##_ENOMEM == s2d::S2D_ENOMEM && XX##_ENODEV == s2d::S2D_ENODEV,                      \
                  #XX "_* differ from the shared status codes")
#define S2D_ASSERT_STATUS_CODES(XX) \
    S2D_ASSERT_COMMON_CODES(XX);    \
    static_assert(XX##_ERANGE == s2d::S2D_ERANGE, #XX "_ERANGE differs from the shared status code")

// SLAM2D_POISON != 0 (test hook): a context fills its buffers with 0xA5 bytes first.  NULL, or the refusal's text
// (XX_EINVAL) with `poison` left alone.  Always inlined, so the library exports no symbol for it.
__attribute__((always_inline)) inline const char *poison_from_env(int &poison)
{
    if (const char *v = getenv("SLAM2D_POISON"))
        if (!parse_knob_int(v, poison)) return "SLAM2D_POISON must be an integer";
    return nullptr;
}

}  // namespace s2d

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "host_timing.h"

// Nothing below is exported from the library: the types and helpers are the capi files' own.
namespace s2d __attribute__((visibility("hidden"))) {

// One module's last error text: a thread_local instance per capi file, so kl_last_error() never shows ke_'s.
struct StageError {
    std::string text;

    const char *c_str() const { return text.c_str(); }  // *_last_error

    int fail(int code, const char *what, hipError_t e = hipSuccess)
    {
        text = what;
        if (e != hipSuccess) {
            text += ": ";
            text += hipGetErrorString(e);
        }
        return code;
    }
};

#define S2D_CHK(err, ehip, expr)                                   \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return (err).fail(ehip, #expr, _e);  \
    } while (0)

inline bool device_present()
{
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev >= 1;
}

// A context's device work is ordered across the streams its calls name: `last` ran the latest call and ev_last
// marks that call's end.
struct StreamOrder {
    hipStream_t stream = nullptr, last = nullptr;  // the context's own; the latest call's
    hipEvent_t ev_last = nullptr;
    std::mutex mu;

    // a blocking stream (not hipStreamNonBlocking): work a caller queued on the legacy default stream (e.g. torch's
    // default stream zeroing an output) is ordered before the context's own kernels
    hipError_t create()
    {
        const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamDefault);
        return e != hipSuccess ? e : hipEventCreateWithFlags(&ev_last, hipEventDisableTiming);
    }

    void destroy()
    {
        if (last) hipStreamSynchronize(last);
        if (stream) hipStreamSynchronize(stream);
        if (ev_last) hipEventDestroy(ev_last);
        if (stream) hipStreamDestroy(stream);
        stream = last = nullptr;
        ev_last = nullptr;
    }

    // the host waits for the latest call (the caller holds mu)
    int wait_last(StageError &err)
    {
        const hipError_t e = last ? hipStreamSynchronize(last) : hipSuccess;
        return e == hipSuccess ? S2D_OK : err.fail(S2D_EHIP, "hipStreamSynchronize(c->last)", e);
    }
};

// One *_device call: holds the context's mutex and picks the call's stream; begin() makes that stream follow the
// previous call, done() marks this call's end.  A call that returns between the two (an error) leaves its mark
// from the destructor, so whatever it enqueued is still waited for by the next call.
class StreamCall {
public:
    const hipStream_t s;

    StreamCall(StreamOrder &order, StageError &err, void *hip_stream)
        : s(hip_stream ? (hipStream_t)hip_stream : order.stream), o_(order), err_(err), lock_(order.mu)
    {
    }
    StreamCall(const StreamCall &) = delete;
    ~StreamCall()
    {
        if (begun_) record();
    }

    int begin()
    {
        const hipError_t e = hipStreamWaitEvent(s, o_.ev_last, 0);
        if (e != hipSuccess) return err_.fail(S2D_EHIP, "hipStreamWaitEvent(s, c->ev_last, 0)", e);
        begun_ = true;
        return S2D_OK;
    }

    int done()
    {
        begun_ = false;
        const hipError_t e = record();
        return e == hipSuccess ? S2D_OK : err_.fail(S2D_EHIP, "hipEventRecord(c->ev_last, s)", e);
    }

private:
    hipError_t record()
    {
        const hipError_t e = hipEventRecord(o_.ev_last, s);
        if (e == hipSuccess) o_.last = s;
        return e;
    }

    StreamOrder &o_;
    StageError &err_;
    std::lock_guard<std::mutex> lock_;
    bool begun_ = false;
};

// Every hipMalloc of a context: the first failure sticks (later calls do nothing), and free_all releases what was
// allocated, so *_destroy keeps no list of its own.  A call that allocates after creation reads the failure with
// take_error and frees what it got, so that a later call can allocate again.
struct DeviceBuffers {
    std::vector<std::pair<void *, size_t>> owned;
    hipError_t error = hipSuccess;

    template <class T>
    void alloc(T *&ptr, size_t bytes)
    {
        void *p = nullptr;
        if (error != hipSuccess || (error = hipMalloc(&p, bytes)) != hipSuccess) return;
        owned.push_back({p, bytes});
        ptr = (T *)p;
    }

    hipError_t take_error() { return std::exchange(error, hipSuccess); }

    template <class T>
    void free(T *&ptr)
    {
        const auto it =
            std::find_if(owned.begin(), owned.end(), [&](const auto &b) { return b.first == (const void *)ptr; });
        if (it == owned.end()) return;
        hipFree(it->first);
        owned.erase(it);
        ptr = nullptr;
    }

    // SLAM2D_POISON: every buffer's bytes
    hipError_t fill(int byte, hipStream_t s)
    {
        hipError_t e = hipSuccess;
        for (const auto &b : owned)
            if ((e = hipMemsetAsync(b.first, byte, b.second, s)) != hipSuccess) break;
        return e;
    }

    void free_all()
    {
        for (const auto &b : owned) hipFree(b.first);
        owned.clear();
    }
};

// *_set_timing, *_kernel_name and *_get_kernel_times over a module's timer and kernel-name table
inline int set_timing(KernelTimer &timer, int enable)
{
    timer.on = enable != 0;
    return S2D_OK;
}

inline const char *kernel_name(const char *const *names, int n, int i)
{
    return (i >= 0 && i < n) ? names[i] : "";
}

inline int get_kernel_times(KernelTimer &timer, StageError &err, double *ms_out, int64_t *launches_out, int reset,
                            int n)
{
    S2D_CHK(err, S2D_EHIP, hipDeviceSynchronize());
    S2D_CHK(err, S2D_EHIP, timer.collect(ms_out, launches_out, reset, n));
    return S2D_OK;
}

}  // namespace s2d
#endif  // __HIPCC__
