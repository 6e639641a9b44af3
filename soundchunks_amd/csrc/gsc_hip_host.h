// Small host-side HIP utilities of the runtime .cpp files: the calling thread's
// error slot and the device check (gsc_runtime.cpp), the host worker pool, a
// clock, and owners of a device buffer and of an event.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <functional>
#include <string>

namespace gsc {

// the calling thread's error slot (gsc_last_error): stores m, returns -1
int set_last_error(const std::string& m);
// 0 on a usable gfx950 device, else -1 with the error slot set (the hot path has no CPU fallback)
int require_device();
// host worker pool: fn(0..n-1) on up to `threads` threads
void parallel_for(int n, int threads, const std::function<void(int)>& fn);
int host_threads();

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// a HIP call of a function that reports through the error slot
#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return gsc::set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#pragma GCC visibility push(hidden)

// diagnostic (GSC_HOST_TIMING): host time inside hipMalloc / hipFree of DevBufs
extern std::atomic<int64_t> g_devbuf_ns;

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() {
        if (p) {
            const double t = now_ms();
            (void)hipFree(p);
            g_devbuf_ns.fetch_add(int64_t((now_ms() - t) * 1e6));
        }
    }
    hipError_t alloc(size_t count) {
        n = count;
        const double t = now_ms();
        const hipError_t e = hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1));
        g_devbuf_ns.fetch_add(int64_t((now_ms() - t) * 1e6));
        return e;
    }
};

// an event destroyed on every return path
struct Event {
    hipEvent_t e = nullptr;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() { return hipEventCreate(&e); }
};

#pragma GCC visibility pop

}  // namespace gsc
