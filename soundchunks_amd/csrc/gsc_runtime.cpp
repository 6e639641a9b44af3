// MI355X runtime, the part every other host file stands on: the host thread
// pool, the calling thread's error and timing slots, device selection and the
// device check.  The stages are in gsc_reduce_host.cpp, gsc_knnfit_host.cpp and
// gsc_encode_pipeline.cpp, the encode C ABI in gsc_encode_abi.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/soundchunks.h"
#include "gsc_encode_host.h"

namespace gsc {

void parallel_for(int n, int threads, const std::function<void(int)>& fn) {
    if (threads <= 1 || n <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    const int t = std::min(threads, n);
    pool.reserve(size_t(t));
    for (int k = 0; k < t; ++k)
        pool.emplace_back([&] {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n) break;
                fn(i);
            }
        });
    for (auto& th : pool) th.join();
}

int host_threads() {
    static int n = [] {
        const char* e = std::getenv("GSC_HOST_THREADS");
        if (e && std::atoi(e) > 0) return std::atoi(e);
        const unsigned hc = std::thread::hardware_concurrency();
        return int(std::min(16u, std::max(1u, hc)));
    }();
    return n;
}

namespace {
thread_local std::string t_err;
thread_local gsc_timing t_tim;
}  // namespace

std::atomic<int64_t> g_devbuf_ns{0};

int set_last_error(const std::string& m) {
    t_err = m;
    return -1;
}
const std::string& last_error() { return t_err; }
gsc_timing& last_timing() { return t_tim; }

// The hot path requires a gfx950 device; there is no CPU fallback.
int require_device() {
    static int state = 0;  // 0 unknown, 1 ok, -1 bad
    static std::string why;
    if (state == 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            why = "no HIP device visible (the MI355X hot path has no CPU fallback)";
            state = -1;
        } else {
            hipDeviceProp_t p;
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) {
                why = "cannot query the HIP device";
                state = -1;
            } else if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0) {
                why = std::string("device is ") + p.gcnArchName + ", kernels are built for gfx950 only";
                state = -1;
            } else {
                state = 1;
            }
        }
    }
    if (state < 0) return set_last_error(why);
    (void)hipGetLastError();  // a failure of an earlier unrelated call must not fail this one's launch checks
    return 0;
}

}  // namespace gsc

extern "C" {

void gsc_last_timing(gsc_timing* t) { *t = gsc::last_timing(); }

int gsc_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return 0;
}

int gsc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* gsc_last_error(void) { return gsc::last_error().c_str(); }

void gsc_free(void* p) { std::free(p); }

}  // extern "C"
