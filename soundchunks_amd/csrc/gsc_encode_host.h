// What the encoder's host translation units share with each other and with
// nobody else: gsc_runtime.cpp (error and timing slots), gsc_reduce_host.cpp,
// gsc_knnfit_host.cpp, gsc_encode_pipeline.cpp and gsc_encode_abi.cpp.
#pragma once
#include <atomic>
#include <string>
#include <vector>

#include "../../include/soundchunks.h"
#include "gsc_device.h"
#include "gsc_hip_host.h"

namespace gsc {
#pragma GCC visibility push(hidden)

// ---- gsc_runtime.cpp: the calling thread's slots behind gsc_last_error / gsc_last_timing
const std::string& last_error();
gsc_timing& last_timing();

// ---- gsc_reduce_host.cpp
// launch rounds of the scan since the last reset (bench: launches of the dominant kernel)
extern std::atomic<int> g_scan_rounds;
// rows of `dp` floats (the device slab) -> rows of the first `d` of them
void compact_rows(std::vector<float>* v, int n, int dp, int d);
// Reduce (yakmo seeding + KNNScanReduce) for a batch of frames of one K.
// dX: device slab, frame i's Ns[i] x D features at dX + xoff[i]
// C / clusters: the frames' centroids (K*D floats) and clusters (Ns[i] ints), concatenated
// cl_host / notify (optional, device pointers of host-mapped memory): the
// batched kernel copies a frame's final clusters to cl_host + its n_off and
// then sets notify[i], so the host can post-process it during the scan tail
// D: the slab's row width (8, 16 or 32); dcol: the real colCount 2*ChunkSize
// (<= D, trailing features zero; 0 = D)
int run_reduce_batch_dev(int D, int K, int precision, const std::vector<int>& Ns, const std::vector<int64_t>& xoff,
                         const float* dX, std::vector<float>* C, std::vector<int>* clusters, std::vector<int>* iters,
                         std::vector<int>* slow, long long* restarts, double* yakmo_ms, double* scan_ms, int* cl_host,
                         int* notify, int dcol);

// ---- gsc_knnfit_host.cpp
// Device scratch of the KNNFit overflow replay: one grow-only hipMalloc
// block carved into aligned sub-buffers, owned by the caller (the encode's
// PostCtx, or the synchronous drop-in call) and freed only when the caller is
// done.  Round 4 ran the replay on stream-ordered pool memory
// (hipMallocAsync / hipFreeAsync); a second replay in one process faulted on
// the null stream, and the workaround there (plain hipMalloc) left the pool
// path in the encoder.  The arena replaces both: no pool, no free while a
// replay can still be in flight (hipFree of a retired block waits for the
// device, so retired blocks are kept until the owner is destroyed), and every
// sub-buffer is poison-filled (0xff bytes: NaN floats, -1 ints) before each
// replay, so a read of memory the replay did not write cannot hide behind the
// zero pages a fresh hipMalloc returns -- the GPU tests run the replay twice
// per process on both streams against the oracle.
struct DevArena {
    char* p = nullptr;
    size_t cap = 0, used = 0;
    std::vector<char*> retired;
    ~DevArena() {
        if (p) (void)hipFree(p);
        for (char* r : retired) (void)hipFree(r);
    }
    static size_t round_up(size_t b) { return (std::max<size_t>(b, 1) + 255) & ~size_t(255); }
    // make room for `bytes` (the sum of round_up of every take of one replay)
    hipError_t reset(size_t bytes) {
        used = 0;
        if (bytes <= cap) return hipSuccess;
        if (p) retired.push_back(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(bytes + bytes / 4, size_t(1) << 20);
        const double t = now_ms();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want);
        g_devbuf_ns.fetch_add(int64_t((now_ms() - t) * 1e6));
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <typename T>
    T* take(size_t count) {
        const size_t b = round_up(sizeof(T) * count);
        if (used + b > cap) return nullptr;
        T* r = reinterpret_cast<T*>(p + used);
        used += b;
        return r;
    }
};

// KNNFit queries whose tie set exceeds ANN's 64-NN bucket (the brute-force
// kernel marks them -1): for each affected frame, the 4R candidate rows in
// the reference order f = 4c + 2neg + rev (encoder.lpr:928-938), ANN's kd-tree
// over them (the DLL's sequential build), and ANN's priority search + the tie
// rule for every such query (gsc_ann.hip knnfit_ann_kernel).
int run_knnfit_overflow(int CS, const std::vector<FitFrame>& fr, const std::vector<int>& ov_frames,
                        const std::vector<float>& eps, const std::vector<float>& cand, const std::vector<float>& q,
                        std::vector<int>* best, hipStream_t st, DevArena* arena);

#pragma GCC visibility pop
}  // namespace gsc
