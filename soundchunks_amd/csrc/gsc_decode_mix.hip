// Gain-weighted sums of crops of bound streams on MI355X (gfx950):
// gsc_crop_binding_mix's one launch (include/soundchunks.h has the definition),
// beside the crop kernels of gsc_decode_crops.hip and gsc_decode_resample.hip,
// whose device pieces it runs with another sink.
//
//   mix_kernel<T, PLANAR, RESAMPLE>  a workgroup owns one tile of one output
//                       row: kMixAccElems / channels samples (at most
//                       kResampleTile with RESAMPLE), every channel.
//     plan     lane k plans source k of the row (bound_plan): the row is bad
//              when one source or one gain is, its `written` is the largest
//              clipped count, and a source takes part in this tile when its
//              clipped count reaches into it.  A bad row is zeroed here, once.
//     sum      per source that takes part: lane 0 plans it again, the job goes
//              through LDS to every wave's scalar registers (bound_job), and
//              the tile's samples come from the frame walk of the fused crop
//              kernel (crop_walk_run, fused_frame) or from the passes of the
//              resampling one (resample_run); the sink adds gain * value to
//              the tile's 64-bit accumulators in LDS, keyed by the element's
//              place in the tile (sample-major), so it does not matter which
//              lane a run hands an element to.
//     store    rounded and clamped (gsc_mix.h), in crop_write_run's coalesced
//              element order, over the whole tile.
// No source's PCM and no intermediate row is written to memory.  The dynamic
// LDS holds the accumulators, then (RESAMPLE) the pass's source span.
//
// Barriers: one before a source is planned (the previous source's job, symbols
// and span are no longer read; the accumulators were zeroed), bound_job's own
// after the plan, those fused_frame and resample_run place around their LDS,
// and one before the store.  The runs of one source never share an element, so
// the adds need no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_launch.h"
#include "gsc_mix.h"

namespace gsc {
namespace {

constexpr int kMixThreads = 256;
static_assert(kMixThreads == kFusedThreads && kMixThreads == kResThreads, "the shared pieces stride by these");
static_assert(kMixMaxSources <= kMixThreads, "one lane plans one source");

// What the plan leaves in LDS for the rest of the kernel.
struct MixPlan {
    long long written;                  // the largest clipped count of the row's sources
    int bad;                            // a source or a gain of the row is bad
    unsigned char takes_part[kMixMaxSources];  // source k reaches into this tile
};

template <typename T, bool PLANAR, bool RESAMPLE>
__global__ __launch_bounds__(kMixThreads) void mix_kernel(const BoundStream* __restrict__ streams, int nstreams,
                                                          const int64_t* __restrict__ sources, int nrows, int nsrc,
                                                          int64_t length, int channels, int tile_len, int tiles,
                                                          int src_cap, T* __restrict__ out, int64_t nout,
                                                          int64_t* __restrict__ written) {
    extern __shared__ __align__(16) unsigned char smem[];  // tile_len * channels int64, then src_cap int16
    __shared__ uint16_t ssym[(RESAMPLE ? kResSegs : kFusedSegs) * kDecodeS];
    __shared__ int slut[32];
    __shared__ SharedJob sjob;
    __shared__ MixPlan plan;
    if (tiles <= 0 || channels <= 0 || tile_len <= 0 || nstreams <= 0 || nsrc <= 0 || nsrc > kMixMaxSources) return;
    const int64_t row = blockIdx.x / tiles;
    if (row >= nrows) return;
    const int64_t tile = blockIdx.x - row * tiles;
    const int64_t t0 = tile * tile_len;
    const int64_t t1 = t0 + tile_len < length ? t0 + tile_len : length;
    if (t0 >= t1) return;
    const int tid = threadIdx.x;
    const int acc_elems = tile_len * channels;
    int64_t* acc = reinterpret_cast<int64_t*>(smem);
    const int64_t* src = sources + row * nsrc * 4;
    const int64_t out_base = row * length * channels;
    auto store = [&](auto value) {
        crop_write_run<T, PLANAR>(t0, t1, channels, length, out_base, out, nout, tid, kMixThreads, value);
    };

    // ---- plan: every source once, before anything is added
    if (tid == 0) {
        plan.written = 0;
        plan.bad = 0;
    }
    __syncthreads();
    if (tid < nsrc) {
        CropJob unused;
        const int64_t w = bound_plan(streams, nstreams, src + 4 * tid, length, channels, &unused);
        const bool bad = w < 0 || !mix_gain_ok(src[4 * tid + 3]);
        if (bad) plan.bad = 1;
        if (!bad && tile == 0 && w > 0) atomicMax(&plan.written, (long long)w);
        plan.takes_part[tid] = !bad && w > t0;
    }
    for (int i = tid; i < acc_elems; i += kMixThreads) acc[i] = 0;
    __syncthreads();
    const bool row_bad = wave_uniform(plan.bad) != 0;
    if (tile == 0 && tid == 0 && written) written[row] = row_bad ? -1 : (int64_t)plan.written;
    if (row_bad) {
        store([](int64_t, int) { return (int16_t)0; });
        return;
    }

    // ---- sum
    for (int k = 0; k < nsrc; ++k) {
        if (wave_uniform((int)plan.takes_part[k]) == 0) continue;
        __syncthreads();  // the previous source's job, symbols and span are no longer read
        const int64_t* s = src + 4 * k;
        const CropJob job = bound_job(streams, nstreams, s, 0, false, length, channels, nullptr, &sjob);
        const int64_t gain = wave_uniform(s[3]);
        // elements of [ua, ub) x channels, sample-major from the tile's first sample
        auto add = [&](int64_t ua, int64_t ub, auto value) {
            const int n = (int)(ub - ua) * channels, base = (int)(ua - t0) * channels;
            for (int l = tid; l < n; l += kMixThreads) {
                const int dt = l / channels, c = l - dt * channels;
                const int i = base + l;
                if (i >= 0 && i < acc_elems) acc[i] += mix_term(gain, value(ua + dt, c));
            }
        };
        auto skip = [](int64_t, int64_t) {};
        if (RESAMPLE) {
            resample_run(job, t0, t1, tile_len, channels, src_cap,
                         reinterpret_cast<int16_t*>(smem + (size_t)acc_elems * sizeof(int64_t)), ssym, slut, add, skip);
        } else {
            crop_walk_run(job, t0, t1, add, skip, fused_frame(ssym, slut, tid));
        }
    }

    // ---- store
    __syncthreads();
    store([&](int64_t t, int c) {
        const int64_t i = (t - t0) * channels + c;
        return i >= 0 && i < acc_elems ? mix_round(acc[i]) : (int16_t)0;
    });
}

// the dynamic-LDS limits of the instantiations: raised when a binding is made
// (gsc_prepare_crop_mix), so that no mix call has to
template <typename T, bool PLANAR, bool RESAMPLE>
LdsLimit& mix_lds_limit() {
    static LdsLimit lim;
    return lim;
}

// accumulators, then the source span from the next 16 bytes on
inline int mix_lds_bytes(int acc_elems, int src_samples) {
    return acc_elems * (int)sizeof(int64_t) + ((src_samples * (int)sizeof(int16_t) + 15) & ~15);
}

template <typename T, bool PLANAR, bool RESAMPLE>
hipError_t launch_mix(const BoundStream* streams, int nstreams, const int64_t* sources, int nrows, int nsrc,
                      int64_t length, int channels, int src_samples, void* out, int64_t* written, hipStream_t st) {
    if (channels > 255 || nsrc > kMixMaxSources) return hipErrorInvalidValue;
    if (RESAMPLE ? (src_samples <= 0 || src_samples > kResampleSrcCap) : src_samples != 0) return hipErrorInvalidValue;
    int tile_len = mix_tile_len(channels, RESAMPLE ? kResampleTile : kMixAccElems);
    tile_len = (int)(length < tile_len ? length : tile_len);
    const int64_t tiles = (length + tile_len - 1) / tile_len;
    if (tiles * nrows > 0x7fffffff) return hipErrorInvalidValue;
    const int lds_bytes = mix_lds_bytes(tile_len * channels, src_samples);
    const hipError_t e =
        allow_lds(mix_kernel<T, PLANAR, RESAMPLE>, lds_bytes, &mix_lds_limit<T, PLANAR, RESAMPLE>());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mix_kernel<T, PLANAR, RESAMPLE>), dim3((unsigned)(tiles * nrows)), dim3(kMixThreads),
                       (size_t)lds_bytes, st, streams, nstreams, sources, nrows, nsrc, length, channels, tile_len,
                       (int)tiles, (lds_bytes - tile_len * channels * (int)sizeof(int64_t)) / 2, static_cast<T*>(out),
                       (int64_t)nrows * length * channels, written);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsc

using namespace gsc;

// Every row of a gsc_crop_binding_mix call in one launch: sources is
// [nrows][nsrc][4] on the device, written [nrows] there or null.  resample: the
// binding converts (src_samples int16 of source span per workgroup, for a tile
// of gsc_mix_tile outputs); otherwise src_samples is 0.
extern "C" hipError_t gsc_launch_crop_mix(const BoundStream* streams, int nstreams, const int64_t* sources, int nrows,
                                          int nsrc, int64_t length, int channels, int is_float, int planar,
                                          int resample, int src_samples, void* out, int64_t* written, hipStream_t st) {
    if (nrows <= 0 || length <= 0 || channels <= 0 || nstreams <= 0 || nsrc <= 0) return hipSuccess;
    return dispatch_out(is_float, planar, [&](auto t, auto p) {
        using T = decltype(t);
        constexpr bool kPlanar = decltype(p)::value;
        return resample ? launch_mix<T, kPlanar, true>(streams, nstreams, sources, nrows, nsrc, length, channels,
                                                       src_samples, out, written, st)
                        : launch_mix<T, kPlanar, false>(streams, nstreams, sources, nrows, nsrc, length, channels, 0,
                                                        out, written, st);
    });
}

// What a mix launch of a converting binding would ask of the runtime besides
// the launch, now: the dynamic-LDS limit of its four instantiations on the
// calling thread's device, for a full tile of `channels` channels.
extern "C" hipError_t gsc_prepare_crop_mix(int channels, int src_samples) {
    if (channels <= 0 || channels > 255 || src_samples <= 0 || src_samples > kResampleSrcCap)
        return hipErrorInvalidValue;
    const int lds_bytes = mix_lds_bytes(mix_tile_len(channels, kResampleTile) * channels, src_samples);
    for (int v = 0; v < 4; ++v) {
        const hipError_t e = dispatch_out(v & 1, v & 2, [&](auto t, auto p) {
            using T = decltype(t);
            constexpr bool kPlanar = decltype(p)::value;
            return allow_lds(mix_kernel<T, kPlanar, true>, lds_bytes, &mix_lds_limit<T, kPlanar, true>());
        });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
