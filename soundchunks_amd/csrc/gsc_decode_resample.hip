// Crops of resident .gsc streams at a common sample rate and channel count on
// MI355X (gfx950): gsc_decode_crops_fmt's one launch, beside the native-rate
// kernels of gsc_decode_crops.hip.  include/soundchunks.h defines the
// resampler; gsc::plan_crops planned every crop (gsc_resample.cpp).
//
//   crop_resample_kernel  a workgroup owns kResampleTile output samples of one
//                         crop, taken in passes of as many outputs as the
//                         source samples they read fit the workgroup's LDS.
//                         A pass derives its source span (T - 1 samples before
//                         its first output's position, T after its last one's),
//                         zeroes it in LDS, and fills what lies inside the
//                         stream: per frame and per stretch of symbol rows its
//                         first lanes unpack the checkpoint segments into LDS
//                         (one lane per segment, as crop_fused_kernel), then
//                         all lanes synthesise the stretch's int16 samples of
//                         every source channel into the span.  Then one lane
//                         per output element: 2 T multiply-adds of its phase's
//                         table row (global memory) with the span (LDS) in an
//                         int64 accumulator, rounded and clamped, per source
//                         channel it needs; the channel map; the store.
//   crop_resample_bound_kernel  the same for gsc_crop_binding_decode: the
//                         workgroup plans its crop itself from device memory
//                         (bound_job, gsc_decode_device.h)
// A crop whose stream already runs at the output rate has T = 0: its span is
// its samples and an output is a source sample.  Consecutive lanes write
// consecutive elements in either layout, and elements past a crop's clipped
// length are zero, as in the other crop kernels.
//
// The kernel checks the job's numbers before it relies on them and every LDS
// and slab index where it is used; a job that fails a check writes zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_launch.h"

namespace gsc {
namespace {

// A workgroup's tile of one crop: outputs [tile * kResampleTile, + kResampleTile)
// of the crop's row (resample_run, gsc_decode_device.h) with a sink that stores.
template <typename T, bool PLANAR>
__device__ __forceinline__ void resample_tile(const CropJob& job, int64_t crop, int64_t tile, int64_t length,
                                              int channels, int src_cap, T* __restrict__ out, int64_t nout,
                                              int16_t* ssrc, uint16_t* ssym, int* slut) {
    const int tid = threadIdx.x;
    const int64_t t0 = tile * kResampleTile;
    const int64_t t1 = t0 + kResampleTile < length ? t0 + kResampleTile : length;
    if (t0 >= t1) return;
    const int64_t out_base = crop * length * channels;
    auto write = [&](int64_t ua, int64_t ub, auto value) {
        crop_write_run<T, PLANAR>(ua, ub, channels, length, out_base, out, nout, tid, kResThreads, value);
    };
    auto blank = [&](int64_t ua, int64_t ub) { write(ua, ub, [](int64_t, int) { return (int16_t)0; }); };
    resample_run(job, t0, t1, kResampleTile, channels, src_cap, ssrc, ssym, slut, write, blank);
}

template <typename T, bool PLANAR>
__global__ __launch_bounds__(kResThreads) void crop_resample_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                    int64_t length, int channels, int tiles,
                                                                    int src_cap, T* __restrict__ out, int64_t nout) {
    extern __shared__ __align__(16) unsigned char smem[];  // src_cap int16: the pass's source span
    __shared__ uint16_t ssym[kResSegs * kDecodeS];
    __shared__ int slut[32];
    if (tiles <= 0 || channels <= 0 || src_cap <= 0) return;
    const int64_t crop = blockIdx.x / tiles;
    if (crop >= ncrops) return;
    resample_tile<T, PLANAR>(jobs[crop], crop, blockIdx.x - crop * tiles, length, channels, src_cap, out, nout,
                             reinterpret_cast<int16_t*>(smem), ssym, slut);
}

// crop_resample_kernel for a bound call (gsc_crop_binding_decode): the job of
// the workgroup's crop comes from crops[crop] = (stream, begin, count) and the
// binding's stream descriptors (bound_job); the crop's first tile reports
// written[crop].  A bad crop's row is zero over the whole length.
template <typename T, bool PLANAR>
__global__ __launch_bounds__(kResThreads) void crop_resample_bound_kernel(
    const BoundStream* __restrict__ streams, int nstreams, const int64_t* __restrict__ crops, int ncrops,
    int64_t length, int channels, int tiles, int src_cap, T* __restrict__ out, int64_t nout,
    int64_t* __restrict__ written) {
    extern __shared__ __align__(16) unsigned char smem[];  // src_cap int16: the pass's source span
    __shared__ uint16_t ssym[kResSegs * kDecodeS];
    __shared__ int slut[32];
    __shared__ SharedJob sjob;
    if (tiles <= 0 || channels <= 0 || src_cap <= 0 || nstreams <= 0) return;
    const int64_t crop = blockIdx.x / tiles;
    if (crop >= ncrops) return;
    const int64_t tile = blockIdx.x - crop * tiles;
    const CropJob job = bound_job(streams, nstreams, crops, crop, tile == 0, length, channels, written, &sjob);
    resample_tile<T, PLANAR>(job, crop, tile, length, channels, src_cap, out, nout, reinterpret_cast<int16_t*>(smem),
                             ssym, slut);
}

// the dynamic-LDS limits of the bound kernel's instantiations: raised when a
// binding is made (gsc_prepare_crop_resample_bound), so that no decode call has to
template <typename T, bool PLANAR>
LdsLimit& bound_lds_limit() {
    static LdsLimit lim;
    return lim;
}

template <typename T, bool PLANAR>
hipError_t launch_resample_bound(const BoundStream* streams, int nstreams, const int64_t* crops, int ncrops,
                                 int64_t length, int channels, int src_samples, void* out, int64_t* written,
                                 hipStream_t st) {
    if (channels > 255 || src_samples <= 0 || src_samples > kResampleSrcCap) return hipErrorInvalidValue;
    const int64_t tiles = (length + kResampleTile - 1) / kResampleTile;
    if (tiles * ncrops > 0x7fffffff) return hipErrorInvalidValue;
    const int lds_bytes = (src_samples * (int)sizeof(int16_t) + 15) & ~15;
    const hipError_t e = allow_lds(crop_resample_bound_kernel<T, PLANAR>, lds_bytes, &bound_lds_limit<T, PLANAR>());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((crop_resample_bound_kernel<T, PLANAR>), dim3((unsigned)(tiles * ncrops)), dim3(kResThreads),
                       (size_t)lds_bytes, st, streams, nstreams, crops, ncrops, length, channels, (int)tiles,
                       lds_bytes / 2, static_cast<T*>(out), (int64_t)ncrops * length * channels, written);
    return hipGetLastError();
}

template <typename T, bool PLANAR>
hipError_t launch_resample(const CropJob* jobs, int ncrops, int64_t length, int channels, int src_samples, void* out,
                           hipStream_t st) {
    if (channels > 255 || src_samples <= 0 || src_samples > kResampleSrcCap) return hipErrorInvalidValue;
    const int64_t tiles = (length + kResampleTile - 1) / kResampleTile;
    if (tiles * ncrops > 0x7fffffff) return hipErrorInvalidValue;
    const int lds_bytes = (src_samples * (int)sizeof(int16_t) + 15) & ~15;
    static LdsLimit lim;  // one per instantiation
    const hipError_t e = allow_lds(crop_resample_kernel<T, PLANAR>, lds_bytes, &lim);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((crop_resample_kernel<T, PLANAR>), dim3((unsigned)(tiles * ncrops)), dim3(kResThreads),
                       (size_t)lds_bytes, st, jobs, ncrops, length, channels, (int)tiles, lds_bytes / 2,
                       static_cast<T*>(out), (int64_t)ncrops * length * channels);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsc

using namespace gsc;

// gsc_launch_crop_resample for a bound call: crops is [ncrops][3] on the
// device, written [ncrops] there or null
extern "C" hipError_t gsc_launch_crop_resample_bound(const BoundStream* streams, int nstreams, const int64_t* crops,
                                                     int ncrops, int64_t length, int channels, int is_float,
                                                     int planar, int src_samples, void* out, int64_t* written,
                                                     hipStream_t st) {
    if (ncrops <= 0 || length <= 0 || channels <= 0 || nstreams <= 0) return hipSuccess;
    return dispatch_out(is_float, planar, [&](auto t, auto p) {
        return launch_resample_bound<decltype(t), decltype(p)::value>(streams, nstreams, crops, ncrops, length,
                                                                      channels, src_samples, out, written, st);
    });
}

// What a launch of src_samples would ask of the runtime besides the launch,
// now: the dynamic-LDS limit of all four instantiations on the calling thread's device.
extern "C" hipError_t gsc_prepare_crop_resample_bound(int src_samples) {
    if (src_samples <= 0 || src_samples > kResampleSrcCap) return hipErrorInvalidValue;
    const int lds_bytes = (src_samples * (int)sizeof(int16_t) + 15) & ~15;
    for (int v = 0; v < 4; ++v) {
        const hipError_t e = dispatch_out(v & 1, v & 2, [&](auto t, auto p) {
            using T = decltype(t);
            constexpr bool kPlanar = decltype(p)::value;
            return allow_lds(crop_resample_bound_kernel<T, kPlanar>, lds_bytes, &bound_lds_limit<T, kPlanar>());
        });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Every crop of a gsc_decode_crops_fmt call in one launch; src_samples: the
// int16 source samples of the dynamic LDS, at most kResampleSrcCap.
extern "C" hipError_t gsc_launch_crop_resample(const CropJob* jobs, int ncrops, int64_t length, int channels,
                                               int is_float, int planar, int src_samples, void* out, hipStream_t st) {
    if (ncrops <= 0 || length <= 0 || channels <= 0) return hipSuccess;
    return dispatch_out(is_float, planar, [&](auto t, auto p) {
        return launch_resample<decltype(t), decltype(p)::value>(jobs, ncrops, length, channels, src_samples, out, st);
    });
}
