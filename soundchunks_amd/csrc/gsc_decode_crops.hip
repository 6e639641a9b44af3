// Sample ranges ("crops") of resident .gsc streams on MI355X (gfx950), beside
// gsc_decode.hip's whole-frame decode.  The streams' bytes, checkpoints,
// codebooks, attenuations and frame tables already live on the device
// (gsc_stream_open); a call uploads only its CropJob descriptors, or nothing.
//
//   crop_fused_kernel   a workgroup takes 4 Ki samples of one crop, unpacks
//                       the checkpoint segments they need into LDS (one lane
//                       per segment, symbol words idx << 2 | neg << 1 | rev as
//                       decode_unpack_kernel) and writes the samples, codebook
//                       from global memory; no scratch, one launch
//   crop_fused_bound_kernel  the same for gsc_crop_binding_decode, whose crops
//                       live on the device: lane 0 of a workgroup plans its
//                       crop from (stream, begin, count) and the binding's
//                       stream descriptor (gsc_crop_plan.h), the job goes
//                       through LDS to every wave's scalar registers, and the
//                       rest is the same code
// Consecutive lanes write consecutive elements of the output in either layout
// ([B][T][C] or [B][C][T]), so the stores coalesce, and elements past a crop's
// clipped length are written as zero.  The two-launch forms these were measured
// against are history (DESIGN.md "f5 decoder").
//
// The arithmetic is decode_synth_kernel's: the low 16 bits of
// (CAttrLookup[neg][att[idx]] * chunk[idx][j']) >> 15 with a wrapping 32-bit
// product; float output is that int16 times 2^-15, which is exact.
//
// The host planned every offset (gsc::plan_crops); the kernels still clamp
// every index and check every offset against its slab, so a stale descriptor
// cannot make them fault.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_launch.h"

namespace gsc {
namespace {

// The walk of both kernels (crop_walk_run, gsc_decode_device.h) with a sink that
// stores: a workgroup owns samples [t0, t1) of one crop's row, every channel;
// what lies past the crop's clipped length and what no frame of a stale span
// covers is zeroed.
template <typename T, bool PLANAR, typename Frame>
__device__ __forceinline__ void crop_walk_job(const CropJob& job, int64_t crop, int64_t tile, int64_t length,
                                              int channels, int tile_len, T* __restrict__ out, int64_t nout,
                                              Frame frame) {
    const int64_t t0 = tile * tile_len;
    const int64_t t1 = t0 + tile_len < length ? t0 + tile_len : length;
    if (t0 >= t1) return;
    const int64_t out_base = crop * length * channels;
    const int tid = threadIdx.x;
    auto write = [&](int64_t ua, int64_t ub, auto value) {
        crop_write_run<T, PLANAR>(ua, ub, channels, length, out_base, out, nout, tid, kFusedThreads, value);
    };
    auto blank = [&](int64_t ua, int64_t ub) { write(ua, ub, [](int64_t, int) { return (int16_t)0; }); };
    crop_walk_run(job, t0, t1, write, blank, frame);
}

// A workgroup: tile blockIdx.x % tiles of crop blockIdx.x / tiles, whose job the
// host planned; unpack and synthesis per frame are fused_frame's (gsc_decode_device.h).
template <typename T, bool PLANAR>
__global__ __launch_bounds__(kFusedThreads) void crop_fused_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                   int64_t length, int channels, int tile_len,
                                                                   int tiles, T* __restrict__ out, int64_t nout) {
    __shared__ uint16_t ssym[kFusedSegs * kDecodeS];
    __shared__ int slut[32];
    if (tiles <= 0 || channels <= 0 || tile_len <= 0) return;
    const int64_t crop = blockIdx.x / tiles;
    if (crop >= ncrops) return;
    crop_walk_job<T, PLANAR>(jobs[crop], crop, blockIdx.x - crop * tiles, length, channels, tile_len, out, nout,
                             fused_frame(ssym, slut, threadIdx.x));
}

// crop_fused_kernel for a bound call (gsc_crop_binding_decode): the workgroup
// makes its crop's job itself from crops[crop] = (stream, begin, count) and the
// binding's stream descriptors (bound_job), and the crop's first tile reports
// written[crop].  A bad crop's row is zero over the whole length.
template <typename T, bool PLANAR>
__global__ __launch_bounds__(kFusedThreads) void crop_fused_bound_kernel(
    const BoundStream* __restrict__ streams, int nstreams, const int64_t* __restrict__ crops, int ncrops,
    int64_t length, int channels, int tile_len, int tiles, T* __restrict__ out, int64_t nout,
    int64_t* __restrict__ written) {
    __shared__ uint16_t ssym[kFusedSegs * kDecodeS];
    __shared__ int slut[32];
    __shared__ SharedJob sjob;
    if (tiles <= 0 || channels <= 0 || tile_len <= 0 || nstreams <= 0) return;
    const int64_t crop = blockIdx.x / tiles;
    if (crop >= ncrops) return;
    const int64_t tile = blockIdx.x - crop * tiles;
    const CropJob job = bound_job(streams, nstreams, crops, crop, tile == 0, length, channels, written, &sjob);
    crop_walk_job<T, PLANAR>(job, crop, tile, length, channels, tile_len, out, nout,
                             fused_frame(ssym, slut, threadIdx.x));
}

template <typename T, bool PLANAR>
hipError_t launch_fused(const CropJob* jobs, int ncrops, int64_t length, int channels, int tile_len, void* out,
                        hipStream_t st) {
    if (tile_len <= 0 || tile_len > (1 << 20) || channels > 255) return hipErrorInvalidValue;
    const int64_t tiles = (length + tile_len - 1) / tile_len;
    if (tiles * ncrops > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL((crop_fused_kernel<T, PLANAR>), dim3((unsigned)(tiles * ncrops)), dim3(kFusedThreads), 0, st,
                       jobs, ncrops, length, channels, tile_len, (int)tiles, static_cast<T*>(out),
                       (int64_t)ncrops * length * channels);
    return hipGetLastError();
}

template <typename T, bool PLANAR>
hipError_t launch_fused_bound(const BoundStream* streams, int nstreams, const int64_t* crops, int ncrops,
                              int64_t length, int channels, int tile_len, void* out, int64_t* written,
                              hipStream_t st) {
    if (tile_len <= 0 || tile_len > (1 << 20) || channels > 255) return hipErrorInvalidValue;
    const int64_t tiles = (length + tile_len - 1) / tile_len;
    if (tiles * ncrops > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL((crop_fused_bound_kernel<T, PLANAR>), dim3((unsigned)(tiles * ncrops)), dim3(kFusedThreads), 0,
                       st, streams, nstreams, crops, ncrops, length, channels, tile_len, (int)tiles,
                       static_cast<T*>(out), (int64_t)ncrops * length * channels, written);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsc

using namespace gsc;

// gsc_launch_crop_fused for a bound call: crops is [ncrops][3] on the device,
// written [ncrops] there or null
extern "C" hipError_t gsc_launch_crop_fused_bound(const BoundStream* streams, int nstreams, const int64_t* crops,
                                                  int ncrops, int64_t length, int channels, int is_float, int planar,
                                                  int tile_len, void* out, int64_t* written, hipStream_t st) {
    if (ncrops <= 0 || length <= 0 || channels <= 0 || nstreams <= 0) return hipSuccess;
    return dispatch_out(is_float, planar, [&](auto t, auto p) {
        return launch_fused_bound<decltype(t), decltype(p)::value>(streams, nstreams, crops, ncrops, length, channels,
                                                                   tile_len, out, written, st);
    });
}

// unpack and synthesis in one launch, tile_len samples of a crop per workgroup
extern "C" hipError_t gsc_launch_crop_fused(const CropJob* jobs, int ncrops, int64_t length, int channels,
                                            int is_float, int planar, int tile_len, void* out, hipStream_t st) {
    if (ncrops <= 0 || length <= 0 || channels <= 0) return hipSuccess;
    return dispatch_out(is_float, planar, [&](auto t, auto p) {
        return launch_fused<decltype(t), decltype(p)::value>(jobs, ncrops, length, channels, tile_len, out, st);
    });
}
