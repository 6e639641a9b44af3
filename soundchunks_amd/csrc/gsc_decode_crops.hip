// Sample ranges ("crops") of resident .gsc streams on MI355X (gfx950), beside
// gsc_decode.hip's whole-frame decode.  The streams' bytes, checkpoints,
// codebooks, attenuations and frame tables already live on the device
// (gsc_stream_open); a call uploads only its CropJob / CropPiece descriptors.
//
//   crop_fused_kernel   the default: a workgroup takes 4 Ki samples of one
//                       crop, unpacks the checkpoint segments they need into
//                       LDS (one lane per segment, symbol words idx << 2 |
//                       neg << 1 | rev as decode_unpack_kernel) and writes the
//                       samples, codebook from global memory; no scratch
// and, behind gsc_decode_crops_variant, the two-launch forms it was measured
// against (DESIGN.md "f5 decoder"):
//   crop_unpack_kernel  one lane per checkpoint segment a crop touches, in
//                       every frame it crosses, to that segment's slot of the
//                       call's symbol scratch
//   crop_synth_kernel   one lane per output element (crop, t, channel); the
//                       lane finds its frame within the crop's frame span and
//                       reads the codebook from global memory
//   crop_synth_lds_kernel  a workgroup takes 16 Ki samples of one crop and
//                       stages the codebook of every frame they cross in LDS,
//                       as decode_synth_kernel does
//   crop_fused_bound_kernel  crop_fused_kernel for gsc_crop_binding_decode,
//                       whose crops live on the device: lane 0 of a workgroup
//                       plans its crop from (stream, begin, count) and the
//                       binding's stream descriptor (gsc_crop_plan.h), the
//                       job goes through LDS to every wave's scalar registers,
//                       and the rest is the same code
// In all of them consecutive lanes write consecutive elements of the output
// in either layout ([B][T][C] or [B][C][T]), so the stores coalesce, and
// elements past a crop's clipped length are written as zero.
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

constexpr int kCropUnpackThreads = 256;
constexpr int kCropSynthThreads = 256;

__global__ __launch_bounds__(kCropUnpackThreads) void crop_unpack_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                         const CropPiece* __restrict__ pieces,
                                                                         int npieces, uint16_t* __restrict__ sym,
                                                                         int64_t nslots) {
    const int64_t slot = (int64_t)blockIdx.x * kCropUnpackThreads + threadIdx.x;
    if (slot >= nslots || npieces <= 0) return;
    // the last piece whose first slot is <= slot (an empty frame's piece owns none)
    const CropPiece pc = pieces[last_le(0, npieces - 1, slot, [&](int i) { return pieces[i].slot0; })];
    const int64_t k = slot - pc.slot0;
    if (k < 0 || k >= pc.nseg || pc.crop < 0 || pc.crop >= ncrops) return;
    const CropJob& job = jobs[pc.crop];
    if (pc.frame < 0 || pc.frame >= job.nframes) return;
    (void)crop_unpack_one(job, job.frames[pc.frame], pc.seg0 + k, sym + slot * kDecodeS);
}

// The symbol word of (symbol row q, channel k) of frame fr of a crop, from the
// call's scratch; false when any index falls outside what the call unpacked.
__device__ __forceinline__ bool crop_symbol(const CropJob& job, const ResFrame& f, int fr, int64_t q, int k,
                                            const CropPiece* __restrict__ pieces, int npieces,
                                            const uint16_t* __restrict__ sym, int64_t nslots, uint32_t* w) {
    const int64_t si = q * f.ch + k;
    if (si < 0 || si >= f.nsym) return false;
    const int64_t pi = (int64_t)job.piece0 + (fr - job.f0);
    if (pi < 0 || pi >= npieces) return false;
    const CropPiece pc = pieces[pi];
    const int64_t rel = si / kDecodeS - pc.seg0;
    if (rel < 0 || rel >= pc.nseg) return false;
    const int64_t slot = pc.slot0 + rel;
    if (slot < 0 || slot >= nslots) return false;
    *w = sym[slot * kDecodeS + (si % kDecodeS)];
    return true;
}

template <typename T, bool PLANAR>
__global__ __launch_bounds__(kCropSynthThreads) void crop_synth_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                       const CropPiece* __restrict__ pieces,
                                                                       int npieces, const uint16_t* __restrict__ sym,
                                                                       int64_t nslots, int64_t length, int channels,
                                                                       T* __restrict__ out, int64_t nout) {
    const int64_t e = (int64_t)blockIdx.x * kCropSynthThreads + threadIdx.x;
    if (e >= nout) return;
    const int64_t per = length * channels;
    const int64_t crop = e / per, r = e - crop * per;
    int64_t t;
    int k;
    if (PLANAR) {
        k = (int)(r / length);
        t = r - (int64_t)k * length;
    } else {
        t = r / channels;
        k = (int)(r - t * channels);
    }
    int16_t val = 0;
    if (crop < ncrops) {
        const CropJob& job = jobs[crop];
        const int f0 = job.f0, f1 = job.f1;
        if (t < job.count && f0 >= 0 && f0 < f1 && f1 <= job.nframes) {
            const int64_t s = job.begin + t;
            const int fr = crop_frame_of(job, f0, f1, s);
            const ResFrame& f = job.frames[fr];
            const int cs = f.cs, count = f.count;
            const int64_t local = s - f.first_sample;
            uint32_t w;
            if (cs > 0 && count > 0 && k < f.ch && local >= 0 &&
                crop_symbol(job, f, fr, local / cs, k, pieces, npieces, sym, nslots, &w)) {
                val = table_sample(f, f.lut, w, (int)(local % cs), StagedTables{}, crop_tables(job));
            }
        }
    }
    out[e] = to_out<T>(val);
}

// The walk of the two tiled kernels.  A workgroup owns samples [t0, t1) of one
// crop's row, every channel: [t0, tc) are decoded, [tc, t1) lie past the
// crop's clipped length and are zeroed.  The frames that [t0, tc) crosses are
// taken one after another: frame(job, f, fr, ta, tb, write) writes the frame's
// share [ta, tb) with write(ua, ub, value), and puts its own barriers around
// what it keeps in LDS.  What no frame of a stale span covers is zeroed too.
template <typename T, bool PLANAR, int THREADS, typename Frame>
__device__ __forceinline__ void crop_walk_job(const CropJob& job, int64_t crop, int64_t tile, int64_t length,
                                              int channels, int tile_len, T* __restrict__ out, int64_t nout,
                                              Frame frame) {
    const int64_t t0 = tile * tile_len;
    const int64_t t1 = t0 + tile_len < length ? t0 + tile_len : length;
    if (t0 >= t1) return;
    const bool span_ok = job.f0 >= 0 && job.f0 < job.f1 && job.f1 <= job.nframes;
    const int64_t tc = !span_ok ? t0 : (job.count < t1 ? (job.count > t0 ? job.count : t0) : t1);
    const int64_t out_base = crop * length * channels;
    const int tid = threadIdx.x;
    auto write = [&](int64_t ua, int64_t ub, auto value) {
        crop_write_run<T, PLANAR>(ua, ub, channels, length, out_base, out, nout, tid, THREADS, value);
    };
    auto zero = [](int64_t, int) { return (int16_t)0; };
    write(tc, t1, zero);
    if (tc <= t0) return;
    const int fa = crop_frame_of(job, job.f0, job.f1, job.begin + t0);
    const int fb = crop_frame_of(job, job.f0, job.f1, job.begin + tc - 1);
    int64_t done = t0;  // every sample of [t0, done) is written
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        if (f.cs <= 0 || f.ch <= 0 || f.ch > 255 || f.count <= 0 || f.nsym <= 0) continue;
        // this frame's share of the run
        int64_t ta = f.first_sample - job.begin, tb = ta + f.nsym / f.ch * f.cs;
        ta = ta < done ? done : ta;
        tb = tb > tc ? tc : tb;
        if (ta >= tb) continue;
        write(done, ta, zero);
        frame(job, f, fr, ta, tb, write);
        done = tb;
    }
    write(done, tc, zero);
}

// crop_walk_job for the workgroup's tile of a call whose jobs the host planned
template <typename T, bool PLANAR, int THREADS, typename Frame>
__device__ __forceinline__ void crop_walk_tile(const CropJob* __restrict__ jobs, int ncrops, int64_t length,
                                               int channels, int tile_len, int tiles, T* __restrict__ out,
                                               int64_t nout, Frame frame) {
    if (tiles <= 0 || channels <= 0 || tile_len <= 0) return;
    const int64_t crop = blockIdx.x / tiles;
    if (crop >= ncrops) return;
    crop_walk_job<T, PLANAR, THREADS>(jobs[crop], crop, blockIdx.x - crop * tiles, length, channels, tile_len, out,
                                      nout, frame);
}

// A workgroup: a run of tile_len samples of one crop.  Each frame's codebook
// and attenuations are staged in LDS when they fit lds_bytes, read from global
// memory otherwise.
template <typename T, bool PLANAR>
__global__ __launch_bounds__(kDecodeSynthThreads) void crop_synth_lds_kernel(
    const CropJob* __restrict__ jobs, int ncrops, const CropPiece* __restrict__ pieces, int npieces,
    const uint16_t* __restrict__ sym, int64_t nslots, int64_t length, int channels, int tile_len, int tiles,
    int lds_bytes, T* __restrict__ out, int64_t nout) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int slut[32];
    const int tid = threadIdx.x;
    crop_walk_tile<T, PLANAR, kDecodeSynthThreads>(
        jobs, ncrops, length, channels, tile_len, tiles, out, nout,
        [&](const CropJob& job, const ResFrame& f, int fr, int64_t ta, int64_t tb, auto write) {
            const int cs = f.cs, ch = f.ch;
            const TableSlabs g = crop_tables(job);
            __syncthreads();  // the previous frame's tables are no longer read
            if (tid < 32) slut[tid] = f.lut[tid];
            const StagedTables lds = stage_tables(f, g, lds_bytes, smem, tid, kDecodeSynthThreads);
            __syncthreads();
            write(ta, tb, [&](int64_t t, int k) {
                const int64_t local = job.begin + t - f.first_sample;
                uint32_t w;
                if (k < ch && local >= 0 && crop_symbol(job, f, fr, local / cs, k, pieces, npieces, sym, nslots, &w))
                    return table_sample(f, slut, w, (int)(local % cs), lds, g);
                return (int16_t)0;
            });
        });
}

// The fused variant (fused_frame, gsc_decode_device.h): no symbol scratch and no unpack launch.
template <typename T, bool PLANAR>
__global__ __launch_bounds__(kFusedThreads) void crop_fused_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                   int64_t length, int channels, int tile_len,
                                                                   int tiles, T* __restrict__ out, int64_t nout) {
    __shared__ uint16_t ssym[kFusedSegs * kDecodeS];
    __shared__ int slut[32];
    crop_walk_tile<T, PLANAR, kFusedThreads>(jobs, ncrops, length, channels, tile_len, tiles, out, nout,
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
    crop_walk_job<T, PLANAR, kFusedThreads>(job, crop, tile, length, channels, tile_len, out, nout,
                                            fused_frame(ssym, slut, threadIdx.x));
}

template <typename T, bool PLANAR>
hipError_t launch_synth(const CropJob* jobs, int ncrops, const CropPiece* pieces, int npieces, const uint16_t* sym,
                        int64_t nslots, int64_t length, int channels, int lds_bytes, int tile_len, void* out,
                        hipStream_t st) {
    const int64_t nout = (int64_t)ncrops * length * channels;
    if (lds_bytes < 0) {
        const int64_t grid = (nout + kCropSynthThreads - 1) / kCropSynthThreads;
        if (grid > 0x7fffffff) return hipErrorInvalidValue;
        hipLaunchKernelGGL((crop_synth_kernel<T, PLANAR>), dim3((unsigned)grid), dim3(kCropSynthThreads), 0, st, jobs,
                           ncrops, pieces, npieces, sym, nslots, length, channels, static_cast<T*>(out), nout);
        return hipGetLastError();
    }
    if (lds_bytes > kDecodeLdsBytes || tile_len <= 0 || tile_len > (1 << 20) || channels > 255)
        return hipErrorInvalidValue;
    const int64_t tiles = (length + tile_len - 1) / tile_len;
    if (tiles * ncrops > 0x7fffffff) return hipErrorInvalidValue;
    static LdsLimit lim;  // one per instantiation
    const hipError_t e = allow_lds(crop_synth_lds_kernel<T, PLANAR>, lds_bytes, &lim);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((crop_synth_lds_kernel<T, PLANAR>), dim3((unsigned)(tiles * ncrops)),
                       dim3(kDecodeSynthThreads), (size_t)lds_bytes, st, jobs, ncrops, pieces, npieces, sym, nslots,
                       length, channels, tile_len, (int)tiles, lds_bytes, static_cast<T*>(out), nout);
    return hipGetLastError();
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

extern "C" hipError_t gsc_launch_crop_unpack(const CropJob* jobs, int ncrops, const CropPiece* pieces, int npieces,
                                             uint16_t* sym, int64_t nslots, hipStream_t st) {
    if (ncrops <= 0 || npieces <= 0 || nslots <= 0) return hipSuccess;
    const int64_t grid = (nslots + kCropUnpackThreads - 1) / kCropUnpackThreads;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crop_unpack_kernel, dim3((unsigned)grid), dim3(kCropUnpackThreads), 0, st, jobs, ncrops, pieces,
                       npieces, sym, nslots);
    return hipGetLastError();
}

// lds_bytes < 0: crop_synth_kernel (codebook from global memory); otherwise
// crop_synth_lds_kernel with that much dynamic LDS and tile_len samples per workgroup
extern "C" hipError_t gsc_launch_crop_synth(const CropJob* jobs, int ncrops, const CropPiece* pieces, int npieces,
                                            const uint16_t* sym, int64_t nslots, int64_t length, int channels,
                                            int is_float, int planar, int lds_bytes, int tile_len, void* out,
                                            hipStream_t st) {
    if (ncrops <= 0 || length <= 0 || channels <= 0) return hipSuccess;
    return dispatch_out(is_float, planar, [&](auto t, auto p) {
        return launch_synth<decltype(t), decltype(p)::value>(jobs, ncrops, pieces, npieces, sym, nslots, length,
                                                             channels, lds_bytes, tile_len, out, st);
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
