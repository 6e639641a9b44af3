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

constexpr int kResThreads = 256;
constexpr int kResSegs = 16;  // checkpoint segments of one stretch in LDS

// Samples [sa, sb) of a crop's stream, every channel, to
// ssrc[(s - ia) * ch + k], by a whole workgroup; what no frame covers stays as it is.
__device__ __forceinline__ void resample_fill(const CropJob& job, int64_t sa, int64_t sb, int64_t ia, int ch,
                                              int16_t* ssrc, int src_cap, uint16_t* ssym, int* slut, int tid) {
    const TableSlabs g = crop_tables(job);
    const int fa = crop_frame_of(job, job.f0, job.f1, sa);
    const int fb = crop_frame_of(job, job.f0, job.f1, sb - 1);
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        if (f.cs <= 0 || f.ch != ch || f.count <= 0 || f.nsym <= 0) continue;
        const int cs = f.cs;
        const int64_t fs = f.first_sample, fe = fs + f.nsym / ch * cs;
        const int64_t xa = sa > fs ? sa : fs, xb = sb < fe ? sb : fe;
        if (xa >= xb) continue;
        const int64_t qa = (xa - fs) / cs, qb = (xb - 1 - fs) / cs;
        // rows per stretch: their symbols span at most kResSegs segments wherever the stretch starts
        const int64_t rows = (int64_t)(kResSegs - 1) * kDecodeS / ch;
        for (int64_t q0 = qa; q0 <= qb; q0 += rows) {
            const int64_t q1 = q0 + rows - 1 < qb ? q0 + rows - 1 : qb;
            const int64_t seg_lo = q0 * ch / kDecodeS;
            int64_t nseg = ((q1 + 1) * ch - 1) / kDecodeS - seg_lo + 1;
            nseg = nseg > kResSegs ? kResSegs : nseg;
            __syncthreads();  // the previous stretch's symbols are no longer read
            if (tid < 32) slut[tid] = f.lut[tid];
            for (int i = tid; i < (int)nseg; i += kResThreads) {
                uint16_t* o = ssym + i * kDecodeS;
                if (!unpack_crop_segment(job, f, seg_lo + i, o))
                    for (int z = 0; z < kDecodeS; ++z) o[z] = 0;
            }
            __syncthreads();
            int64_t ua = fs + q0 * cs, ub = fs + (q1 + 1) * cs;
            ua = ua < xa ? xa : ua;
            ub = ub > xb ? xb : ub;
            const int64_t n = (ub - ua) * ch;
            for (int64_t l = tid; l < n; l += kResThreads) {
                const int64_t s = ua + l / ch;
                const int k = (int)(l % ch);
                const int64_t local = s - fs;
                const int64_t si = local / cs * ch + k, rel = si - seg_lo * kDecodeS;
                int16_t v = 0;
                if (rel >= 0 && rel < nseg * kDecodeS && si < f.nsym)
                    v = table_sample(f, slut, ssym[rel], (int)(local % cs), StagedTables{}, g);
                const int64_t di = (s - ia) * ch + k;
                if (di >= 0 && di < src_cap) ssrc[di] = v;
            }
        }
    }
}

// A workgroup's tile of one crop: outputs [tile * kResampleTile, + kResampleTile)
// of the crop's row.  ssrc holds src_cap int16, ssym kResSegs segments, slut 32 words.
template <typename T, bool PLANAR>
__device__ __forceinline__ void resample_tile(const CropJob& job, int64_t crop, int64_t tile, int64_t length,
                                              int channels, int src_cap, T* __restrict__ out, int64_t nout,
                                              int16_t* ssrc, uint16_t* ssym, int* slut) {
    const int tid = threadIdx.x;
    const int64_t t0 = tile * kResampleTile;
    const int64_t t1 = t0 + kResampleTile < length ? t0 + kResampleTile : length;
    if (t0 >= t1) return;
    const int L = job.rate_up, M = job.rate_down, H = job.half_taps, C = job.src_ch;
    const int taps = 2 * H, before = H > 0 ? H - 1 : 0;
    // what the 32-bit position arithmetic of a pass and the LDS indices rely on
    bool ok = job.f0 >= 0 && job.f0 < job.f1 && job.f1 <= job.nframes && L > 0 && L <= (1 << 17) && M > 0 &&
              M <= (1 << 21) && H >= 0 && taps <= kResampleMaxTaps && (H == 0 || job.table != nullptr) && C > 0 &&
              C <= 255 && job.out_ch == channels && (C == channels || C == 1 || channels == 1) && job.begin >= 0 &&
              job.begin <= ((int64_t)1 << 40) && job.src_begin >= 0 && job.src_begin <= job.src_end;
    const int64_t cap = ok ? src_cap / C : 0;  // source samples per channel of a pass
    ok = ok && cap - taps - 2 >= 0;
    // outputs per pass: n outputs read at most (n - 1) * M / L + taps + 2 source samples
    int64_t sub = ok ? (cap - taps - 2) * L / M + 1 : 1;
    sub = sub > kResampleTile ? kResampleTile : sub;
    const int64_t tc = !ok ? t0 : (job.count < t1 ? (job.count > t0 ? job.count : t0) : t1);
    const int64_t out_base = crop * length * channels;
    auto write = [&](int64_t ua, int64_t ub, auto value) {
        crop_write_run<T, PLANAR>(ua, ub, channels, length, out_base, out, nout, tid, kResThreads, value);
    };
    auto zero = [](int64_t, int) { return (int16_t)0; };
    write(tc, t1, zero);
    for (int64_t na = t0; na < tc; na += sub) {
        const int64_t nb = na + sub < tc ? na + sub : tc;
        // output n sits at source position (begin * L + n * M) / L; within a pass the offset fits 32 bits
        const int64_t p = job.begin * L + na * M;
        const int64_t bi = p / L;
        const uint32_t br = (uint32_t)(p - bi * L);
        const uint32_t ul = br + (uint32_t)(nb - 1 - na) * (uint32_t)M;
        const int64_t ia = bi - before, ib = bi + ul / (uint32_t)L + H;  // the span, both ends included
        const int64_t span = ib - ia + 1;
        if (span > cap) {  // never, by the choice of sub
            write(na, nb, zero);
            continue;
        }
        __syncthreads();  // the previous pass's span is no longer read
        for (int i = tid; i < (int)span * C; i += kResThreads) ssrc[i] = 0;
        __syncthreads();
        const int64_t sa = ia > job.src_begin ? ia : job.src_begin, sb = ib + 1 < job.src_end ? ib + 1 : job.src_end;
        if (sa < sb) resample_fill(job, sa, sb, ia, C, ssrc, (int)span * C, ssym, slut, tid);
        __syncthreads();
        // channel k of the output at offset u = br + (n - na) * M of the pass
        auto one = [&](uint32_t qi, const int32_t* __restrict__ row, int k) {
            const int16_t* x = ssrc + (int)qi * C + k;  // (qi + taps - 1) * C + k < span * C
            if (H == 0) return (int)x[0];
            int64_t acc = 0;
            for (int j = 0; j < taps; ++j) acc += (int64_t)row[j] * (int64_t)x[j * C];
            const int64_t y = (acc + ((int64_t)1 << (kResampleShift - 1))) >> kResampleShift;
            return (int)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
        };
        write(na, nb, [&](int64_t n, int c) {
            const uint32_t u = br + (uint32_t)(n - na) * (uint32_t)M;
            const uint32_t qi = u / (uint32_t)L, phase = u - qi * (uint32_t)L;
            const int32_t* row = job.table + (int64_t)phase * taps;
            if (C == channels) return (int16_t)one(qi, row, c);
            if (C == 1) return (int16_t)one(qi, row, 0);
            int sum = 0;  // channels == 1: the mean, rounded half up
            for (int k = 0; k < C; ++k) sum += one(qi, row, k);
            const int num = 2 * sum + C, den = 2 * C;
            int q = num / den;
            q -= (num % den < 0) ? 1 : 0;
            return (int16_t)q;
        });
    }
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
