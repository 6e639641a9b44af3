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

#include <atomic>

#include "gsc_decode.h"
#include "gsc_decode_device.h"

namespace gsc {
namespace {

constexpr int kCropUnpackThreads = 256;
constexpr int kCropSynthThreads = 256;

// Segment seg of frame f of a crop's stream to o[0 .. kDecodeS); false (nothing
// written) when the segment or its checkpoint lies outside the stream's slabs.
__device__ __forceinline__ bool crop_unpack_one(const CropJob& job, const ResFrame& f, int64_t seg, uint16_t* o) {
    if (seg < 0 || seg > f.nsym / kDecodeS) return false;
    const int64_t s0 = seg * kDecodeS;
    if (s0 >= f.nsym) return false;
    const int n = (int)(f.nsym - s0 < kDecodeS ? f.nsym - s0 : kDecodeS);
    const int64_t c = f.cp_first + seg;
    if (c < 0 || c >= job.ncp || f.bs_off < 0) return false;
    unpack_segment(job.words, job.nwords, f.bs_off, job.cps[c], f.ver, f.count, n, o);
    return true;
}

__global__ __launch_bounds__(kCropUnpackThreads) void crop_unpack_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                         const CropPiece* __restrict__ pieces,
                                                                         int npieces, uint16_t* __restrict__ sym,
                                                                         int64_t nslots) {
    const int64_t slot = (int64_t)blockIdx.x * kCropUnpackThreads + threadIdx.x;
    if (slot >= nslots || npieces <= 0) return;
    // the last piece whose first slot is <= slot (an empty frame's piece owns none)
    int lo = 0, hi = npieces - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pieces[mid].slot0 <= slot) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    const CropPiece pc = pieces[lo];
    const int64_t k = slot - pc.slot0;
    if (k < 0 || k >= pc.nseg || pc.crop < 0 || pc.crop >= ncrops) return;
    const CropJob& job = jobs[pc.crop];
    if (pc.frame < 0 || pc.frame >= job.nframes) return;
    (void)crop_unpack_one(job, job.frames[pc.frame], pc.seg0 + k, sym + slot * kDecodeS);
}

template <typename T>
__device__ __forceinline__ T to_out(int16_t v);
template <>
__device__ __forceinline__ int16_t to_out<int16_t>(int16_t v) {
    return v;
}
template <>
__device__ __forceinline__ float to_out<float>(int16_t v) {
    return (float)v * (1.0f / 32768.0f);
}

// the frame of [f0, f1) that holds sample s: the last one whose first sample is <= s
__device__ __forceinline__ int crop_frame_of(const CropJob& job, int f0, int f1, int64_t s) {
    int lo = f0, hi = f1 - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (job.frames[mid].first_sample <= s) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
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

// One sample from a stream's tables in global memory, every index clamped to its slab.
__device__ __forceinline__ int16_t crop_value_global(const CropJob& job, const ResFrame& f, const int* lut, uint32_t w,
                                                     int j) {
    int idx, neg, jj;
    symbol_fields(w, f.count, f.cs, j, &idx, &neg, &jj);
    int64_t ai = f.att_off + idx, ci = f.cb_off + (int64_t)idx * f.cs + jj;
    ai = ai < 0 ? 0 : (ai >= job.natt ? job.natt - 1 : ai);
    ci = ci < 0 ? 0 : (ci >= job.ncb ? job.ncb - 1 : ci);
    return synth_sample(lut[neg * 16 + (job.att[ai] & 15)], job.cb[ci]);
}

// Element l of a run of nt samples x channels that starts at sample ta of a
// crop's row: its sample, its channel, and its place in the output.
template <bool PLANAR>
__device__ __forceinline__ int64_t crop_elem(int l, int nt, int64_t ta, int channels, int64_t length, int64_t out_base,
                                             int64_t* t, int* k) {
    if (PLANAR) {
        *k = l / nt;
        *t = ta + (l - *k * nt);
        return out_base + (int64_t)*k * length + *t;
    }
    *t = ta + l / channels;
    *k = l % channels;
    return out_base + *t * channels + *k;
}

// zeros for samples [ta, tb) of a crop's row, every channel
template <typename T, bool PLANAR>
__device__ __forceinline__ void crop_zero_run(int64_t ta, int64_t tb, int channels, int64_t length, int64_t out_base,
                                              T* __restrict__ out, int64_t nout, int tid, int threads) {
    const int nt = (int)(tb - ta);
    for (int l = tid; l < nt * channels; l += threads) {
        int64_t t;
        int k;
        const int64_t oi = crop_elem<PLANAR>(l, nt, ta, channels, length, out_base, &t, &k);
        if (oi >= 0 && oi < nout) out[oi] = to_out<T>(0);
    }
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
                val = crop_value_global(job, f, f.lut, w, (int)(local % cs));
            }
        }
    }
    out[e] = to_out<T>(val);
}

// What a workgroup of the two tiled kernels owns: samples [t0, t1) of one
// crop's row, every channel, of which [t0, tc) are decoded and [tc, t1) are
// past the crop's clipped length.  false: nothing to do.
struct CropTile {
    int64_t crop, t0, t1, tc, out_base;
};
__device__ __forceinline__ bool crop_tile(const CropJob* __restrict__ jobs, int ncrops, int64_t length, int channels,
                                          int tile_len, int tiles, CropTile* ct) {
    if (tiles <= 0 || channels <= 0 || tile_len <= 0) return false;
    ct->crop = blockIdx.x / tiles;
    if (ct->crop >= ncrops) return false;
    const CropJob& job = jobs[ct->crop];
    ct->t0 = (int64_t)(blockIdx.x - ct->crop * tiles) * tile_len;
    ct->t1 = ct->t0 + tile_len < length ? ct->t0 + tile_len : length;
    if (ct->t0 >= ct->t1) return false;
    const bool span_ok = job.f0 >= 0 && job.f0 < job.f1 && job.f1 <= job.nframes;
    ct->tc = !span_ok ? ct->t0 : (job.count < ct->t1 ? (job.count > ct->t0 ? job.count : ct->t0) : ct->t1);
    ct->out_base = ct->crop * length * channels;
    return true;
}

// A workgroup: a run of tile_len samples of one crop.  The frames the run
// crosses are taken one after another, each one's codebook and attenuations
// staged in LDS when they fit lds_bytes, read from global memory otherwise.
template <typename T, bool PLANAR>
__global__ __launch_bounds__(kDecodeSynthThreads) void crop_synth_lds_kernel(
    const CropJob* __restrict__ jobs, int ncrops, const CropPiece* __restrict__ pieces, int npieces,
    const uint16_t* __restrict__ sym, int64_t nslots, int64_t length, int channels, int tile_len, int tiles,
    int lds_bytes, T* __restrict__ out, int64_t nout) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int slut[32];
    CropTile ct;
    if (!crop_tile(jobs, ncrops, length, channels, tile_len, tiles, &ct)) return;
    const int tid = threadIdx.x;
    const CropJob& job = jobs[ct.crop];
    crop_zero_run<T, PLANAR>(ct.tc, ct.t1, channels, length, ct.out_base, out, nout, tid, kDecodeSynthThreads);
    if (ct.tc <= ct.t0) return;
    const int fa = crop_frame_of(job, job.f0, job.f1, job.begin + ct.t0);
    const int fb = crop_frame_of(job, job.f0, job.f1, job.begin + ct.tc - 1);
    int64_t done = ct.t0;  // every sample of [t0, done) is written
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        const int cs = f.cs, ch = f.ch, count = f.count;
        if (cs <= 0 || ch <= 0 || count <= 0 || f.nsym <= 0) continue;
        // this frame's share of the run
        int64_t ta = f.first_sample - job.begin, tb = ta + f.nsym / ch * cs;
        ta = ta < done ? done : ta;
        tb = tb > ct.tc ? ct.tc : tb;
        if (ta >= tb) continue;
        __syncthreads();  // the previous frame's tables are no longer read
        if (tid < 32) slut[tid] = f.lut[tid];
        const int64_t cbn = (int64_t)count * cs;
        const int64_t att_at = (cbn * 2 + 3) & ~(int64_t)3;
        const bool staged = att_at + count <= lds_bytes && f.cb_off >= 0 && (f.cb_off & 1) == 0 &&
                            f.cb_off + cbn + 1 <= job.ncb && f.att_off >= 0 && f.att_off + count <= job.natt;
        const int16_t* lcb = reinterpret_cast<const int16_t*>(smem);
        const uint8_t* latt = smem + att_at;
        if (staged) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(job.cb + f.cb_off);
            uint32_t* dst = reinterpret_cast<uint32_t*>(smem);
            const int nw = (int)((cbn + 1) / 2);
            for (int i = tid; i < nw; i += kDecodeSynthThreads) dst[i] = src[i];
            for (int i = tid; i < count; i += kDecodeSynthThreads) smem[att_at + i] = job.att[f.att_off + i];
        }
        __syncthreads();
        crop_zero_run<T, PLANAR>(done, ta, channels, length, ct.out_base, out, nout, tid, kDecodeSynthThreads);
        const int nt = (int)(tb - ta);
        for (int l = tid; l < nt * channels; l += kDecodeSynthThreads) {
            int64_t t;
            int k;
            const int64_t oi = crop_elem<PLANAR>(l, nt, ta, channels, length, ct.out_base, &t, &k);
            if (oi < 0 || oi >= nout) continue;
            const int64_t local = job.begin + t - f.first_sample;
            int16_t val = 0;
            uint32_t w;
            if (k < ch && local >= 0 && crop_symbol(job, f, fr, local / cs, k, pieces, npieces, sym, nslots, &w)) {
                const int j = (int)(local % cs);
                if (staged) {
                    int idx, neg, jj;
                    symbol_fields(w, count, cs, j, &idx, &neg, &jj);
                    val = synth_sample(slut[neg * 16 + (latt[idx] & 15)], lcb[idx * cs + jj]);
                } else {
                    val = crop_value_global(job, f, slut, w, j);
                }
            }
            out[oi] = to_out<T>(val);
        }
        done = tb;
    }
    // what no frame of a stale span covered
    crop_zero_run<T, PLANAR>(done, ct.tc, channels, length, ct.out_base, out, nout, tid, kDecodeSynthThreads);
}

// The fused variant: no symbol scratch and no unpack launch.  A workgroup
// takes a run of tile_len samples of one crop; per frame the run crosses, and
// per stretch of symbol rows whose symbols span at most kFusedSegs checkpoint
// segments, its first lanes unpack those segments into LDS (one lane per
// segment, as crop_unpack_kernel), then all lanes write the stretch's samples
// with the codebook read from global memory.
constexpr int kFusedThreads = 256;
constexpr int kFusedSegs = 64;

template <typename T, bool PLANAR>
__global__ __launch_bounds__(kFusedThreads) void crop_fused_kernel(const CropJob* __restrict__ jobs, int ncrops,
                                                                   int64_t length, int channels, int tile_len,
                                                                   int tiles, T* __restrict__ out, int64_t nout) {
    __shared__ uint16_t ssym[kFusedSegs * kDecodeS];
    __shared__ int slut[32];
    CropTile ct;
    if (!crop_tile(jobs, ncrops, length, channels, tile_len, tiles, &ct)) return;
    const int tid = threadIdx.x;
    const CropJob& job = jobs[ct.crop];
    crop_zero_run<T, PLANAR>(ct.tc, ct.t1, channels, length, ct.out_base, out, nout, tid, kFusedThreads);
    if (ct.tc <= ct.t0) return;
    const int fa = crop_frame_of(job, job.f0, job.f1, job.begin + ct.t0);
    const int fb = crop_frame_of(job, job.f0, job.f1, job.begin + ct.tc - 1);
    int64_t done = ct.t0;
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        const int cs = f.cs, ch = f.ch, count = f.count;
        if (cs <= 0 || ch <= 0 || ch > 255 || count <= 0 || f.nsym <= 0) continue;
        int64_t ta = f.first_sample - job.begin, tb = ta + f.nsym / ch * cs;
        ta = ta < done ? done : ta;
        tb = tb > ct.tc ? ct.tc : tb;
        if (ta >= tb) continue;
        crop_zero_run<T, PLANAR>(done, ta, channels, length, ct.out_base, out, nout, tid, kFusedThreads);
        const int64_t off = job.begin - f.first_sample;  // sample of the frame = off + t
        const int64_t qa = (off + ta) / cs, qb = (off + tb - 1) / cs;
        // rows per stretch: their symbols span at most kFusedSegs segments wherever the stretch starts
        const int64_t rows = (int64_t)(kFusedSegs - 1) * kDecodeS / ch;
        for (int64_t q0 = qa; q0 <= qb; q0 += rows) {
            const int64_t q1 = q0 + rows - 1 < qb ? q0 + rows - 1 : qb;
            const int64_t seg_lo = q0 * ch / kDecodeS;
            int64_t nseg = ((q1 + 1) * ch - 1) / kDecodeS - seg_lo + 1;
            nseg = nseg > kFusedSegs ? kFusedSegs : nseg;
            __syncthreads();  // the previous stretch's symbols are no longer read
            if (tid < 32) slut[tid] = f.lut[tid];
            for (int i = tid; i < (int)nseg; i += kFusedThreads) {
                uint16_t* o = ssym + i * kDecodeS;
                if (!crop_unpack_one(job, f, seg_lo + i, o))
                    for (int z = 0; z < kDecodeS; ++z) o[z] = 0;
            }
            __syncthreads();
            int64_t ua = q0 * cs - off, ub = (q1 + 1) * cs - off;
            ua = ua < ta ? ta : ua;
            ub = ub > tb ? tb : ub;
            const int nt = (int)(ub - ua);
            for (int l = tid; l < nt * channels; l += kFusedThreads) {
                int64_t t;
                int k;
                const int64_t oi = crop_elem<PLANAR>(l, nt, ua, channels, length, ct.out_base, &t, &k);
                if (oi < 0 || oi >= nout) continue;
                const int64_t local = off + t;
                const int64_t rel = local / cs * ch + k - seg_lo * kDecodeS;  // the symbol's place in ssym
                int16_t val = 0;
                if (k < ch && local >= 0 && rel >= 0 && rel < nseg * kDecodeS && local / cs * ch + k < f.nsym)
                    val = crop_value_global(job, f, slut, ssym[rel], (int)(local % cs));
                out[oi] = to_out<T>(val);
            }
        }
        done = tb;
    }
    crop_zero_run<T, PLANAR>(done, ct.tc, channels, length, ct.out_base, out, nout, tid, kFusedThreads);
}

// the dynamic LDS a kernel may use is raised once per kernel and size, not per launch
template <typename K>
hipError_t allow_lds(K kernel, int lds_bytes, std::atomic<int>* allowed) {
    if (lds_bytes <= 32 * 1024 || lds_bytes <= allowed->load(std::memory_order_relaxed)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e == hipSuccess) allowed->store(lds_bytes, std::memory_order_relaxed);
    return e;
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
    static std::atomic<int> allowed{0};  // one per instantiation
    const hipError_t e = allow_lds(crop_synth_lds_kernel<T, PLANAR>, lds_bytes, &allowed);
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

}  // namespace
}  // namespace gsc

using namespace gsc;

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
    if (is_float)
        return planar ? launch_synth<float, true>(jobs, ncrops, pieces, npieces, sym, nslots, length, channels,
                                                  lds_bytes, tile_len, out, st)
                      : launch_synth<float, false>(jobs, ncrops, pieces, npieces, sym, nslots, length, channels,
                                                   lds_bytes, tile_len, out, st);
    return planar ? launch_synth<int16_t, true>(jobs, ncrops, pieces, npieces, sym, nslots, length, channels,
                                                lds_bytes, tile_len, out, st)
                  : launch_synth<int16_t, false>(jobs, ncrops, pieces, npieces, sym, nslots, length, channels,
                                                 lds_bytes, tile_len, out, st);
}

// unpack and synthesis in one launch, tile_len samples of a crop per workgroup
extern "C" hipError_t gsc_launch_crop_fused(const CropJob* jobs, int ncrops, int64_t length, int channels,
                                            int is_float, int planar, int tile_len, void* out, hipStream_t st) {
    if (ncrops <= 0 || length <= 0 || channels <= 0) return hipSuccess;
    if (is_float)
        return planar ? launch_fused<float, true>(jobs, ncrops, length, channels, tile_len, out, st)
                      : launch_fused<float, false>(jobs, ncrops, length, channels, tile_len, out, st);
    return planar ? launch_fused<int16_t, true>(jobs, ncrops, length, channels, tile_len, out, st)
                  : launch_fused<int16_t, false>(jobs, ncrops, length, channels, tile_len, out, st);
}
