// Block error energy of resident .gsc streams against their source PCM on
// MI355X (gfx950), straight from the compressed slabs:
// gsc_crop_binding_fidelity (include/soundchunks.h has the definition).  No PCM
// is written to memory.
//
//   fidelity_kernel   envelope_kernel's tiles, layout search, plan and walk
//                     (tile_plan, tile_walk: gsc_envelope_device.h), with a
//                     second operand: a decoded sample x meets its reference
//                     sample r on the way into the reduction.
//
// The reduction.  Consecutive lanes take consecutive elements (sample, channel)
// of a run, which are consecutive int16 of the interleaved reference too: a wave
// reads 128 contiguous bytes of it, one 2-byte load per lane, zero past the
// reference's end.  Each lane forms d = x - r, d^2 (below 2^32, so an unsigned
// 32-bit product widened), r^2 and |d|.  The 64 elements of a wave lie in at
// most two blocks (a hop is at least 64 samples): the wave reduces the share of
// its first lane's block with shuffles, two 64-bit sums and one 32-bit maximum,
// and the share of the next block only when a lane is in it; lane 0 of the wave
// adds them to the tile's LDS accumulators (per block of the tile two 64-bit
// sums and one 32-bit maximum, at most 64 of each) with LDS atomics, each
// quantity only when the wave's share of it is not zero: a wave whose samples
// all equal the reference still carries reference energy.  What no frame covers
// decodes to zero and goes through the same reduction, so every sample of the
// stream meets its reference.  Integer sums and maxima do not depend on the
// order.  Each block's three results are written once with ordinary stores.
//
// Bounds: the envelope kernel's, and an element of the reference is read only
// when its sample lies in [0, R), R from the call's descriptor of the stream
// the layout search found, so a stale descriptor gives zeros and cannot make
// the kernel fault.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_envelope.h"
#include "gsc_envelope_device.h"
#include "gsc_launch.h"

namespace gsc {
namespace {

// two sums and a maximum over the wave's 64 lanes, in every lane
__device__ __forceinline__ void wave_sum2_max(unsigned long long* e, unsigned long long* q, int* p) {
    for (int m = 32; m >= 1; m >>= 1) {
        *e += __shfl_xor(*e, m);
        *q += __shfl_xor(*q, m);
        const int o = __shfl_xor(*p, m);
        *p = o > *p ? o : *p;
    }
}

// the tile's accumulators: per block the error energy, the reference energy and the largest error
struct FidelityAcc {
    unsigned long long* err;
    unsigned long long* ref;
    int* peak;
    int count;  // blocks of the tile
};

// value(t, k) of samples [ua, ub) of the tile, every channel, by a whole
// workgroup, against ref[(begin + t) * ch + k] (zero from sample nref on), into
// the accumulators of the blocks t / hop.  begin: the tile's first sample.
template <typename Value>
__device__ __forceinline__ void fidelity_run(int64_t ua, int64_t ub, int ch, int hop, int64_t begin,
                                             const int16_t* __restrict__ ref, int64_t nref, const FidelityAcc& acc,
                                             int tid, Value value) {
    const int n = (int)(ub - ua) * ch;
    const int first = (int)ua;
    // the trip count is the workgroup's: every lane of a wave is active in the shuffles
    for (int base = 0; base < n; base += kFusedThreads) {
        const int l = base + tid;
        const bool valid = l < n;
        const int t = first + (valid ? l / ch : 0);
        const int k = valid ? l % ch : 0;
        const int64_t s = begin + t;  // the sample of the stream
        const int r = valid && s >= 0 && s < nref ? (int)ref[s * ch + k] : 0;
        const int v = valid ? (int)value((int64_t)t, k) : 0;
        const int d = v - r;  // |d| <= 65535
        const int blk = t / hop;
        const int b_lo = wave_uniform(blk);  // the first lane's: no lane of the wave is in an earlier block
        const bool hi = valid && blk != b_lo;
        const unsigned a = (unsigned)(d < 0 ? -d : d);
        const unsigned long long sq = (unsigned long long)(a * a);            // at most 65535^2 < 2^32
        const unsigned long long rr = (unsigned long long)(unsigned)(r * r);  // at most 2^30
        unsigned long long e_lo = hi ? 0ull : sq, q_lo = hi ? 0ull : rr;
        int p_lo = hi ? 0 : (int)a;
        wave_sum2_max(&e_lo, &q_lo, &p_lo);
        unsigned long long e_hi = 0, q_hi = 0;
        int p_hi = 0;
        if (__ballot(hi) != 0ull) {  // alike in every lane of the wave
            e_hi = hi ? sq : 0ull;
            q_hi = hi ? rr : 0ull;
            p_hi = hi ? (int)a : 0;
            wave_sum2_max(&e_hi, &q_hi, &p_hi);
        }
        if ((tid & 63) == 0) {
            if (b_lo >= 0 && b_lo < acc.count) {
                if (p_lo > 0) {
                    atomicAdd(&acc.err[b_lo], e_lo);
                    atomicMax(&acc.peak[b_lo], p_lo);
                }
                if (q_lo != 0ull) atomicAdd(&acc.ref[b_lo], q_lo);
            }
            if (b_lo + 1 >= 0 && b_lo + 1 < acc.count) {
                if (p_hi > 0) {
                    atomicAdd(&acc.err[b_lo + 1], e_hi);
                    atomicMax(&acc.peak[b_lo + 1], p_hi);
                }
                if (q_hi != 0ull) atomicAdd(&acc.ref[b_lo + 1], q_hi);
            }
        }
    }
}

// layout as envelope_kernel reads it; refs[nstreams]: every stream's reference
__global__ __launch_bounds__(kFusedThreads) void fidelity_kernel(const BoundStream* __restrict__ streams, int nstreams,
                                                                 const int64_t* __restrict__ layout,
                                                                 const FidelityRef* __restrict__ refs, int hop,
                                                                 int64_t* __restrict__ err_energy,
                                                                 int64_t* __restrict__ ref_energy,
                                                                 int32_t* __restrict__ err_peak, int64_t nblocks) {
    __shared__ uint16_t ssym[kFusedSegs * kDecodeS];
    __shared__ int slut[32];
    __shared__ SharedJob sjob;
    __shared__ TilePlace splace;
    __shared__ FidelityRef sref;
    __shared__ unsigned long long acc_e[kEnvelopeMaxBlocks];
    __shared__ unsigned long long acc_r[kEnvelopeMaxBlocks];
    __shared__ int acc_p[kEnvelopeMaxBlocks];
    if (nstreams <= 0 || hop < kEnvelopeMinHop || hop > kEnvelopeMaxHop) return;
    const int tid = threadIdx.x;
    const int tile_len = envelope_tile_len(hop);
    const int bpt = tile_len / hop;  // 1 .. kEnvelopeMaxBlocks
    if (tid < kEnvelopeMaxBlocks) {
        acc_e[tid] = 0;
        acc_r[tid] = 0;
        acc_p[tid] = 0;
    }
    if (tid == 0) {
        CropJob j;
        TilePlace pl;
        tile_plan(streams, nstreams, layout, hop, blockIdx.x, &j, &pl);
        sjob.job = j;
        splace = pl;
        // pl.stream is in [0, nstreams); a null reference has no samples to read
        FidelityRef r = refs[pl.stream];
        if (!r.pcm || r.samples < 0) r = FidelityRef{nullptr, 0};
        sref = r;
    }
    __syncthreads();
    const CropJob job = shared_job_load(&sjob.job);
    const int64_t out_first = wave_uniform(splace.first);
    const int out_count = wave_uniform(splace.count);
    const int16_t* ref = wave_uniform(sref.pcm);
    const int64_t nref = wave_uniform(sref.samples);
    const int ch = job.src_ch;
    const FidelityAcc acc{acc_e, acc_r, acc_p, bpt};
    auto run = [&](int64_t ua, int64_t ub, auto value) {
        fidelity_run(ua, ub, ch, hop, job.begin, ref, nref, acc, tid, value);
    };
    tile_walk(job, tile_samples(job, tile_len), ssym, slut, tid, run, [&](int64_t ua, int64_t ub) {
        if (ua < ub) run(ua, ub, [](int64_t, int) { return (int16_t)0; });
    });
    __syncthreads();
    if (tid < out_count && tid < bpt) {
        const int64_t o = out_first + tid;
        if (o >= 0 && o < nblocks) {
            err_energy[o] = (int64_t)acc_e[tid];
            ref_energy[o] = (int64_t)acc_r[tid];
            err_peak[o] = acc_p[tid];
        }
    }
}

}  // namespace
}  // namespace gsc

using namespace gsc;

// layout as fidelity_kernel reads it, ntiles = tile0[nstreams]: one workgroup each
extern "C" hipError_t gsc_launch_fidelity(const BoundStream* streams, int nstreams, const int64_t* layout,
                                          int64_t ntiles, const FidelityRef* refs, int hop, int64_t* err_energy,
                                          int64_t* ref_energy, int32_t* err_peak, int64_t nblocks, hipStream_t st) {
    if (nstreams <= 0 || ntiles <= 0 || nblocks <= 0) return hipSuccess;
    if (hop < kEnvelopeMinHop || hop > kEnvelopeMaxHop || ntiles > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fidelity_kernel, dim3((unsigned)ntiles), dim3(kFusedThreads), 0, st, streams, nstreams, layout,
                       refs, hop, err_energy, ref_energy, err_peak, nblocks);
    return hipGetLastError();
}
