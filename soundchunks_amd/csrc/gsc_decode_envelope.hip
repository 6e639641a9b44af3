// Block energy and peak of resident .gsc streams on MI355X (gfx950), straight
// from the compressed slabs: gsc_crop_binding_envelope (include/soundchunks.h
// has the definition).  No PCM is written to memory.
//
//   envelope_kernel   a workgroup of 256 lanes owns one tile of one stream, a
//                     whole number of hops, finds it with tile_plan and decodes
//                     it with tile_walk (gsc_envelope_device.h, which
//                     fidelity_kernel shares), and a sample goes into the
//                     reduction below where the crop kernels store it.
//
// The reduction.  Consecutive lanes take consecutive elements (sample, channel)
// of a run, so the 64 elements of a wave lie in at most two blocks (a hop is at
// least 64 samples).  Each lane squares and takes |.| of its sample; the wave
// reduces the share of its first lane's block with shuffles, and the share of
// the next block only when a lane is in it; lane 0 of the wave adds the sums to
// the tile's LDS accumulators (one 64-bit sum and one 32-bit maximum per block
// of the tile, at most 64 of each) with LDS atomics.  Integer sums and maxima do
// not depend on the order.  The accumulators live from the workgroup's start to
// its end, across frames and stretches, and each block's two results are then
// written once with ordinary stores: zero where nothing decodes.
//
// Bounds: those of the crop kernels (every index clamped or checked against its
// slab), the stream index and the tile against the layout, an accumulator index
// against the tile's blocks and an output index against nblocks, so a stale
// descriptor gives zeros and cannot make the kernel fault.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_envelope.h"
#include "gsc_envelope_device.h"
#include "gsc_launch.h"

namespace gsc {
namespace {

// sum and maximum over the wave's 64 lanes, in every lane
__device__ __forceinline__ void wave_sum_max(unsigned long long* e, int* p) {
    for (int m = 32; m >= 1; m >>= 1) {
        *e += __shfl_xor(*e, m);
        const int q = __shfl_xor(*p, m);
        *p = q > *p ? q : *p;
    }
}

// value(t, k) of samples [ua, ub) of the tile, every channel, by a whole
// workgroup, into the accumulators of the blocks t / hop (nacc of them)
template <typename Value>
__device__ __forceinline__ void envelope_run(int64_t ua, int64_t ub, int ch, int hop, int nacc,
                                             unsigned long long* acc_e, int* acc_p, int tid, Value value) {
    const int n = (int)(ub - ua) * ch;
    const int first = (int)ua;
    // the trip count is the workgroup's: every lane of a wave is active in the shuffles
    for (int base = 0; base < n; base += kFusedThreads) {
        const int l = base + tid;
        const bool valid = l < n;
        const int t = first + (valid ? l / ch : 0);
        const int v = valid ? (int)value((int64_t)t, l % ch) : 0;
        const int blk = t / hop;
        const int b_lo = wave_uniform(blk);  // the first lane's: no lane of the wave is in an earlier block
        const bool hi = valid && blk != b_lo;
        const unsigned long long sq = (unsigned long long)(unsigned)(v * v);  // at most 2^30
        const int a = v < 0 ? -v : v;
        unsigned long long e_lo = hi ? 0ull : sq;
        int p_lo = hi ? 0 : a;
        wave_sum_max(&e_lo, &p_lo);
        unsigned long long e_hi = 0;
        int p_hi = 0;
        if (__ballot(hi) != 0ull) {  // alike in every lane of the wave
            e_hi = hi ? sq : 0ull;
            p_hi = hi ? a : 0;
            wave_sum_max(&e_hi, &p_hi);
        }
        if ((tid & 63) == 0) {
            if (p_lo > 0 && b_lo >= 0 && b_lo < nacc) {
                atomicAdd(&acc_e[b_lo], e_lo);
                atomicMax(&acc_p[b_lo], p_lo);
            }
            if (p_hi > 0 && b_lo + 1 >= 0 && b_lo + 1 < nacc) {
                atomicAdd(&acc_e[b_lo + 1], e_hi);
                atomicMax(&acc_p[b_lo + 1], p_hi);
            }
        }
    }
}

// layout: tile0[nstreams + 1] (stream i's first workgroup), then block0[nstreams + 1] (its first block)
__global__ __launch_bounds__(kFusedThreads) void envelope_kernel(const BoundStream* __restrict__ streams, int nstreams,
                                                                 const int64_t* __restrict__ layout, int hop,
                                                                 int64_t* __restrict__ energy,
                                                                 int32_t* __restrict__ peak, int64_t nblocks) {
    __shared__ uint16_t ssym[kFusedSegs * kDecodeS];
    __shared__ int slut[32];
    __shared__ SharedJob sjob;
    __shared__ TilePlace splace;
    __shared__ unsigned long long acc_e[kEnvelopeMaxBlocks];
    __shared__ int acc_p[kEnvelopeMaxBlocks];
    if (nstreams <= 0 || hop < kEnvelopeMinHop || hop > kEnvelopeMaxHop) return;
    const int tid = threadIdx.x;
    const int tile_len = envelope_tile_len(hop);
    const int bpt = tile_len / hop;  // 1 .. kEnvelopeMaxBlocks
    if (tid < kEnvelopeMaxBlocks) {
        acc_e[tid] = 0;
        acc_p[tid] = 0;
    }
    if (tid == 0) {
        CropJob j;
        TilePlace pl;
        tile_plan(streams, nstreams, layout, hop, blockIdx.x, &j, &pl);
        sjob.job = j;
        splace = pl;
    }
    __syncthreads();
    const CropJob job = shared_job_load(&sjob.job);
    const int64_t out_first = wave_uniform(splace.first);
    const int out_count = wave_uniform(splace.count);
    const int ch = job.src_ch;
    // the walk without its zeros: what no frame covers adds nothing to a sum of squares or a peak
    tile_walk(
        job, tile_samples(job, tile_len), ssym, slut, tid,
        [&](int64_t ua, int64_t ub, auto value) { envelope_run(ua, ub, ch, hop, bpt, acc_e, acc_p, tid, value); },
        [](int64_t, int64_t) {});
    __syncthreads();
    if (tid < out_count && tid < bpt) {
        const int64_t o = out_first + tid;
        if (o >= 0 && o < nblocks) {
            energy[o] = (int64_t)acc_e[tid];
            peak[o] = acc_p[tid];
        }
    }
}

}  // namespace
}  // namespace gsc

using namespace gsc;

// layout as envelope_kernel reads it, ntiles = tile0[nstreams]: one workgroup each
extern "C" hipError_t gsc_launch_envelope(const BoundStream* streams, int nstreams, const int64_t* layout,
                                          int64_t ntiles, int hop, int64_t* energy, int32_t* peak, int64_t nblocks,
                                          hipStream_t st) {
    if (nstreams <= 0 || ntiles <= 0 || nblocks <= 0) return hipSuccess;
    if (hop < kEnvelopeMinHop || hop > kEnvelopeMaxHop || ntiles > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(envelope_kernel, dim3((unsigned)ntiles), dim3(kFusedThreads), 0, st, streams, nstreams, layout,
                       hop, energy, peak, nblocks);
    return hipGetLastError();
}
