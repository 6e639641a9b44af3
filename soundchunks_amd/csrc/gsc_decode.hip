// .gsc decode on MI355X (gfx950): SURVEY.md §8 f5, decoder/decoder.lpr:163-203.
//
//   decode_unpack_kernel  one lane per checkpoint segment (gsc_decode_index.cpp's
//                         walk leaves a checkpoint every kDecodeS symbols):
//                         reads the segment's bits from the compressed bytes
//                         and writes one u16 word per symbol,
//                         idx << 2 | neg << 1 | rev (pack_kernel's codes_out
//                         and recon_kernel's chunk word)
//   decode_verify_kernel  the same lanes and the same walk (walk_segment,
//                         gsc_decode_device.h) over a claimed seek table:
//                         nothing is written but one status word
//   expand_tables_kernel  one lane per 8 codebook values: a stream set's packed
//                         codebook codes and attenuation nibbles, already in
//                         the byte slab, to the int16 and byte tables the
//                         other kernels read (decoder.lpr:115-158)
//   decode_synth_kernel   one lane per output sample: the low 16 bits of
//                         (CAttrLookup[neg][att[idx]] * chunk[idx][j']) >> 15
//                         in 32-bit arithmetic (the reference wraps, it does
//                         not clamp), interleaved [sample][channel]
//
// The host validated every index and length; the kernels still clamp every
// index and check every slab bound, so a stale index cannot make them fault.
// The bytes are read as aligned 32-bit words of the byte slab (its base is
// allocation-aligned and its tail zero-padded), so a bitstream may start at
// any byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_launch.h"

namespace gsc {
namespace {

constexpr int kUnpackThreads = 256;

__global__ __launch_bounds__(kUnpackThreads) void decode_unpack_kernel(const DecFrame* __restrict__ frames, int nframes,
                                                                       const uint64_t* __restrict__ cps, int64_t ncp,
                                                                       const uint32_t* __restrict__ words,
                                                                       int64_t nwords, uint16_t* __restrict__ sym,
                                                                       int64_t nsym) {
    const int64_t c = (int64_t)blockIdx.x * kUnpackThreads + threadIdx.x;
    if (c >= ncp) return;
    // the last frame whose first checkpoint is <= c (empty frames own none)
    const DecFrame& f = frames[last_le(0, nframes - 1, c, [&](int i) { return frames[i].cp_first; })];
    const int64_t s0 = (c - f.cp_first) * kDecodeS;
    if (s0 < 0 || s0 >= f.nsym) return;
    const int n = (int)(f.nsym - s0 < kDecodeS ? f.nsym - s0 : kDecodeS);
    const int64_t so = f.sym_off + s0;
    if (so < 0 || so + n > nsym || f.bs_off < 0) return;
    unpack_segment(words, nwords, f.bs_off, cps[c], f.ver, f.count, n, sym + so);
}

// A claimed seek table against the stream (gsc_decode_index.cpp,
// index_from_table): one lane per checkpoint segment, the frame found as
// above.  The lane walks its segment from checkpoint c and must land on
// checkpoint c + 1 in bit offset and header state, or, in the frame's last
// segment, on the frame's claimed bit count (the header state is free there);
// no raw index may reach ChunkCount.  A frame's checkpoint 0 is (0, -1) by
// definition (the host checked it), so when no lane objects every checkpoint
// is the one the sequential walk would have left.  A lane that objects
// lowers *status to its checkpoint << 8 | reason: the smallest one wins,
// whichever lane comes first.
__global__ __launch_bounds__(kUnpackThreads) void decode_verify_kernel(const ResFrame* __restrict__ frames,
                                                                       const uint64_t* __restrict__ frame_bits,
                                                                       int nframes, const uint64_t* __restrict__ cps,
                                                                       int64_t ncp, const uint32_t* __restrict__ words,
                                                                       int64_t nwords,
                                                                       unsigned long long* __restrict__ status) {
    const int64_t c = (int64_t)blockIdx.x * kUnpackThreads + threadIdx.x;
    if (c >= ncp) return;
    const int fi = last_le(0, nframes - 1, c, [&](int i) { return frames[i].cp_first; });
    const ResFrame& f = frames[fi];
    const int64_t s0 = (c - f.cp_first) * kDecodeS;
    int reason = 0;
    if (s0 < 0 || s0 >= f.nsym || f.bs_off < 0) {
        reason = kVerifyBounds;
    } else {
        const int n = (int)(f.nsym - s0 < kDecodeS ? f.nsym - s0 : kDecodeS);
        const bool last = s0 + n == f.nsym;
        if (!last && c + 1 >= ncp) {
            reason = kVerifyBounds;
        } else {
            const int count = f.count;
            bool over = false;
            const WalkEnd end = walk_segment(words, nwords, f.bs_off, cps[c], f.ver, n,
                                             [&](int, int idx, uint32_t, uint32_t) { over |= idx >= count; });
            const uint64_t want = last ? make_checkpoint(frame_bits[fi], end.hdr) : cps[c + 1];
            const uint64_t got = make_checkpoint(end.bit, end.hdr);
            reason = over ? kVerifyIndex : (got >> 3) != (want >> 3) ? kVerifyBit : got != want ? kVerifyHeader : 0;
        }
    }
    if (reason) atomicMin(status, (unsigned long long)c << 8 | (unsigned long long)reason);
}

// A byte of the byte slab; zero outside it.
__device__ __forceinline__ int slab_byte(const uint8_t* __restrict__ bytes, int64_t nbytes, int64_t i) {
    return i >= 0 && i < nbytes ? (int)bytes[i] : 0;
}

// The tables of every frame of a stream set in one launch, value for value
// what frame_tables_expand (gsc_decode_index.cpp) writes on the host.  A
// frame's codebook occupies a multiple of 8 int16 from a cb_off that is a
// multiple of 8, so group g of 8 values belongs to one frame: the last one
// whose cb_off is <= 8 g (a frame without a codebook owns no group).  The lane
// writes the group with one 16-byte store, values past count * cs as zero, and
// attenuations [8 l, 8 l + 8) of its frame when l is its group within the
// frame: there are at least count / 8 groups, so every attenuation is written.
//   8 bit:  (b - 128) * 2047 / 127, truncated toward zero
//   12 bit: 3 bytes b0 b1 b2 -> (b1 | (b0 & 0xf0) << 4) - 2048, (b2 | (b0 & 0x0f) << 8) - 2048;
//           an odd ChunkSize ends each chunk with 2 bytes for one value
//   attenuations: high nibble first
// Cost accepted: every lane runs its own binary search over the frame table in
// global memory, and the 12-bit path divides a 64-bit index per value; the
// whole launch is 0.02 ms for 1024 streams, 1 % of an open.
__global__ __launch_bounds__(kUnpackThreads) void expand_tables_kernel(const ResFrame* __restrict__ frames,
                                                                       const TableSrc* __restrict__ src, int nframes,
                                                                       int64_t ngroups,
                                                                       const uint8_t* __restrict__ bytes,
                                                                       int64_t nbytes, int16_t* __restrict__ cb,
                                                                       int64_t ncb, uint8_t* __restrict__ att,
                                                                       int64_t natt) {
    const int64_t g = (int64_t)blockIdx.x * kUnpackThreads + threadIdx.x;
    if (g >= ngroups) return;
    const int fi = last_le(0, nframes - 1, g * 8, [&](int i) { return frames[i].cb_off; });
    const ResFrame& f = frames[fi];
    const TableSrc s = src[fi];
    const int cs = f.cs, count = f.count;
    const int64_t e0 = g * 8 - f.cb_off;  // the group's first value within the frame
    if (cs <= 0 || count <= 0 || e0 < 0 || (f.cb_off & 7) != 0) return;
    const int64_t n = (int64_t)count * cs;
    const int chunk_bytes = (cs / 2) * 3 + (cs & 1) * 2;
    uint32_t w[4] = {0u, 0u, 0u, 0u};  // the 8 values, two per word, low half first
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t e = e0 + k;
        int val = 0;
        if (e < n) {
            if (s.bd == 8) {
                val = (slab_byte(bytes, nbytes, s.cb_byte + e) - 128) * 2047 / 127;
            } else {
                const int64_t i = e / cs;
                const int j = (int)(e - i * cs);
                const int64_t p = s.cb_byte + i * chunk_bytes + (j / 2) * 3;
                const int b = slab_byte(bytes, nbytes, p);
                val = (j & 1) ? (slab_byte(bytes, nbytes, p + 2) | (b & 0x0f) << 8) - 2048
                              : (slab_byte(bytes, nbytes, p + 1) | (b & 0xf0) << 4) - 2048;
            }
        }
        w[k >> 1] |= (uint32_t)(uint16_t)(int16_t)val << (16 * (k & 1));
    }
    const int64_t o = f.cb_off + e0;
    if (o + 8 <= ncb) *reinterpret_cast<uint4*>(cb + o) = make_uint4(w[0], w[1], w[2], w[3]);
    const int64_t a0 = e0;  // 8 (e0 / 8): this lane's attenuations
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t a = a0 + k, ai = f.att_off + a;
        if (a >= count || ai < 0 || ai >= natt) continue;
        const int b = slab_byte(bytes, nbytes, s.att_byte + a / 2);
        att[ai] = (uint8_t)((a & 1) ? b & 0x0f : b >> 4);
    }
}

__global__ __launch_bounds__(kDecodeSynthThreads) void decode_synth_kernel(
    const DecFrame* __restrict__ frames, int nframes, const DecJob* __restrict__ jobs, int njobs, int lds_bytes,
    const uint16_t* __restrict__ sym, int64_t nsym, const int16_t* __restrict__ cb, int64_t ncb,
    const uint8_t* __restrict__ att, int64_t natt, int16_t* __restrict__ out, int64_t nout) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int slut[32];
    if ((int)blockIdx.x >= njobs) return;
    const DecJob job = jobs[blockIdx.x];
    if (job.frame < 0 || job.frame >= nframes) return;
    const DecFrame& f = frames[job.frame];
    const int cs = f.cs, ch = f.ch;
    if (cs <= 0 || ch <= 0 || f.count <= 0 || job.rows <= 0 || job.row0 < 0) return;
    const int row = cs * ch;
    if ((int64_t)job.rows * row > ((int64_t)1 << 30)) return;
    const int tid = threadIdx.x;
    if (tid < 32) slut[tid] = f.lut[tid];
    // the frame's codebook and attenuations in LDS when they fit
    const TableSlabs g{cb, ncb, att, natt};
    const StagedTables lds = stage_tables(f, g, lds_bytes, smem, tid, kDecodeSynthThreads);
    __syncthreads();
    const int total = job.rows * row;
    const int64_t sym_base = f.sym_off + job.row0 * ch;
    const int64_t out_base = f.out_off + job.row0 * row;
    for (int l = tid; l < total; l += kDecodeSynthThreads) {
        const int t = l / ch, k = l - t * ch;  // sample within the job, channel
        const int q = t / cs, j = t - q * cs;  // symbol row, sample within the chunk
        const int64_t si = sym_base + (int64_t)q * ch + k;
        const int64_t oi = out_base + l;
        if (si < 0 || si >= nsym || oi < 0 || oi >= nout) continue;
        out[oi] = table_sample(f, slut, sym[si], j, lds, g);
    }
}

}  // namespace
}  // namespace gsc

using namespace gsc;

extern "C" hipError_t gsc_launch_decode_unpack(const DecFrame* frames, int nframes, const uint64_t* cps, int64_t ncp,
                                               const uint32_t* words, int64_t nwords, uint16_t* sym, int64_t nsym,
                                               hipStream_t st) {
    if (nframes <= 0 || ncp <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((ncp + kUnpackThreads - 1) / kUnpackThreads);
    hipLaunchKernelGGL(decode_unpack_kernel, dim3(grid), dim3(kUnpackThreads), 0, st, frames, nframes, cps, ncp, words,
                       nwords, sym, nsym);
    return hipGetLastError();
}

// *status must hold kVerifyOk; frame_bits: the claimed bit count of every frame; *launched (may be
// null) is incremented when a kernel is launched
extern "C" hipError_t gsc_launch_decode_verify(const ResFrame* frames, const uint64_t* frame_bits, int nframes,
                                               const uint64_t* cps, int64_t ncp, const uint32_t* words, int64_t nwords,
                                               unsigned long long* status, hipStream_t st, int* launched) {
    if (nframes <= 0 || ncp <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((ncp + kUnpackThreads - 1) / kUnpackThreads);
    hipLaunchKernelGGL(decode_verify_kernel, dim3(grid), dim3(kUnpackThreads), 0, st, frames, frame_bits, nframes, cps,
                       ncp, words, nwords, status);
    if (launched) ++*launched;
    return hipGetLastError();
}

// Writes the codebook of every frame (its padding included) and every
// attenuation; the slabs' zero tails are the allocation's.  *launched (may be
// null) is incremented when the kernel is launched.
extern "C" hipError_t gsc_launch_expand_tables(const ResFrame* frames, const TableSrc* src, int nframes, int64_t ncb_used,
                                               const uint8_t* bytes, int64_t nbytes, int16_t* cb, int64_t ncb,
                                               uint8_t* att, int64_t natt, hipStream_t st, int* launched) {
    const int64_t ngroups = ncb_used / 8;
    if (nframes <= 0 || ngroups <= 0) return hipSuccess;
    if (ngroups > (int64_t(1) << 31) * kUnpackThreads - 1) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((ngroups + kUnpackThreads - 1) / kUnpackThreads);
    hipLaunchKernelGGL(expand_tables_kernel, dim3(grid), dim3(kUnpackThreads), 0, st, frames, src, nframes, ngroups,
                       bytes, nbytes, cb, ncb, att, natt);
    if (launched) ++*launched;
    return hipGetLastError();
}

extern "C" hipError_t gsc_launch_decode_synth(const DecFrame* frames, int nframes, const DecJob* jobs, int njobs,
                                              int lds_bytes, const uint16_t* sym, int64_t nsym, const int16_t* cb,
                                              int64_t ncb, const uint8_t* att, int64_t natt, int16_t* out, int64_t nout,
                                              hipStream_t st) {
    if (nframes <= 0 || njobs <= 0) return hipSuccess;
    if (lds_bytes < 0 || lds_bytes > kDecodeLdsBytes) return hipErrorInvalidValue;
    static LdsLimit lim;
    const hipError_t e = allow_lds(decode_synth_kernel, lds_bytes, &lim);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(decode_synth_kernel, dim3((unsigned)njobs), dim3(kDecodeSynthThreads), (size_t)lds_bytes, st,
                       frames, nframes, jobs, njobs, lds_bytes, sym, nsym, cb, ncb, att, natt, out, nout);
    return hipGetLastError();
}
