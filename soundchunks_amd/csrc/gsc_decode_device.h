// Device code the decode kernels share (gsc_decode.hip, gsc_decode_crops.hip):
// the bit walk of one checkpoint segment and the sample arithmetic, each in
// one place (decoder/decoder.lpr:163-203).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"

namespace gsc {

// Walks n symbols (n <= kDecodeS) from checkpoint cp of a bitstream that
// starts at byte bs_off of the word slab, and writes one word per symbol,
// idx << 2 | neg << 1 | rev, to o[0 .. n).  The bytes are read as aligned
// 32-bit words; a word past nwords reads as zero, an index past count - 1 is
// clamped.  The caller checked bs_off >= 0 and that o holds n words.
__device__ __forceinline__ void unpack_segment(const uint32_t* __restrict__ words, int64_t nwords, int64_t bs_off,
                                               uint64_t cp, int ver, int count, int n, uint16_t* o) {
    int hdr = (int)(cp & 7) - 1;  // variableCodingHeader on entry
    hdr = hdr > 3 ? 3 : hdr;
    const uint64_t bit = (cp >> 3) + (uint64_t)bs_off * 8;
    int64_t w = (int64_t)(bit >> 5);
    const int sh = (int)(bit & 31);
    const int rev_bit = ver > 0 ? 1 : 0;
    const int idx_max = count > 0 ? count - 1 : 0;
    uint64_t buf = (w >= 0 && w < nwords ? words[w] : 0u) >> sh;
    int have = 32 - sh;
    ++w;
    for (int i = 0; i < n; ++i) {
        if (have <= 32) {  // refill: 33 bits or more, a symbol has at most 17
            buf |= (uint64_t)(w >= 0 && w < nwords ? words[w] : 0u) << have;
            have += 32;
            ++w;
        }
        const uint32_t v = (uint32_t)buf;
        const uint32_t neg = v & 1u;
        const uint32_t rev = rev_bit ? (v >> 1) & 1u : 0u;
        int used = 1 + rev_bit;
        const int has = (int)((v >> used) & 1u);
        const int nh = (int)((v >> (used + 1)) & 3u);
        hdr = has ? nh : hdr;
        used += 1 + 2 * has;
        // the next four 3-bit blocks, first block most significant; the hdr + 1
        // leading ones are the index (no per-lane trip count: lanes stay converged)
        const uint32_t g = v >> used;
        const uint32_t r4 = (g & 7u) << 9 | ((g >> 3) & 7u) << 6 | ((g >> 6) & 7u) << 3 | ((g >> 9) & 7u);
        int idx = (int)(r4 >> (3 * (3 - hdr)));
        used += 3 * (hdr + 1);
        buf >>= used;
        have -= used;
        idx = idx > idx_max ? idx_max : idx;
        o[i] = (uint16_t)((uint32_t)idx << 2 | neg << 1 | rev);
    }
}

// The fields of a symbol word for sample j of its chunk: the chunk index
// (clamped to count - 1), the negate flag, and j mirrored when the chunk is reversed.
__device__ __forceinline__ void symbol_fields(uint32_t w, int count, int cs, int j, int* idx, int* neg, int* jj) {
    const int i = (int)(w >> 2);
    *idx = i >= count ? count - 1 : i;
    *neg = (int)((w >> 1) & 1u);
    *jj = (w & 1u) ? cs - 1 - j : j;
}

// Cardinal(attr * chunkSmp) shr 15, low word (decoder.lpr:198-201): the
// product wraps in 32 bits, it is not clamped
__device__ __forceinline__ int16_t synth_sample(int lut, int v) {
    return (int16_t)(uint16_t)(((uint32_t)(lut * v)) >> 15);
}

}  // namespace gsc
