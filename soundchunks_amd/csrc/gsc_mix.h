// The arithmetic of a mix (gsc_crop_binding_mix, include/soundchunks.h has the
// definition), for the host and the device alike, as functions that compile
// with and without HIP: the mix kernels (gsc_decode_mix.hip) accumulate and
// round with them, gsc_mix_model (gsc_mix.cpp) is the same functions on the
// host.  tools/decode/mix_check.cpp holds them against 128-bit arithmetic.
#pragma once
#include <stdint.h>

#ifndef GSC_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GSC_HD __host__ __device__
#else
#define GSC_HD
#endif
#endif

namespace gsc {

constexpr int kMixMaxSources = 256;                // sources of one output row
constexpr int kMixGainShift = 15;                  // Q15: 1 << 15 is unity
constexpr int64_t kMixMaxGain = int64_t(1) << 20;  // |gain| <= 32 x unity
// 64-bit accumulator elements of one workgroup's tile in LDS (32 KiB): a tile
// holds kMixAccElems / channels output samples, at most kResampleTile of the
// resampling kernel
constexpr int kMixAccElems = 4096;

// Output samples of one workgroup's tile for a row of `channels` channels, at most max_tile.
GSC_HD inline int mix_tile_len(int channels, int max_tile) {
    const int fit = channels > 0 && channels <= kMixAccElems ? kMixAccElems / channels : 1;
    return fit < max_tile ? fit : max_tile;
}

GSC_HD inline bool mix_gain_ok(int64_t gain) { return gain >= -kMixMaxGain && gain <= kMixMaxGain; }

// One term of the sum.  |gain * x| <= 2^20 * 2^15, and kMixMaxSources of them
// stay below 2^43: nothing leaves 64 bits.
GSC_HD inline int64_t mix_term(int64_t gain, int16_t x) { return gain * int64_t(x); }

// The sum to an output sample: rounded half up (an arithmetic shift floors), clamped.
GSC_HD inline int16_t mix_round(int64_t sum) {
    const int64_t y = (sum + (int64_t(1) << (kMixGainShift - 1))) >> kMixGainShift;
    return int16_t(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
}

}  // namespace gsc
