// Stream envelopes and stream fidelity (include/soundchunks.h has the
// definitions): how the blocks of a binding's streams are laid out and how
// envelope_kernel (gsc_decode_envelope.hip) and fidelity_kernel
// (gsc_decode_fidelity.hip) split them into workgroups, for the host and the
// device alike, and the reference descriptors of a fidelity call.
// tools/decode/envelope_check.cpp and fidelity_check.cpp check them without a
// device.
#pragma once
#include <stdint.h>

#include <string>

#include "gsc_crop_plan.h"

namespace gsc {

constexpr int kEnvelopeMinHop = 64;
constexpr int kEnvelopeMaxHop = 65536;
constexpr int kEnvelopeTile = 4096;     // samples of one workgroup when a hop is no longer
constexpr int kEnvelopeMaxBlocks = kEnvelopeTile / kEnvelopeMinHop;  // of one tile: its LDS accumulators

// The samples one workgroup owns: a whole number of hops, the largest multiple
// of hop not above kEnvelopeTile, or one hop.  So a block never has two owners.
GSC_HD constexpr int envelope_tile_len(int hop) { return hop > kEnvelopeTile ? hop : kEnvelopeTile / hop * hop; }
// ceil(samples / hop) without the sum
GSC_HD constexpr int64_t envelope_blocks(int64_t samples, int hop) { return samples / hop + (samples % hop != 0); }
// workgroups of a stream of nb blocks
GSC_HD constexpr int64_t envelope_tiles(int64_t nb, int hop) {
    return (nb + envelope_tile_len(hop) / hop - 1) / (envelope_tile_len(hop) / hop);
}

// offsets[i]: the first block of stream i, offsets[n] the total; tile0 (may be
// null) the same for workgroups.  Refuses (-1, *err) hop outside
// [kEnvelopeMinHop, kEnvelopeMaxHop], n < 0, a negative length and 2^31 or more
// blocks in all.  Host only.
int envelope_layout(const int64_t* samples, int n, int hop, int64_t* offsets, int64_t* tile0, std::string* err);

// The reference of one stream of a fidelity call as fidelity_kernel reads it:
// int16 [samples, channels of the stream] interleaved in device memory; null
// with 0 samples is an all-zero reference.
struct FidelityRef {
    const int16_t* pcm;
    int64_t samples;
};
static_assert(sizeof(FidelityRef) == 16, "two int64 of the call's upload per stream");

// out[i] for n streams from the call's host arrays.  Refuses (-1, *err, the
// stream named) a negative length and a null pointer with a positive length; a
// pointer with 0 samples is kept as null, so that nothing can be read through
// it.  Host only.
int fidelity_refs(const void* const* pcm, const int64_t* samples, int n, FidelityRef* out, std::string* err);

}  // namespace gsc
