// The block and workgroup layout of a stream envelope and the reference
// descriptors of a fidelity call (gsc_envelope.h).  Host only: no device, no HIP.
#include "gsc_envelope.h"

namespace gsc {

int envelope_layout(const int64_t* samples, int n, int hop, int64_t* offsets, int64_t* tile0, std::string* err) {
    auto fail = [&](const std::string& m) {
        if (err) *err = m;
        return -1;
    };
    if (hop < kEnvelopeMinHop || hop > kEnvelopeMaxHop)
        return fail("gsc envelope: hop " + std::to_string(hop) + " outside [" + std::to_string(kEnvelopeMinHop) + ", " +
                    std::to_string(kEnvelopeMaxHop) + "]");
    if (n < 0 || (n > 0 && !samples) || !offsets) return fail("gsc envelope: invalid argument");
    const int64_t limit = int64_t(1) << 31;
    int64_t blocks = 0, tiles = 0;
    for (int i = 0; i < n; ++i) {
        if (samples[i] < 0)
            return fail("gsc envelope: stream " + std::to_string(i) + " has " + std::to_string(samples[i]) + " samples");
        const int64_t nb = envelope_blocks(samples[i], hop);
        if (nb >= limit - blocks)
            return fail("gsc envelope: stream " + std::to_string(i) + ": 2^31 or more blocks of " +
                        std::to_string(hop) + " samples in all");
        offsets[i] = blocks;
        if (tile0) tile0[i] = tiles;
        blocks += nb;
        tiles += envelope_tiles(nb, hop);
    }
    offsets[n] = blocks;
    if (tile0) tile0[n] = tiles;
    return 0;
}

int fidelity_refs(const void* const* pcm, const int64_t* samples, int n, FidelityRef* out, std::string* err) {
    auto fail = [&](const std::string& m) {
        if (err) *err = m;
        return -1;
    };
    if (n < 0 || (n > 0 && (!pcm || !samples || !out))) return fail("gsc fidelity: invalid argument");
    for (int i = 0; i < n; ++i) {
        if (samples[i] < 0)
            return fail("gsc fidelity: stream " + std::to_string(i) + ": the reference has " +
                        std::to_string(samples[i]) + " samples");
        if (!pcm[i] && samples[i] > 0)
            return fail("gsc fidelity: stream " + std::to_string(i) + ": the reference is null and has " +
                        std::to_string(samples[i]) + " samples");
        out[i] = FidelityRef{samples[i] > 0 ? static_cast<const int16_t*>(pcm[i]) : nullptr, samples[i]};
    }
    return 0;
}

}  // namespace gsc
