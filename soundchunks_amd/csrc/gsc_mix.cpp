// gsc_mix_model: the mix arithmetic of gsc_mix.h on the host, so that its
// rounding and clamping can be held without a device.  Host only; builds with a
// host compiler alone (tools/decode/mix_check.cpp).
#include "gsc_mix.h"

extern "C" int gsc_mix_model(const int16_t* x, const long long* gain, int n, int16_t* y) {
    if (!x || !gain || !y || n < 1 || n > gsc::kMixMaxSources) return -1;
    int64_t sum = 0;
    for (int i = 0; i < n; ++i) {
        if (!gsc::mix_gain_ok(gain[i])) return -1;
        sum += gsc::mix_term(gain[i], x[i]);
    }
    *y = gsc::mix_round(sum);
    return 0;
}
