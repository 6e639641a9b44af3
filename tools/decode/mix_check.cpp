// Stand-alone driver of the mix arithmetic (gsc_mix.h) and of gsc_mix_model
// (gsc_mix.cpp), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc mix_check
// Unity and inversion over every int16, the half-way round, both clamps, the
// extremes (256 terms of the largest gain times either rail: the sum stays in
// 64 bits, which the undefined-behaviour sanitizer would report otherwise),
// random terms, all against sums formed in 128 bits with a floor division of
// the check's own, the tile rule, and the refusals, which write nothing.
// Exit status 0 when nothing failed.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_mix.h"

extern "C" int gsc_mix_model(const int16_t* x, const long long* gain, int n, int16_t* y);

namespace {

int g_bad = 0;

#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                  \
            std::printf("\n");                                         \
            ++g_bad;                                                   \
            return;                                                    \
        }                                                              \
    } while (0)

// the definition, with nothing shared with gsc_mix.h: a 128-bit sum, floor((s + 16384) / 32768) by division
int16_t model(const std::vector<int16_t>& x, const std::vector<long long>& g) {
    __int128 s = 0;
    for (size_t i = 0; i < x.size(); ++i) s += (__int128)g[i] * (__int128)x[i];
    s += 16384;
    __int128 q = s / 32768;
    if (s % 32768 != 0 && s < 0) --q;
    return int16_t(q < -32768 ? -32768 : (q > 32767 ? 32767 : q));
}

// gsc_mix_model into the middle of three values: the neighbours stay as they are
bool run(const std::vector<int16_t>& x, const std::vector<long long>& g, int16_t* y) {
    int16_t out[3] = {0x5555, 0x5555, 0x5555};
    const int rc = gsc_mix_model(x.data(), g.data(), int(x.size()), out + 1);
    *y = out[1];
    return rc == 0 && out[0] == 0x5555 && out[2] == 0x5555;
}

void check_single_terms() {
    for (int v = -32768; v <= 32767; ++v) {
        int16_t y = 0;
        CHECK(run({int16_t(v)}, {32768}, &y) && y == v, "unity: %d -> %d", v, y);
        const int want = v == -32768 ? 32767 : -v;
        CHECK(run({int16_t(v)}, {-32768}, &y) && y == want, "inversion: %d -> %d", v, y);
        CHECK(run({int16_t(v)}, {0}, &y) && y == 0, "gain 0: %d -> %d", v, y);
        for (long long g : {16384LL, -16384LL, 1LL, -1LL, 8192LL, 1LL << 20, -(1LL << 20), 32767LL, 49152LL}) {
            CHECK(run({int16_t(v)}, {g}, &y) && y == model({int16_t(v)}, {g}), "gain %lld: %d -> %d", g, v, y);
        }
    }
    int16_t y = 0;
    CHECK(run({1}, {16384}, &y) && y == 1, "half of 1 rounds up, got %d", y);
    CHECK(run({-1}, {16384}, &y) && y == 0, "half of -1 rounds up, got %d", y);
    std::printf("unity, inversion, halves and nine gains over every int16: ok\n");
}

void check_sums() {
    int16_t y = 0;
    CHECK(run({32767, 32767}, {32768, 32768}, &y) && y == 32767, "two upper rails: %d", y);
    CHECK(run({-32768, -32768}, {32768, 32768}, &y) && y == -32768, "two lower rails: %d", y);
    CHECK(run({32767, -32768}, {32768, 32768}, &y) && y == -1, "both rails: %d", y);
    CHECK(run({1234, 1234}, {777, -777}, &y) && y == 0, "+g and -g: %d", y);
    // the extremes: 256 terms of either rail at either end of the gain range
    const long long G = gsc::kMixMaxGain;
    for (int16_t rail : {int16_t(32767), int16_t(-32768)}) {
        for (long long g : {G, -G}) {
            const std::vector<int16_t> x(gsc::kMixMaxSources, rail);
            const std::vector<long long> gg(gsc::kMixMaxSources, g);
            const int want = (rail > 0) == (g > 0) ? 32767 : -32768;
            CHECK(run(x, gg, &y) && y == want && y == model(x, gg), "256 x %d x %lld -> %d", rail, g, y);
        }
    }
    // ... and cancelling to a small value from the largest partial sums
    {
        std::vector<int16_t> x(gsc::kMixMaxSources, 32767);
        std::vector<long long> gg(gsc::kMixMaxSources, G);
        for (size_t i = 1; i < x.size(); i += 2) gg[i] = -G;
        gg.back() = -G + 3;
        CHECK(run(x, gg, &y) && y == model(x, gg), "cancelling extremes -> %d, model %d", y, model(x, gg));
    }
    std::mt19937_64 rng(20240607);
    for (int it = 0; it < 200000; ++it) {
        const int n = 1 + int(rng() % (it % 16 == 0 ? gsc::kMixMaxSources : 6));
        std::vector<int16_t> x(static_cast<size_t>(n));
        std::vector<long long> gg(static_cast<size_t>(n));
        const int wide = it % 3;
        for (int i = 0; i < n; ++i) {
            x[size_t(i)] = int16_t(rng() % 65536);
            const long long span = wide == 0 ? G : (wide == 1 ? 65536 : 40000);
            gg[size_t(i)] = (long long)(rng() % (2 * span + 1)) - span;
        }
        CHECK(run(x, gg, &y) && y == model(x, gg), "random case %d (%d terms): %d, model %d", it, n, y, model(x, gg));
    }
    std::printf("rails, extremes of 256 terms and 200000 random sums against 128 bits: ok\n");
}

void check_pieces() {
    CHECK(gsc::mix_gain_ok(gsc::kMixMaxGain) && gsc::mix_gain_ok(-gsc::kMixMaxGain) && gsc::mix_gain_ok(0), "range");
    CHECK(!gsc::mix_gain_ok(gsc::kMixMaxGain + 1) && !gsc::mix_gain_ok(-gsc::kMixMaxGain - 1), "range + 1");
    CHECK(!gsc::mix_gain_ok(INT64_MAX) && !gsc::mix_gain_ok(INT64_MIN), "range at the ends of int64");
    CHECK(gsc::mix_round(INT64_MAX - 16384) == 32767 && gsc::mix_round(INT64_MIN) == -32768, "round at the ends");
    // a tile's accumulators fit kMixAccElems for every channel count, and a tile is never empty
    for (int ch = 1; ch <= 255; ++ch) {
        for (int cap : {512, 4096}) {
            const int t = gsc::mix_tile_len(ch, cap);
            CHECK(t >= 1 && t <= cap && t * ch <= gsc::kMixAccElems, "tile of %d channels: %d", ch, t);
            CHECK(t == cap || (t + 1) * ch > gsc::kMixAccElems, "tile of %d channels is not the largest: %d", ch, t);
        }
    }
    std::printf("gain range, rounding at the ends of int64 and the tile rule: ok\n");
}

void check_refusals() {
    const int16_t x[2] = {5, 6};
    const long long g[2] = {32768, 32768};
    const long long over[2] = {32768, gsc::kMixMaxGain + 1}, under[2] = {-gsc::kMixMaxGain - 1, 0};
    int16_t y = 0x5555;
    CHECK(gsc_mix_model(nullptr, g, 2, &y) == -1 && gsc_mix_model(x, nullptr, 2, &y) == -1, "null inputs");
    CHECK(gsc_mix_model(x, g, 2, nullptr) == -1, "null output");
    CHECK(gsc_mix_model(x, g, 0, &y) == -1 && gsc_mix_model(x, g, -1, &y) == -1, "n < 1");
    CHECK(gsc_mix_model(x, g, gsc::kMixMaxSources + 1, &y) == -1, "n = 257 (nothing is read)");
    CHECK(gsc_mix_model(x, over, 2, &y) == -1 && gsc_mix_model(x, under, 2, &y) == -1, "gain out of range");
    CHECK(y == 0x5555, "a refused call wrote %d", y);
    std::printf("refusals: ok\n");
}

}  // namespace

int main() {
    check_single_terms();
    check_sums();
    check_pieces();
    check_refusals();
    if (g_bad) std::printf("%d check(s) failed\n", g_bad);
    return g_bad ? 1 : 0;
}
