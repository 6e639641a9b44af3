// Stand-alone driver of the resampler's host side (gsc_resample.cpp, no HIP:
// gsc::resample_shape, resample_table, and plan_crops, which the crop calls
// run before they launch anything), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc resample_check
//   soundchunks_amd/lib/decode_resample_check FILE.gsc...
// Tables of six pairs of rates: shape, every row summing to 2^24, phase L - p
// the mirror of phase p within the remainder's bound, and the cache returning
// the same pointer.  For every file and each of four output rates: edge and
// random crops through the planner, checking the clipped count against the
// formula and that the source range is the filter's reach clipped to the
// stream, non-empty exactly when the crop writes something, and covered by
// [f0, f1).  Then the refusals.  One line per file; exit status 0 when nothing failed.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_decode.h"

namespace {

int g_bad = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++g_bad;                      \
            return;                       \
        }                                 \
    } while (0)

void check_table(int fi, int fo, int phases, int taps) {
    gsc::ResampleShape sh;
    std::string err;
    const int32_t* t = gsc::resample_table(fi, fo, &sh, &err);
    CHECK(t != nullptr, "%d -> %d refused: %s", fi, fo, err.c_str());
    CHECK(sh.phases == phases && sh.taps() == taps, "%d -> %d: %d phases x %d taps", fi, fo, sh.phases, sh.taps());
    CHECK(gsc::resample_table(fi, fo, nullptr, nullptr) == t, "%d -> %d: the cache built a second table", fi, fo);
    for (int p = 0; p < phases; ++p) {
        int64_t sum = 0;
        for (int j = 0; j < taps; ++j) sum += t[size_t(p) * taps + j];
        CHECK(sum == (int64_t(1) << gsc::kResampleShift), "%d -> %d: phase %d sums to %lld", fi, fo, p, (long long)sum);
        if (p == 0) continue;
        for (int j = 0; j < taps; ++j) {
            const int64_t d = int64_t(t[size_t(p) * taps + j]) - t[size_t(phases - p) * taps + (taps - 1 - j)];
            CHECK(std::llabs(d) <= taps / 2 + 1, "%d -> %d: phase %d tap %d is not phase %d's mirror", fi, fo, p, j,
                  phases - p);
        }
    }
}

void must_refuse_pair(int fi, int fo) {
    std::string err;
    CHECK(gsc::resample_table(fi, fo, nullptr, &err) == nullptr, "%d -> %d accepted", fi, fo);
    CHECK(err.find(std::to_string(fi)) != std::string::npos && err.find(std::to_string(fo)) != std::string::npos,
          "%d -> %d: the message names no rates: %s", fi, fo, err.c_str());
}

void check_plan(const gsc::Index& ix, int out_rate, const std::vector<gsc::Crop>& crops, int64_t length) {
    const gsc::Index* ixs[1] = {&ix};
    gsc::CropPlan plan;
    std::string err;
    const int rc = gsc::plan_crops(ixs, 1, crops.data(), int(crops.size()), length, out_rate, 0, &plan, &err);
    CHECK(rc == 0, "-> %d: plan refused: %s", out_rate, err.c_str());
    CHECK(plan.crops.size() == crops.size() && plan.channels == ix.channels, "plan shape");
    const int g = std::gcd(ix.rate, out_rate);
    const int64_t L = out_rate / g, M = ix.rate / g, n = ix.samples;
    for (size_t ci = 0; ci < crops.size(); ++ci) {
        const gsc::PlanCrop& pc = plan.crops[ci];
        const int64_t b = crops[ci].begin;
        // the first output whose position reaches the stream's end, by counting
        int64_t lim = (n - b) * L / M;
        while (lim > 0 && (b * L + (lim - 1) * M) / L >= n) --lim;
        while ((b * L + lim * M) / L < n) ++lim;
        const int64_t want = std::min<int64_t>(crops[ci].count, lim);
        CHECK(pc.begin == b && pc.count == want, "-> %d crop %zu: count %lld, want %lld", out_rate, ci,
              (long long)pc.count, (long long)want);
        CHECK(pc.rate_up == L && pc.rate_down == M, "-> %d crop %zu: ratio", out_rate, ci);
        if (L == M) CHECK(pc.half_taps == 0, "-> %d crop %zu: a filter at the stream's own rate", out_rate, ci);
        if (pc.count == 0) {
            CHECK(pc.f0 == pc.f1 && pc.src_begin == pc.src_end, "-> %d crop %zu: an empty crop reads", out_rate, ci);
            continue;
        }
        const int64_t T = pc.half_taps, last = (b * L + (pc.count - 1) * M) / L;
        CHECK(last < n, "-> %d crop %zu: last output at %lld of %lld", out_rate, ci, (long long)last, (long long)n);
        CHECK(pc.src_begin == std::max<int64_t>(b - (T > 0 ? T - 1 : 0), 0) &&
                  pc.src_end == std::min<int64_t>(last + T + 1, n) && pc.src_begin < pc.src_end,
              "-> %d crop %zu: source range [%lld, %lld)", out_rate, ci, (long long)pc.src_begin, (long long)pc.src_end);
        CHECK(pc.f0 >= 0 && pc.f0 < pc.f1 && size_t(pc.f1) <= ix.frames.size(), "-> %d crop %zu: span", out_rate, ci);
        const gsc::IndexFrame &fa = ix.frames[size_t(pc.f0)], &fb = ix.frames[size_t(pc.f1 - 1)];
        CHECK(fa.first_sample <= pc.src_begin && pc.src_end <= fb.first_sample + int64_t(fb.flen) * fb.cs,
              "-> %d crop %zu: frames [%d, %d) do not cover the source range", out_rate, ci, pc.f0, pc.f1);
    }
}

void must_refuse(const std::vector<const gsc::Index*>& ixs, gsc::Crop c, int64_t length, int rate, int channels,
                 const char* what) {
    gsc::CropPlan plan;
    std::string err;
    const int rc = gsc::plan_crops(ixs.data(), int(ixs.size()), &c, 1, length, rate, channels, &plan, &err);
    CHECK(rc != 0 && !err.empty(), "%s accepted", what);
}

}  // namespace

int main(int argc, char** argv) {
    check_table(44100, 48000, 160, 32);
    check_table(48000, 44100, 147, 36);
    check_table(26390, 44100, 630, 32);
    check_table(32000, 8000, 1, 128);
    check_table(8000, 32000, 4, 32);
    check_table(44100, 22050, 1, 64);
    check_table(32000, 2000, 1, 512);
    must_refuse_pair(44101, 192000);
    must_refuse_pair(48000, 2000);
    must_refuse_pair(0, 44100);
    must_refuse_pair(44100, -1);
    std::printf("tables: %s\n", g_bad ? "FAILED" : "ok");

    std::vector<gsc::Index> all(size_t(argc > 1 ? argc - 1 : 0));
    std::mt19937_64 rng(20240611);
    for (int a = 1; a < argc; ++a) {
        std::FILE* fp = std::fopen(argv[a], "rb");
        if (!fp) {
            std::printf("%s: cannot open\n", argv[a]);
            ++g_bad;
            continue;
        }
        std::vector<uint8_t> g;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, fp)) > 0;) g.insert(g.end(), buf, buf + n);
        std::fclose(fp);
        gsc::Index& ix = all[size_t(a - 1)];
        std::string err;
        if (gsc::decode_walk(g.data(), g.size(), &ix, &err) != 0) {
            std::printf("%s: refused: %s\n", argv[a], err.c_str());
            ++g_bad;
            continue;
        }
        const int bad_before = g_bad;
        const int64_t n = ix.samples, length = 6000;
        std::vector<gsc::Crop> crops{{0, 0, 0}, {0, n, 0}, {0, n, length}, {0, 0, length}, {0, 0, 1},
                                     {0, std::max<int64_t>(n - 1, 0), length}, {0, std::max<int64_t>(n - 1, 0), 1}};
        for (const auto& f : ix.frames)
            for (int64_t d = -2; d <= 1; ++d)
                for (int64_t c : {int64_t(1), int64_t(2), length}) {
                    const int64_t b = f.first_sample + d;
                    if (b >= 0 && b <= n) crops.push_back({0, b, c});
                }
        for (int i = 0; i < 64 && n > 0; ++i)
            crops.push_back({0, int64_t(rng() % uint64_t(n + 1)), int64_t(rng() % uint64_t(length + 1))});
        const int rates[] = {ix.rate, 48000, 44100, 16000, ix.rate / 16 + 1};
        for (int r : rates) check_plan(ix, r, crops, length);
        std::vector<const gsc::Index*> ixs{&ix};
        must_refuse(ixs, {0, -1, 1}, length, 48000, 0, "begin -1");
        must_refuse(ixs, {0, n + 1, 0}, length, 48000, 0, "begin samples + 1");
        must_refuse(ixs, {0, 0, length + 1}, length, 48000, 0, "count length + 1");
        must_refuse(ixs, {1, 0, 1}, length, 48000, 0, "stream index 1 of 1");
        must_refuse(ixs, {0, 0, 1}, length, -1, 0, "rate -1");
        must_refuse(ixs, {0, 0, 1}, length, 48000, -1, "channels -1");
        if (n > 0) must_refuse(ixs, {0, 0, 1}, length, ix.rate / 17, 0, "a seventeenth of the rate");
        if (ix.channels > 1) must_refuse(ixs, {0, 0, 1}, length, 0, ix.channels + 1, "one channel more");
        std::printf("%s: %zu frames, %lld samples at %d Hz: %zu crops x 5 rates planned%s\n", argv[a], ix.frames.size(),
                    (long long)n, ix.rate, crops.size(), g_bad == bad_before ? "" : " FAILED");
    }
    // neighbours as the streams of one call: different channel counts need out_channels 1, or a mono stream
    for (size_t i = 0; i + 1 < all.size(); ++i) {
        if (all[i].frames.empty() || all[i + 1].frames.empty()) continue;
        std::vector<const gsc::Index*> ixs{&all[i], &all[i + 1]};
        const int ca = all[i].channels, cb = all[i + 1].channels;
        gsc::CropPlan plan;
        std::string err;
        gsc::Crop c{1, 0, 1};
        if (gsc::plan_crops(ixs.data(), 2, &c, 1, 16, 44100, 1, &plan, &err) != 0 || plan.channels != 1) {
            std::printf("FAIL: a mono output of %d and %d channels refused: %s\n", ca, cb, err.c_str());
            ++g_bad;
        }
        if (ca != cb) must_refuse(ixs, c, 16, 44100, 0, "streams of different channel counts, no out_channels");
        if (ca != cb && ca != 1 && cb != 1) must_refuse(ixs, c, 16, 44100, ca, "channels that do not map");
    }
    std::printf("resample_check: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
