// Stand-alone driver of the crop planner the bound kernels run
// (gsc_crop_plan.h: gsc::crop_plan_one, which compiles for the host and the
// device alike) against the host planners of the other crop calls
// (gsc::plan_crops, gsc::plan_crops_fmt), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc bound_check
//   soundchunks_amd/lib/decode_bound_check FILE.gsc...
// For every file, at its own rate (against both host planners), at 44100 Hz
// and at 16000 Hz: edge crops of the stream and of every frame and random
// crops, every field compared (clipped count, source range, frame span, and
// that a crop which writes nothing reads nothing); the six kinds of bad crop,
// each told from the others; and crops that start and end at the first sample
// of every run of frames that start at the same sample, whose frame must be
// the last of the run.  Then the same over a made-up frame table with runs at
// its start, in its middle and at its end, with nothing but first samples.
// One line per file; exit status 0 when nothing failed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_crop_plan.h"
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

// the shared planner over a host index, as the kernels run it over a BoundStream
int shared_plan(const gsc::Index& ix, const gsc::ResampleShape& sh, const gsc::Crop& c, int64_t length,
                gsc::CropSpan* sp) {
    const int st = gsc::crop_stream_status(c.stream, 1);
    if (st != gsc::kCropGood) {
        *sp = gsc::CropSpan{0, 0, 0, 0, 0};
        return st;
    }
    return gsc::crop_plan_one(c.begin, c.count, length, ix.samples, int32_t(ix.frames.size()), sh.phases, sh.step,
                              sh.half_taps, [&](int32_t i) { return ix.frames[size_t(i)].first_sample; }, sp);
}

// rate 0: plan_crops; otherwise plan_crops_fmt at that rate
void compare(const gsc::Index& ix, int rate, const std::vector<gsc::Crop>& crops, int64_t length) {
    const gsc::Index* ixs[1] = {&ix};
    gsc::CropPlan plan;
    std::string err;
    const int rc = rate == 0
                       ? gsc::plan_crops(ixs, 1, crops.data(), int(crops.size()), length, &plan, &err)
                       : gsc::plan_crops_fmt(ixs, 1, crops.data(), int(crops.size()), length, rate, 0, &plan, &err);
    CHECK(rc == 0 && plan.crops.size() == crops.size(), "-> %d: host plan refused: %s", rate, err.c_str());
    gsc::ResampleShape sh;
    if (rate != 0 && rate != ix.rate && ix.samples > 0)
        CHECK(gsc::resample_shape(ix.rate, rate, &sh, &err) == 0, "-> %d: %s", rate, err.c_str());
    for (size_t i = 0; i < crops.size(); ++i) {
        const gsc::PlanCrop& pc = plan.crops[i];
        gsc::CropSpan sp;
        CHECK(shared_plan(ix, sh, crops[i], length, &sp) == gsc::kCropGood, "-> %d crop %zu: good crop called bad", rate,
              i);
        CHECK(sp.count == pc.count && sp.f0 == pc.f0 && sp.f1 == pc.f1,
              "-> %d crop %zu (%lld, %lld): count %lld frames [%d, %d), host %lld [%d, %d)", rate, i,
              (long long)crops[i].begin, (long long)crops[i].count, (long long)sp.count, sp.f0, sp.f1,
              (long long)pc.count, pc.f0, pc.f1);
        if (rate != 0) {
            CHECK(sp.src_begin == pc.src_begin && sp.src_end == pc.src_end && sh.phases == pc.rate_up &&
                      sh.step == pc.rate_down && sh.half_taps == pc.half_taps,
                  "-> %d crop %zu: source [%lld, %lld), host [%lld, %lld)", rate, i, (long long)sp.src_begin,
                  (long long)sp.src_end, (long long)pc.src_begin, (long long)pc.src_end);
        } else if (sp.count > 0) {
            CHECK(sp.src_begin == pc.begin && sp.src_end == pc.begin + pc.count, "crop %zu: native source range", i);
        }
        if (sp.count == 0)
            CHECK(sp.f0 == 0 && sp.f1 == 0 && sp.src_begin == 0 && sp.src_end == 0, "-> %d crop %zu: an empty crop reads",
                  rate, i);
        else
            CHECK(sp.f0 >= 0 && sp.f0 < sp.f1 && size_t(sp.f1) <= ix.frames.size(), "-> %d crop %zu: span", rate, i);
    }
}

void check_bad(const gsc::Index& ix, const gsc::ResampleShape& sh, int64_t length) {
    const int64_t n = ix.samples;
    const struct {
        gsc::Crop c;
        int want;
        const char* what;
    } bad[] = {{{-1, 0, 1}, gsc::kCropBadStream, "stream -1"},      {{1, 0, 1}, gsc::kCropBadStream, "stream 1 of 1"},
               {{0, -1, 1}, gsc::kCropBadBegin, "begin -1"},         {{0, n + 1, 0}, gsc::kCropBadBegin, "begin samples + 1"},
               {{0, 0, -1}, gsc::kCropBadCount, "count -1"},         {{0, 0, length + 1}, gsc::kCropBadCount, "count length + 1"},
               {{0, int64_t(1) << 62, 1}, gsc::kCropBadBegin, "begin 2^62"},
               {{0, -(int64_t(1) << 62), 1}, gsc::kCropBadBegin, "begin -2^62"},
               {{0, 0, int64_t(1) << 62}, gsc::kCropBadCount, "count 2^62"}};
    for (const auto& b : bad) {
        gsc::CropSpan sp;
        const int st = shared_plan(ix, sh, b.c, length, &sp);
        CHECK(st == b.want, "%s: status %d, want %d", b.what, st, b.want);
        CHECK(sp.count == 0 && sp.f0 == 0 && sp.f1 == 0 && sp.src_begin == 0 && sp.src_end == 0, "%s: a bad crop reads",
              b.what);
    }
    // the edges themselves are good
    for (const gsc::Crop& c : {gsc::Crop{0, 0, 0}, gsc::Crop{0, n, 0}, gsc::Crop{0, n, length}, gsc::Crop{0, 0, length}}) {
        gsc::CropSpan sp;
        CHECK(shared_plan(ix, sh, c, length, &sp) == gsc::kCropGood, "an edge crop called bad");
    }
}

// Runs of frames that start at the same sample: a crop that starts (ends) at
// that sample starts (ends) in the run's last frame.  firsts has nframes + 1
// entries, the last one the stream's samples.
void check_runs(const std::vector<int64_t>& firsts, int* runs_seen) {
    const int32_t nf = int32_t(firsts.size()) - 1;
    const int64_t samples = firsts[size_t(nf)];
    auto first = [&](int32_t i) { return firsts[size_t(i)]; };
    for (int32_t a = 0; a < nf;) {
        int32_t b = a;
        while (b + 1 < nf && firsts[size_t(b + 1)] == firsts[size_t(a)]) ++b;
        // [a, b] start at the same sample; b holds it when it holds anything
        const int64_t s = firsts[size_t(a)];
        if (b > a) ++*runs_seen;
        if (s < samples && firsts[size_t(b + 1)] > s) {
            CHECK(gsc::crop_frame_at(nf, s, first) == b, "sample %lld: frame %d, want %d", (long long)s,
                  gsc::crop_frame_at(nf, s, first), b);
            gsc::CropSpan sp;
            CHECK(gsc::crop_plan_one(s, 1, 8, samples, nf, 1, 1, 0, first, &sp) == gsc::kCropGood && sp.f0 == b &&
                      sp.f1 == b + 1,
                  "a crop of sample %lld: frames [%d, %d), want [%d, %d)", (long long)s, sp.f0, sp.f1, b, b + 1);
            if (s > 0) {  // ending just before the run: the frame before it
                CHECK(gsc::crop_plan_one(s - 1, 2, 8, samples, nf, 1, 1, 0, first, &sp) == gsc::kCropGood && sp.f1 == b + 1 &&
                          sp.f0 < a,
                      "a crop across sample %lld: frames [%d, %d)", (long long)s, sp.f0, sp.f1);
            }
        }
        a = b + 1;
    }
}

}  // namespace

int main(int argc, char** argv) {
    std::mt19937_64 rng(20250920);
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
        gsc::Index ix;
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
                for (int64_t c : {int64_t(1), int64_t(2), int64_t(3), length}) {
                    const int64_t b = f.first_sample + d;
                    if (b >= 0 && b <= n) crops.push_back({0, b, c});
                }
        for (int i = 0; i < 64 && n > 0; ++i)
            crops.push_back({0, int64_t(rng() % uint64_t(n + 1)), int64_t(rng() % uint64_t(length + 1))});
        for (int rate : {0, ix.rate, 44100, 16000}) {
            compare(ix, rate, crops, length);
            gsc::ResampleShape sh;
            if (rate != 0 && rate != ix.rate && n > 0 && gsc::resample_shape(ix.rate, rate, &sh, &err) != 0) {
                std::printf("FAIL %s -> %d: %s\n", argv[a], rate, err.c_str());
                ++g_bad;
                continue;
            }
            check_bad(ix, sh, length);
        }
        std::vector<int64_t> firsts;
        for (const auto& f : ix.frames) firsts.push_back(f.first_sample);
        firsts.push_back(n);
        int runs = 0;
        if (!ix.frames.empty()) check_runs(firsts, &runs);
        std::printf("%s: %zu frames, %lld samples at %d Hz: %zu crops x 4 plans, %d runs of equal first samples%s\n",
                    argv[a], ix.frames.size(), (long long)n, ix.rate, crops.size(), runs,
                    g_bad == bad_before ? "" : " FAILED");
    }
    // a frame table of nothing but first samples: runs of three at the start, of two and four in the
    // middle, of three at the end (the last two frames empty)
    {
        const std::vector<int64_t> firsts{0, 0, 0, 40, 90, 90, 130, 130, 130, 130, 200, 260, 260, 260, 260};
        int runs = 0;
        const int bad_before = g_bad;
        check_runs(firsts, &runs);
        const int32_t nf = int32_t(firsts.size()) - 1;
        auto first = [&](int32_t i) { return firsts[size_t(i)]; };
        // every sample against a linear search for the last frame that starts at or before it
        for (int64_t s = 0; s < firsts.back(); ++s) {
            int32_t want = 0;
            for (int32_t i = 0; i < nf; ++i)
                if (firsts[size_t(i)] <= s) want = i;
            if (gsc::crop_frame_at(nf, s, first) != want) {
                std::printf("FAIL made-up table: sample %lld: frame %d, want %d\n", (long long)s,
                            gsc::crop_frame_at(nf, s, first), want);
                ++g_bad;
            }
        }
        // the run at the end holds nothing: a crop up to the last sample ends in frame 10
        gsc::CropSpan sp;
        if (gsc::crop_plan_one(0, 260, 260, 260, nf, 1, 1, 0, first, &sp) != gsc::kCropGood || sp.f0 != 2 || sp.f1 != 11) {
            std::printf("FAIL made-up table: the whole stream spans [%d, %d)\n", sp.f0, sp.f1);
            ++g_bad;
        }
        std::printf("made-up table: %d frames, %d runs%s\n", nf, runs, g_bad == bad_before ? "" : " FAILED");
    }
    std::printf("bound_check: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
