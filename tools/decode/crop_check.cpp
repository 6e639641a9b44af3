// Stand-alone driver of the decoder's sample locator and crop planning, none
// of which needs HIP: gsc::index_locate (gsc_decode_index.cpp), which
// gsc_index_locate wraps; gsc::plan_crops (gsc_resample.cpp), which
// gsc_decode_crops and gsc_decode_crops_fmt run before they launch anything;
// and gsc::crop_plan_one (gsc_crop_plan.h), which plan_crops calls per crop and
// the kernels of a bound call run themselves.  Meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc crop_check
//   soundchunks_amd/lib/decode_crop_check FILE.gsc...
// For every file: locate at every frame edge +-1 and at random positions
// against a linear search.  Then, at the stream's own rate (rate 0 and the rate
// itself), at 44100 Hz and at 16000 Hz, edge crops of the stream and of every
// frame and random crops through plan_crops, every field compared with a model
// written here, which does not call the planner's code: a linear search over
// first samples and the closed formulas min(count, ceil((samples - begin) L /
// M)) and [begin - (T - 1), last + T + 1) clipped to the stream.  Checked too:
//   - a crop that writes nothing reads nothing (all spans 0),
//   - every sample of a crop's source range (its ends, the frame edges inside
//     it, random ones) lies in a frame of the crop's span,
//   - every frame of a span has its checkpoints, bits and tables inside the slabs,
//   - the six kinds of bad crop, each told from the others by crop_plan_one and
//     refused with the matching words by plan_crops,
//   - crops that start and end at the first sample of a run of frames that
//     start at the same sample: their frame is the last of the run.
// Then the runs again over a made-up frame table with runs at its start, in its
// middle and at its end, and all files pairwise as the streams of one call.
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

void check_locate(const gsc::Index& ix, int64_t s) {
    int fr = -1, within = -1;
    int64_t row = -1, cp = -1;
    std::string err;
    const int rc = gsc::index_locate(ix, s, &fr, &row, &within, &cp, &err);
    if (s < 0 || s >= ix.samples) {
        CHECK(rc != 0 && !err.empty(), "sample %lld accepted", (long long)s);
        return;
    }
    CHECK(rc == 0, "sample %lld refused: %s", (long long)s, err.c_str());
    int want = -1;
    for (size_t i = 0; i < ix.frames.size(); ++i) {
        const gsc::IndexFrame& f = ix.frames[i];
        if (s >= f.first_sample && s < f.first_sample + int64_t(f.flen) * f.cs) want = int(i);
    }
    CHECK(fr == want, "sample %lld: frame %d, want %d", (long long)s, fr, want);
    const gsc::IndexFrame& f = ix.frames[size_t(fr)];
    CHECK(row == (s - f.first_sample) / f.cs && within == int((s - f.first_sample) % f.cs), "sample %lld: row",
          (long long)s);
    CHECK(cp == int64_t(f.cp_first) + row * f.ch / gsc::kDecodeS, "sample %lld: checkpoint", (long long)s);
    CHECK(cp >= int64_t(f.cp_first) && cp < int64_t(f.cp_first + f.cp_count) && size_t(cp) < ix.cps.size(),
          "sample %lld: checkpoint %lld outside the frame's", (long long)s, (long long)cp);
}

// ---- the model: nothing of gsc_crop_plan.h ----------------------------------
struct Model {
    int status;  // 0 good, 1 stream, 2 begin, 3 count
    int64_t count, src_begin, src_end;
    int f0, f1;
};

// the last frame that starts at or before s; firsts has nframes + 1 entries, the last one the stream's samples
int model_frame(const std::vector<int64_t>& firsts, int64_t s) {
    int want = 0;
    for (size_t i = 0; i + 1 < firsts.size(); ++i)
        if (firsts[i] <= s) want = int(i);
    return want;
}

// L / M the resampler's ratio, T its taps per side (1, 1, 0: none)
Model model_plan(const std::vector<int64_t>& firsts, int nstreams, const gsc::Crop& c, int64_t length, int64_t L,
                 int64_t M, int64_t T) {
    using wide = __int128;
    const int64_t samples = firsts.back();
    Model m{0, 0, 0, 0, 0, 0};
    if (c.stream < 0 || c.stream >= nstreams) m.status = 1;
    else if (c.begin < 0 || c.begin > samples) m.status = 2;
    else if (c.count < 0 || c.count > length) m.status = 3;
    if (m.status != 0 || firsts.size() < 2) return m;
    const wide avail = (wide(samples - c.begin) * L + M - 1) / M;
    m.count = avail < wide(c.count) ? int64_t(avail) : c.count;
    if (m.count == 0) return m;
    const int64_t last = int64_t((wide(c.begin) * L + wide(m.count - 1) * M) / L);
    m.src_begin = std::max<int64_t>(c.begin - (T > 0 ? T - 1 : 0), 0);
    m.src_end = std::min<int64_t>(last + T + 1, samples);
    m.f0 = model_frame(firsts, m.src_begin);
    m.f1 = model_frame(firsts, m.src_end - 1) + 1;
    return m;
}

std::vector<int64_t> first_samples(const gsc::Index& ix) {
    std::vector<int64_t> firsts;
    for (const auto& f : ix.frames) firsts.push_back(f.first_sample);
    firsts.push_back(ix.samples);
    return firsts;
}

// what the kernels read of frame fi lies inside the index's arrays and the file
void check_frame(const gsc::Index& ix, int fi) {
    const gsc::IndexFrame& f = ix.frames[size_t(fi)];
    const int64_t S = gsc::kDecodeS;
    CHECK(int64_t(f.cp_count) == (f.nsym + S - 1) / S && f.cp_first + f.cp_count <= ix.cps.size(),
          "frame %d: %zu checkpoints for %lld symbols", fi, f.cp_count, (long long)f.nsym);
    for (size_t s = 0; s < f.cp_count; ++s) {
        const uint64_t cpv = ix.cps[f.cp_first + s];
        CHECK(f.bs_off + (cpv >> 3) / 8 < ix.len && (cpv >> 3) <= f.nbits && (cpv & 7) <= 4, "frame %d: checkpoint %zu",
              fi, s);
    }
    CHECK(f.cb_first + size_t(f.count) * size_t(f.cs) <= ix.codebook.size() &&
              f.att_first + size_t(f.count) <= ix.att.size(),
          "frame %d: tables past their slabs", fi);
}

// one planned crop against the model, and its source samples against index_locate
void check_crop(const gsc::Index& ix, const gsc::PlanCrop& pc, const Model& m, const gsc::ResampleShape& sh, int rate,
                size_t ci, std::mt19937_64& rng) {
    CHECK(m.status == 0, "-> %d crop %zu: the model calls a planned crop bad", rate, ci);
    CHECK(pc.count == m.count && pc.f0 == m.f0 && pc.f1 == m.f1 && pc.src_begin == m.src_begin &&
              pc.src_end == m.src_end,
          "-> %d crop %zu (begin %lld): count %lld source [%lld, %lld) frames [%d, %d), model %lld [%lld, %lld) [%d, %d)",
          rate, ci, (long long)pc.begin, (long long)pc.count, (long long)pc.src_begin, (long long)pc.src_end, pc.f0,
          pc.f1, (long long)m.count, (long long)m.src_begin, (long long)m.src_end, m.f0, m.f1);
    CHECK(pc.rate_up == sh.phases && pc.rate_down == sh.step && pc.half_taps == sh.half_taps, "-> %d crop %zu: resampler",
          rate, ci);
    if (pc.count == 0) {
        CHECK(pc.f0 == 0 && pc.f1 == 0 && pc.src_begin == 0 && pc.src_end == 0, "-> %d crop %zu: an empty crop reads",
              rate, ci);
        return;
    }
    CHECK(pc.f0 >= 0 && pc.f0 < pc.f1 && size_t(pc.f1) <= ix.frames.size(), "-> %d crop %zu: span", rate, ci);
    if (sh.half_taps == 0)
        CHECK(pc.src_begin == pc.begin && pc.src_end == pc.begin + pc.count, "-> %d crop %zu: native source range", rate,
              ci);
    for (int fi = pc.f0; fi < pc.f1; ++fi) check_frame(ix, fi);
    std::vector<int64_t> ss{pc.src_begin, pc.src_end - 1, (pc.src_begin + pc.src_end) / 2};
    for (int fi = pc.f0; fi < pc.f1; ++fi)
        for (int64_t d = -1; d <= 1; ++d) {
            const int64_t s = ix.frames[size_t(fi)].first_sample + d;
            if (s >= pc.src_begin && s < pc.src_end) ss.push_back(s);
        }
    for (int i = 0; i < 16; ++i) ss.push_back(pc.src_begin + int64_t(rng() % uint64_t(pc.src_end - pc.src_begin)));
    for (int64_t s : ss) {
        int fr = -1;
        std::string err;
        CHECK(gsc::index_locate(ix, s, &fr, nullptr, nullptr, nullptr, &err) == 0 && fr >= pc.f0 && fr < pc.f1,
              "-> %d crop %zu: sample %lld in frame %d outside [%d, %d) %s", rate, ci, (long long)s, fr, pc.f0, pc.f1,
              err.c_str());
    }
}

// the resampler of stream ix for out_rate, as plan_crops chooses it
bool shape_of(const gsc::Index& ix, int rate, gsc::ResampleShape* sh) {
    *sh = gsc::ResampleShape();
    std::string err;
    if (rate == 0 || rate == ix.rate || ix.samples <= 0 || gsc::resample_shape(ix.rate, rate, sh, &err) == 0) return true;
    std::printf("FAIL %d -> %d: %s\n", ix.rate, rate, err.c_str());
    ++g_bad;
    return false;
}

// a call of good crops: planned, every crop compared
void check_plan(const std::vector<const gsc::Index*>& ixs, int rate, const std::vector<gsc::Crop>& crops,
                int64_t length, std::mt19937_64& rng) {
    gsc::CropPlan plan;
    std::string err;
    const int rc =
        gsc::plan_crops(ixs.data(), int(ixs.size()), crops.data(), int(crops.size()), length, rate, 0, &plan, &err);
    CHECK(rc == 0, "-> %d: plan refused: %s", rate, err.c_str());
    CHECK(plan.crops.size() == crops.size() && plan.channels == ixs[0]->channels, "-> %d: plan shape", rate);
    for (size_t ci = 0; ci < crops.size(); ++ci) {
        const gsc::PlanCrop& pc = plan.crops[ci];
        CHECK(pc.stream == crops[ci].stream && pc.begin == crops[ci].begin && pc.count <= length, "-> %d crop %zu", rate,
              ci);
        const gsc::Index& ix = *ixs[size_t(pc.stream)];
        gsc::ResampleShape sh;
        if (!shape_of(ix, rate, &sh)) return;
        const Model m = model_plan(first_samples(ix), int(ixs.size()), crops[ci], length, sh.phases, sh.step, sh.half_taps);
        check_crop(ix, pc, m, sh, rate, ci, rng);
    }
}

// The kinds of bad crop: crop_stream_status / crop_plan_one name the kind and
// read nothing, plan_crops refuses the call that holds one and names the crop.
void check_bad(const gsc::Index& ix, int rate, int64_t length, int* refusals) {
    const int64_t n = ix.samples;
    const gsc::Index* ixs[1] = {&ix};
    gsc::ResampleShape sh;
    if (!shape_of(ix, rate, &sh)) return;
    const std::vector<int64_t> firsts = first_samples(ix);
    const struct {
        gsc::Crop c;
        int want;
        const char* what;
        const char* words;
    } bad[] = {{{-1, 0, 1}, gsc::kCropBadStream, "stream -1", "crop 1: stream index -1"},
               {{1, 0, 1}, gsc::kCropBadStream, "stream 1 of 1", "crop 1: stream index 1"},
               {{0, -1, 1}, gsc::kCropBadBegin, "begin -1", "crop 1: begin -1 outside [0, "},
               {{0, n + 1, 0}, gsc::kCropBadBegin, "begin samples + 1", "crop 1: begin "},
               {{0, 0, -1}, gsc::kCropBadCount, "count -1", "crop 1: count -1 outside [0, length "},
               {{0, 0, length + 1}, gsc::kCropBadCount, "count length + 1", "crop 1: count "},
               {{0, int64_t(1) << 62, 1}, gsc::kCropBadBegin, "begin 2^62", "crop 1: begin "},
               {{0, -(int64_t(1) << 62), 1}, gsc::kCropBadBegin, "begin -2^62", "crop 1: begin "},
               {{0, 0, int64_t(1) << 62}, gsc::kCropBadCount, "count 2^62", "crop 1: count "}};
    for (const auto& b : bad) {
        gsc::CropSpan sp{0, 0, 0, 0, 0};
        int st = gsc::crop_stream_status(b.c.stream, 1);
        if (st == gsc::kCropGood)
            st = gsc::crop_plan_one(b.c.begin, b.c.count, length, n, int32_t(ix.frames.size()), sh.phases, sh.step,
                                    sh.half_taps, [&](int32_t i) { return ix.frames[size_t(i)].first_sample; }, &sp);
        CHECK(st == b.want && st == model_plan(firsts, 1, b.c, length, sh.phases, sh.step, sh.half_taps).status,
              "-> %d %s: status %d, want %d", rate, b.what, st, b.want);
        CHECK(sp.count == 0 && sp.f0 == 0 && sp.f1 == 0 && sp.src_begin == 0 && sp.src_end == 0,
              "-> %d %s: a bad crop reads", rate, b.what);
        gsc::CropPlan plan;
        std::string err;
        const gsc::Crop crops[2] = {gsc::Crop{0, 0, 0}, b.c};
        CHECK(gsc::plan_crops(ixs, 1, crops, 2, length, rate, 0, &plan, &err) != 0 &&
                  err.find(b.words) != std::string::npos,
              "-> %d %s: accepted, or refused as \"%s\"", rate, b.what, err.c_str());
        ++*refusals;
    }
}

// Runs of frames that start at the same sample: a crop that starts (ends) at
// that sample starts (ends) in the run's last frame.
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
            CHECK(gsc::crop_frame_at(nf, s, first) == b && model_frame(firsts, s) == b, "sample %lld: frame %d, want %d",
                  (long long)s, gsc::crop_frame_at(nf, s, first), b);
            gsc::CropSpan sp;
            CHECK(gsc::crop_plan_one(s, 1, 8, samples, nf, 1, 1, 0, first, &sp) == gsc::kCropGood && sp.f0 == b &&
                      sp.f1 == b + 1,
                  "a crop of sample %lld: frames [%d, %d), want [%d, %d)", (long long)s, sp.f0, sp.f1, b, b + 1);
            if (s > 0) {  // ending just before the run: the frame before it
                CHECK(gsc::crop_plan_one(s - 1, 2, 8, samples, nf, 1, 1, 0, first, &sp) == gsc::kCropGood &&
                          sp.f1 == b + 1 && sp.f0 < a,
                      "a crop across sample %lld: frames [%d, %d)", (long long)s, sp.f0, sp.f1);
            }
        }
        a = b + 1;
    }
}

void must_refuse(const std::vector<const gsc::Index*>& ixs, gsc::Crop c, int64_t length, const char* what) {
    gsc::CropPlan plan;
    std::string err;
    CHECK(gsc::plan_crops(ixs.data(), int(ixs.size()), &c, 1, length, 0, 0, &plan, &err) != 0 && !err.empty(),
          "%s accepted", what);
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<gsc::Index> all(size_t(argc > 1 ? argc - 1 : 0));
    std::mt19937_64 rng(20240519);
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
        const int64_t n = ix.samples;
        std::vector<int64_t> pos{-1, 0, 1, n - 1, n, n + 1, -(int64_t(1) << 62), int64_t(1) << 62};
        for (const auto& f : ix.frames)
            for (int64_t d = -1; d <= 1; ++d) pos.push_back(f.first_sample + d);
        for (int i = 0; i < 200 && n > 0; ++i) pos.push_back(int64_t(rng() % uint64_t(n)));
        for (int64_t s : pos) check_locate(ix, s);

        // crops: edges of the stream and of every frame, zero and one sample, past the end, random
        std::vector<const gsc::Index*> ixs{&ix};
        const int64_t length = std::max<int64_t>(1, std::min<int64_t>(n, 50000));
        std::vector<gsc::Crop> crops{{0, 0, 0}, {0, n, 0}, {0, n, length}, {0, 0, std::min(n, length)}, {0, 0, length},
                                     {0, std::max<int64_t>(n - 1, 0), length}, {0, std::max<int64_t>(n - 1, 0), 1},
                                     {0, 0, 1}};
        for (const auto& f : ix.frames)
            for (int64_t d = -2; d <= 1; ++d)
                for (int64_t c : {int64_t(1), int64_t(2), int64_t(3), length}) {
                    const int64_t b = f.first_sample + d;
                    if (b >= 0 && b <= n) crops.push_back({0, b, c});
                }
        for (int i = 0; i < 64 && n > 0; ++i)
            crops.push_back({0, int64_t(rng() % uint64_t(n + 1)), int64_t(rng() % uint64_t(length + 1))});
        int refusals = 0, runs = 0;
        for (int rate : {0, ix.rate, 44100, 16000}) {
            check_plan(ixs, rate, crops, length, rng);
            check_plan(ixs, rate, {}, length, rng);
            check_bad(ix, rate, length, &refusals);
        }
        if (!ix.frames.empty()) check_runs(first_samples(ix), &runs);
        std::printf(
            "%s: %zu frames, %lld samples at %d Hz: %zu positions located, %zu crops compared per rate (0, %d, 44100, "
            "16000), %d refusals, %d runs of equal first samples%s\n",
            argv[a], ix.frames.size(), (long long)n, ix.rate, pos.size(), crops.size(), ix.rate, refusals, runs,
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
        // every sample against the linear search, and every crop of 1, 2 and 50 samples from it against the model,
        // at the table's own rate and through a made-up 3 : 2 resampler of 5 taps per side
        for (int64_t s = 0; s < firsts.back(); ++s) {
            if (gsc::crop_frame_at(nf, s, first) != model_frame(firsts, s)) {
                std::printf("FAIL made-up table: sample %lld: frame %d, want %d\n", (long long)s,
                            gsc::crop_frame_at(nf, s, first), model_frame(firsts, s));
                ++g_bad;
            }
            for (int64_t count : {int64_t(1), int64_t(2), int64_t(50)})
                for (int T : {0, 5}) {
                    const int L = T ? 3 : 1, M = T ? 2 : 1;
                    gsc::CropSpan sp;
                    const int st = gsc::crop_plan_one(s, count, 64, firsts.back(), nf, L, M, T, first, &sp);
                    const Model m = model_plan(firsts, 1, gsc::Crop{0, s, count}, 64, L, M, T);
                    if (st != m.status || sp.count != m.count || sp.src_begin != m.src_begin ||
                        sp.src_end != m.src_end || sp.f0 != m.f0 || sp.f1 != m.f1) {
                        std::printf("FAIL made-up table: crop (%lld, %lld) T %d: frames [%d, %d), model [%d, %d)\n",
                                    (long long)s, (long long)count, T, sp.f0, sp.f1, m.f0, m.f1);
                        ++g_bad;
                    }
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
    // all files as the streams of one call: crops over streams of equal channel count, the others refused
    for (size_t i = 0; i + 1 < all.size(); ++i) {
        if (all[i].frames.empty() || all[i + 1].frames.empty()) continue;
        std::vector<const gsc::Index*> ixs{&all[i], &all[i + 1]};
        const int64_t length = 4096;
        if (all[i].channels != all[i + 1].channels) {
            must_refuse(ixs, {1, 0, 1}, length, "streams of different channel counts");
            continue;
        }
        std::vector<gsc::Crop> crops;
        for (int j = 0; j < 32; ++j) {
            const int s = int(rng() & 1);
            crops.push_back({s, int64_t(rng() % uint64_t(ixs[size_t(s)]->samples + 1)), int64_t(rng() % (length + 1))});
        }
        check_plan(ixs, 0, crops, length, rng);
    }
    std::printf("crop_check: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
