// Stand-alone driver of the decoder's sample locator and crop planner
// (gsc_decode_index.cpp, which needs no HIP: gsc::index_locate, which
// gsc_index_locate wraps, and gsc::plan_crops, which gsc_decode_crops runs
// before it launches anything), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc crop_check
//   soundchunks_amd/lib/decode_crop_check FILE.gsc...
// For every file: locate at every frame edge +-1 and at random positions
// against a linear search, then batches of edge and random crops through the
// planner, checking that
//   - every sample of a crop (its ends, the frame edges inside it, random ones)
//     lies in a frame of the crop's span whose piece's segments hold its symbol,
//   - every offset the kernels derive from the plan stays inside its slab
//     (checkpoints, the byte slab, codebook, attenuations, the symbol scratch),
//   - the slots of the pieces tile the scratch without overlap,
//   - crops that must be refused are refused with a message.
// Prints one line per file; exit status 0 when nothing failed.
#include <cstdio>
#include <cstdlib>
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

// one sample of crop ci: its symbol must sit in a slot the plan unpacks
void check_sample(const std::vector<const gsc::Index*>& ixs, const gsc::CropPlan& plan, size_t ci, int64_t t) {
    const gsc::PlanCrop& pc = plan.crops[ci];
    const gsc::Index& ix = *ixs[size_t(pc.stream)];
    int fr = -1, within = -1;
    int64_t row = -1, cp = -1;
    std::string err;
    CHECK(gsc::index_locate(ix, pc.begin + t, &fr, &row, &within, &cp, &err) == 0, "crop %zu t %lld: %s", ci,
          (long long)t, err.c_str());
    CHECK(fr >= pc.f0 && fr < pc.f1, "crop %zu t %lld: frame %d outside [%d, %d)", ci, (long long)t, fr, pc.f0, pc.f1);
    const size_t pi = size_t(pc.piece0 + (fr - pc.f0));
    CHECK(pi < plan.pieces.size(), "crop %zu: piece index", ci);
    const gsc::CropPiece& p = plan.pieces[pi];
    CHECK(p.crop == int(ci) && p.frame == fr, "crop %zu: piece %zu names crop %d frame %d", ci, pi, p.crop, p.frame);
    const gsc::IndexFrame& f = ix.frames[size_t(fr)];
    for (int k = 0; k < f.ch; k += (f.ch > 1 ? f.ch - 1 : 1)) {
        const int64_t si = row * f.ch + k;
        const int64_t rel = si / gsc::kDecodeS - p.seg0;
        CHECK(si < f.nsym && rel >= 0 && rel < p.nseg, "crop %zu t %lld ch %d: symbol %lld not in segments [%lld, +%d)",
              ci, (long long)t, k, (long long)si, (long long)p.seg0, p.nseg);
        CHECK(p.slot0 + rel < plan.slots, "crop %zu: slot past the scratch", ci);
    }
}

void check_plan(const std::vector<const gsc::Index*>& ixs, const std::vector<gsc::Crop>& crops, int64_t length,
                std::mt19937_64& rng) {
    gsc::CropPlan plan;
    std::string err;
    const int rc = gsc::plan_crops(ixs.data(), int(ixs.size()), crops.data(), int(crops.size()), length, &plan, &err);
    CHECK(rc == 0, "plan refused: %s", err.c_str());
    CHECK(plan.crops.size() == crops.size(), "crop count");
    int64_t slot = 0;
    size_t piece = 0;
    for (size_t ci = 0; ci < crops.size(); ++ci) {
        const gsc::PlanCrop& pc = plan.crops[ci];
        const gsc::Index& ix = *ixs[size_t(pc.stream)];
        const int64_t want = std::min<int64_t>(crops[ci].count, ix.samples - crops[ci].begin);
        CHECK(pc.begin == crops[ci].begin && pc.count == want && pc.count <= length, "crop %zu: clipped count %lld", ci,
              (long long)pc.count);
        CHECK(size_t(pc.piece0) == piece && pc.f0 >= 0 && pc.f0 <= pc.f1 && size_t(pc.f1) <= ix.frames.size(),
              "crop %zu: span", ci);
        CHECK((pc.count == 0) == (pc.f0 == pc.f1), "crop %zu: empty span", ci);
        for (int fi = pc.f0; fi < pc.f1; ++fi, ++piece) {
            CHECK(piece < plan.pieces.size(), "crop %zu: pieces run out", ci);
            const gsc::CropPiece& p = plan.pieces[piece];
            const gsc::IndexFrame& f = ix.frames[size_t(fi)];
            CHECK(p.slot0 == slot && p.nseg >= 0 && p.seg0 >= 0, "crop %zu frame %d: slots do not tile", ci, fi);
            CHECK((f.nsym == 0) == (p.nseg == 0), "crop %zu frame %d: nseg %d for %lld symbols", ci, fi, p.nseg,
                  (long long)f.nsym);
            // every segment is one of the frame's checkpoints, and its bits start inside the file
            CHECK(p.seg0 + p.nseg <= int64_t(f.cp_count), "crop %zu frame %d: segments past the frame's checkpoints", ci,
                  fi);
            for (int64_t s = p.seg0; s < p.seg0 + p.nseg; ++s) {
                const uint64_t cpv = ix.cps[f.cp_first + size_t(s)];
                CHECK(f.bs_off + (cpv >> 3) / 8 < ix.len && (cpv >> 3) <= f.nbits && (cpv & 7) <= 4,
                      "crop %zu frame %d: checkpoint %lld", ci, fi, (long long)s);
                CHECK(s * gsc::kDecodeS < f.nsym, "crop %zu frame %d: empty segment", ci, fi);
            }
            CHECK(f.cb_first + size_t(f.count) * size_t(f.cs) <= ix.codebook.size() &&
                      f.att_first + size_t(f.count) <= ix.att.size(),
                  "crop %zu frame %d: tables past their slabs", ci, fi);
            slot += p.nseg;
        }
        if (pc.count > 0) {
            std::vector<int64_t> ts{0, pc.count - 1, pc.count / 2};
            for (int fi = pc.f0; fi < pc.f1; ++fi) {
                const int64_t e = ix.frames[size_t(fi)].first_sample - pc.begin;
                for (int64_t d = -1; d <= 1; ++d)
                    if (e + d >= 0 && e + d < pc.count) ts.push_back(e + d);
            }
            for (int i = 0; i < 16; ++i) ts.push_back(int64_t(rng() % uint64_t(pc.count)));
            for (int64_t t : ts) check_sample(ixs, plan, ci, t);
        }
    }
    CHECK(piece == plan.pieces.size() && slot == plan.slots, "pieces / slots left over");
}

void must_refuse(const std::vector<const gsc::Index*>& ixs, gsc::Crop c, int64_t length, const char* what) {
    gsc::CropPlan plan;
    std::string err;
    std::vector<gsc::Crop> crops{gsc::Crop{0, 0, 0}, c};
    const int rc = gsc::plan_crops(ixs.data(), int(ixs.size()), crops.data(), 2, length, &plan, &err);
    CHECK(rc != 0 && !err.empty(), "%s accepted", what);
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
        std::vector<gsc::Crop> crops{{0, 0, 0}, {0, n, 0}, {0, n, length}, {0, 0, std::min(n, length)},
                                     {0, std::max<int64_t>(n - 1, 0), length}, {0, 0, 1}};
        for (const auto& f : ix.frames)
            for (int64_t d = -2; d <= 1; ++d)
                for (int64_t c : {int64_t(1), int64_t(2), int64_t(3), length}) {
                    const int64_t b = f.first_sample + d;
                    if (b >= 0 && b <= n) crops.push_back({0, b, c});
                }
        for (int i = 0; i < 64 && n > 0; ++i)
            crops.push_back({0, int64_t(rng() % uint64_t(n + 1)), int64_t(rng() % uint64_t(length + 1))});
        check_plan(ixs, crops, length, rng);
        check_plan(ixs, {}, length, rng);

        must_refuse(ixs, {0, -1, 1}, length, "begin -1");
        must_refuse(ixs, {0, n + 1, 0}, length, "begin samples + 1");
        must_refuse(ixs, {0, 0, -1}, length, "count -1");
        must_refuse(ixs, {0, 0, length + 1}, length, "count length + 1");
        must_refuse(ixs, {1, 0, 1}, length, "stream index 1 of 1");
        must_refuse(ixs, {-1, 0, 1}, length, "stream index -1");
        must_refuse(ixs, {0, int64_t(1) << 62, 1}, length, "begin 2^62");
        std::printf("%s: %zu frames, %lld samples: %zu positions located, %zu crops planned, 7 refusals%s\n", argv[a],
                    ix.frames.size(), (long long)n, pos.size(), crops.size(), g_bad == bad_before ? "" : " FAILED");
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
        check_plan(ixs, crops, length, rng);
    }
    std::printf("crop_check: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
