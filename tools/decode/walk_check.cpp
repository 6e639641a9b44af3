// Stand-alone driver of the decoder's host walk (gsc_decode_index.cpp, which
// needs no HIP), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc walk_check
//   soundchunks_amd/lib/decode_walk_check FILE.gsc...
// Every file is copied into a heap block of exactly its size, so a read past
// the end is a sanitizer report.  Besides the file as it is, the walk runs on
// the malformed variants tests/test_decode_index.py uses: every cut among
// 1, 11, 13, mid-codebook, mid-FrameLength, len - 1, plus a sweep of cuts, and
// single-byte edits of the header (blend, bit depth, ChunkSize, ChannelCount
// of a second frame).  Prints one line per input; exit status 0 when the
// whole file indexed and no variant was accepted that must be refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_decode.h"

namespace {

// the walk on an exact-size heap copy of [p, p + n)
int walk(const uint8_t* p, size_t n, gsc::Index* ix, std::string* err) {
    uint8_t* c = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    if (n) std::memcpy(c, p, n);
    const int rc = gsc::decode_walk(n ? c : nullptr, n, ix, err);
    std::free(c);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* fp = std::fopen(argv[a], "rb");
        if (!fp) {
            std::printf("%s: cannot open\n", argv[a]);
            ++bad;
            continue;
        }
        std::vector<uint8_t> g;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, fp)) > 0;) g.insert(g.end(), buf, buf + n);
        std::fclose(fp);
        gsc::Index ix;
        std::string err;
        if (walk(g.data(), g.size(), &ix, &err) != 0) {
            std::printf("%s: refused: %s\n", argv[a], err.c_str());
            ++bad;
            continue;
        }
        const gsc::IndexFrame& f0 = ix.frames[0];
        std::vector<size_t> cuts{1, 11, 13, f0.cb_off + (f0.bs_off - 4 - f0.cb_off) / 2, f0.bs_off - 2, g.size() - 1};
        for (size_t c = 0; c < g.size(); c += 1 + g.size() / 97) cuts.push_back(c);
        int refused = 0, accepted = 0;
        for (size_t c : cuts) {
            if (c >= g.size()) continue;
            gsc::Index t;
            std::string e;
            const int rc = walk(g.data(), c, &t, &e);
            // a cut at a frame boundary is a shorter valid stream
            bool boundary = false;
            for (const auto& f : ix.frames) boundary |= f.off == c && c > 0;
            if (rc != 0 && !e.empty()) {
                ++refused;
            } else if (boundary) {
                ++accepted;
            } else {
                std::printf("%s: cut at %zu accepted\n", argv[a], c);
                ++bad;
            }
        }
        struct Edit {
            size_t at;
            uint8_t v;
        };
        std::vector<Edit> edits{{f0.off + 9, 1}, {f0.off + 4, 10}, {f0.off + 5, 0}, {f0.off + 1, 0}, {f0.off + 10, 0}};
        if (ix.frames.size() > 1) edits.push_back({ix.frames[1].off + 1, uint8_t(f0.ch + 1)});
        for (const Edit& ed : edits) {
            std::vector<uint8_t> m = g;
            if (ed.at == f0.off + 10) m[ed.at + 1] = 0;  // AttenuationDivider 0
            m[ed.at] = ed.v;
            gsc::Index t;
            std::string e;
            if (walk(m.data(), m.size(), &t, &e) == 0 || e.empty()) {
                std::printf("%s: edit at %zu accepted\n", argv[a], ed.at);
                ++bad;
            } else {
                ++refused;
            }
        }
        // every byte of the first frame's bitstream head flipped: any outcome but a fault
        for (size_t i = 0; i < 64 && f0.bs_off + i < g.size(); ++i) {
            std::vector<uint8_t> m = g;
            m[f0.bs_off + i] ^= 0xff;
            gsc::Index t;
            std::string e;
            (void)walk(m.data(), m.size(), &t, &e);
        }
        std::printf("%s: %zu frames, %lld samples x %d ch @ %d Hz, %zu checkpoints; %d variants refused, %d boundary cuts\n",
                    argv[a], ix.frames.size(), (long long)ix.samples, ix.channels, ix.rate, ix.cps.size(), refused,
                    accepted);
    }
    return bad ? 1 : 0;
}
