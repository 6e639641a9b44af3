// Stand-alone driver of the envelope's layout (gsc_envelope.h:
// gsc::envelope_layout and the tile rule envelope_kernel runs by), meant for a
// host sanitizer build:
//   make -C soundchunks_amd/csrc envelope_check
//   soundchunks_amd/lib/decode_envelope_check FILE.gsc...
// Over the lengths of all files as one binding (with a stream of no samples
// among them) and the hops 64, 65, 1000, 1024, 4096, 4097 and 65536: the block
// offsets against ceil(samples / hop) summed up; the tile rule (a whole number
// of hops, the largest not above 4096 samples, or one hop); that the tiles of a
// stream, taken as envelope_kernel takes them (workgroup -> last stream whose
// first workgroup is not behind it, tile = the difference, blocks [tile * bpt,
// min((tile + 1) * bpt, nb))), cover every block of the output exactly once and
// nothing else, and that a tile's samples are those of its blocks; and the
// refusals.  One line per hop; exit status 0 when nothing failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_decode.h"
#include "../../soundchunks_amd/csrc/gsc_envelope.h"

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

void check_hop(const std::vector<int64_t>& samples, int hop) {
    const int n = int(samples.size());
    std::vector<int64_t> off(size_t(n) + 1, -1), tile0(size_t(n) + 1, -1);
    std::string err;
    CHECK(gsc::envelope_layout(samples.data(), n, hop, off.data(), tile0.data(), &err) == 0, "hop %d refused: %s", hop,
          err.c_str());
    // the tile rule
    const int tile = gsc::envelope_tile_len(hop);
    CHECK(tile % hop == 0 && tile >= hop, "hop %d: tile %d", hop, tile);
    if (hop > gsc::kEnvelopeTile) {
        CHECK(tile == hop, "hop %d: tile %d", hop, tile);
    } else {
        CHECK(tile <= gsc::kEnvelopeTile && tile + hop > gsc::kEnvelopeTile, "hop %d: tile %d", hop, tile);
    }
    const int bpt = tile / hop;
    CHECK(bpt >= 1 && bpt <= gsc::kEnvelopeMaxBlocks, "hop %d: %d blocks per tile", hop, bpt);
    // the offsets
    int64_t blocks = 0, tiles = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(off[size_t(i)] == blocks && tile0[size_t(i)] == tiles, "hop %d stream %d: offsets", hop, i);
        const int64_t nb = (samples[size_t(i)] + hop - 1) / hop;
        blocks += nb;
        tiles += (nb + bpt - 1) / bpt;
    }
    CHECK(off[size_t(n)] == blocks && tile0[size_t(n)] == tiles, "hop %d: totals", hop);
    // the kernel's walk: every workgroup's blocks
    std::vector<int> owners(size_t(blocks), 0);
    for (int64_t wg = 0; wg < tiles; ++wg) {
        int lo = 0, hi = n - 1;  // last_le
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tile0[size_t(mid)] <= wg) {
                lo = mid;
            } else {
                hi = mid - 1;
            }
        }
        const int s = lo;
        const int64_t t = wg - tile0[size_t(s)], nt = tile0[size_t(s) + 1] - tile0[size_t(s)];
        const int64_t nb = off[size_t(s) + 1] - off[size_t(s)];
        CHECK(t >= 0 && t < nt && t * bpt < nb, "hop %d workgroup %lld: stream %d tile %lld of %lld", hop,
              (long long)wg, s, (long long)t, (long long)nt);
        const int64_t b1 = std::min<int64_t>((t + 1) * bpt, nb);
        for (int64_t b = t * bpt; b < b1; ++b) ++owners[size_t(off[size_t(s)] + b)];
        // the tile's samples are those of its blocks
        const int64_t s0 = t * tile, s1 = std::min<int64_t>(s0 + tile, samples[size_t(s)]);
        CHECK(s0 == t * bpt * hop && s0 < s1 && (s1 - s0 + hop - 1) / hop == b1 - t * bpt,
              "hop %d workgroup %lld: samples [%lld, %lld)", hop, (long long)wg, (long long)s0, (long long)s1);
    }
    for (int64_t b = 0; b < blocks; ++b)
        CHECK(owners[size_t(b)] == 1, "hop %d: block %lld has %d owners", hop, (long long)b, owners[size_t(b)]);
    std::printf("hop %d: tile %d, %d streams, %lld blocks in %lld tiles\n", hop, tile, n, (long long)blocks,
                (long long)tiles);
}

void check_refusals() {
    const int64_t one[1] = {1000}, neg[2] = {5, -1};
    int64_t off[3];
    std::string err;
    for (int hop : {63, 65537, 0, -1024}) {
        err.clear();
        CHECK(gsc::envelope_layout(one, 1, hop, off, nullptr, &err) != 0 && !err.empty(), "hop %d accepted", hop);
    }
    CHECK(gsc::envelope_layout(one, -1, 1024, off, nullptr, &err) != 0, "n = -1 accepted");
    CHECK(gsc::envelope_layout(neg, 2, 1024, off, nullptr, &err) != 0, "a negative length accepted");
    // 2^31 blocks in one stream, and in two; one fewer is taken
    const int64_t big[1] = {(int64_t(1) << 31) * 64}, two[2] = {(int64_t(1) << 30) * 64, (int64_t(1) << 30) * 64};
    const int64_t under[2] = {(int64_t(1) << 30) * 64, ((int64_t(1) << 30) - 1) * 64};
    CHECK(gsc::envelope_layout(big, 1, 64, off, nullptr, &err) != 0, "2^31 blocks accepted");
    CHECK(gsc::envelope_layout(two, 2, 64, off, nullptr, &err) != 0, "2 x 2^30 blocks accepted");
    CHECK(gsc::envelope_layout(under, 2, 64, off, nullptr, &err) == 0 && off[2] == (int64_t(1) << 31) - 1,
          "2^31 - 1 blocks refused");
    const int64_t huge[1] = {INT64_MAX};
    CHECK(gsc::envelope_layout(huge, 1, 65536, off, nullptr, &err) != 0, "2^63 - 1 samples accepted");
    // no streams: no blocks
    CHECK(gsc::envelope_layout(nullptr, 0, 1024, off, nullptr, &err) == 0 && off[0] == 0, "no streams refused");
    std::printf("refusals: checked\n");
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<int64_t> samples{0};
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
        samples.push_back(ix.samples);
    }
    // around a hop and a tile, and an empty stream at the end
    for (int64_t s : {1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 0}) samples.push_back(s);
    for (int hop : {64, 65, 1000, 1024, 4096, 4097, 65536}) check_hop(samples, hop);
    check_refusals();
    std::printf("envelope_check: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
