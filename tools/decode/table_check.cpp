// Stand-alone driver of the seek-table code (gsc_decode_index.cpp, which needs
// no HIP), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc table_check
//   soundchunks_amd/lib/decode_table_check FILE.gsc...
// Every stream and every table is copied into a heap block of exactly its
// size, so a read past either end is a sanitizer report.  Per file: the walk,
// index_table_write (twice, the bytes must agree), the host half of
// index_from_table on the table as written (it must accept, and fill the
// index as the walk did), on the table cut at every length below its size and
// one byte longer (each must be refused), on every header field overwritten
// with a few values, on shifted frame offsets and bit counts and on edited
// checkpoints (any answer but a fault; those that must be refused are
// counted).  Prints one line per input; exit status 0 when nothing was
// accepted that must be refused and nothing differed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_decode.h"

namespace {

struct Exact {  // an exact-size heap copy
    uint8_t* p;
    size_t n;
    Exact(const uint8_t* s, size_t len) : p(static_cast<uint8_t*>(std::malloc(len ? len : 1))), n(len) {
        if (len) std::memcpy(p, s, len);
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

int from_table(const Exact& g, const uint8_t* t, size_t tn, gsc::Index* ix, std::string* err) {
    const Exact tc(t, tn);
    return gsc::index_from_table(g.p, g.n, tc.p, tc.n, ix, err);
}

bool same_index(const gsc::Index& a, const gsc::Index& b) {
    if (a.frames.size() != b.frames.size() || a.cps != b.cps || a.codebook != b.codebook || a.att != b.att ||
        a.channels != b.channels || a.rate != b.rate || a.samples != b.samples || a.symbols != b.symbols ||
        a.len != b.len)
        return false;
    for (size_t i = 0; i < a.frames.size(); ++i) {
        const gsc::IndexFrame &x = a.frames[i], &y = b.frames[i];
        if (x.off != y.off || x.att_off != y.att_off || x.cb_off != y.cb_off || x.bs_off != y.bs_off ||
            x.end_off != y.end_off || x.ver != y.ver || x.ch != y.ch || x.count != y.count || x.bd != y.bd ||
            x.cs != y.cs || x.rate != y.rate || x.adiv != y.adiv || x.flen != y.flen || x.nsym != y.nsym ||
            x.nbits != y.nbits || x.first_sample != y.first_sample || x.cp_first != y.cp_first ||
            x.cp_count != y.cp_count || x.cb_first != y.cb_first || x.att_first != y.att_first ||
            std::memcmp(x.lut, y.lut, sizeof(x.lut)) != 0)
            return false;
    }
    return true;
}

void put(std::vector<uint8_t>* t, size_t at, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) (*t)[at + size_t(i)] = uint8_t(v >> (8 * i));
}
uint64_t get64(const std::vector<uint8_t>& t, size_t at) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = v << 8 | t[at + size_t(i)];
    return v;
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
        const Exact gc(g.data(), g.size());
        if (gsc::decode_walk(gc.p, gc.n, &ix, &err) != 0) {
            std::printf("%s: the walk refused it: %s\n", argv[a], err.c_str());
            ++bad;
            continue;
        }
        std::vector<uint8_t> t, t2;
        gsc::index_table_write(ix, &t);
        gsc::index_table_write(ix, &t2);
        const size_t F = ix.frames.size(), P = ix.cps.size();
        if (t != t2 || t.size() != 32 + 16 * F + 8 * P) {
            std::printf("%s: table of %zu bytes, F %zu P %zu, or two writes differ\n", argv[a], t.size(), F, P);
            ++bad;
            continue;
        }
        gsc::Index jx;
        if (from_table(gc, t.data(), t.size(), &jx, &err) != 0 || !same_index(ix, jx)) {
            std::printf("%s: its own table: %s\n", argv[a], err.empty() ? "another index than the walk's" : err.c_str());
            ++bad;
            continue;
        }
        int refused = 0, other = 0;
        auto must_refuse = [&](const std::vector<uint8_t>& m, size_t n, const char* what, size_t at) {
            gsc::Index k;
            std::string e;
            if (from_table(gc, m.data(), n, &k, &e) == 0 || e.empty()) {
                std::printf("%s: %s at %zu accepted\n", argv[a], what, at);
                ++bad;
            } else {
                ++refused;
            }
        };
        auto any = [&](const std::vector<uint8_t>& m) {
            gsc::Index k;
            std::string e;
            if (from_table(gc, m.data(), m.size(), &k, &e) != 0) {
                ++refused;
            } else {
                ++other;  // left to the check on the device
            }
        };
        // every length below the table's size, and one byte more
        for (size_t n = 0; n < t.size(); ++n) must_refuse(t, n, "cut", n);
        {
            std::vector<uint8_t> m = t;
            m.push_back(0);
            must_refuse(m, m.size(), "over-long table", m.size());
        }
        // every header field
        struct Field {
            size_t at;
            int bytes;
        };
        const Field fields[] = {{0, 4}, {4, 4}, {8, 4}, {12, 4}, {16, 8}, {24, 8}};
        for (const Field& fd : fields) {
            uint64_t cur = 0;
            for (int i = fd.bytes - 1; i >= 0; --i) cur = cur << 8 | t[fd.at + size_t(i)];
            const uint64_t vals[] = {0, cur + 1, cur - 1, cur * 2 + 3, ~uint64_t(0), uint64_t(1) << 31, uint64_t(1) << 61};
            for (const uint64_t v : vals) {
                std::vector<uint8_t> m = t;
                put(&m, fd.at, v, fd.bytes);
                if (m == t) continue;
                must_refuse(m, m.size(), "header field", fd.at);
            }
        }
        // frame offsets and bit counts shifted; checkpoints edited
        for (size_t k = 0; k < F && k < 64; ++k) {
            const size_t at = 32 + 16 * k;
            for (const int64_t d : {-16, -2, -1, 1, 2, 16}) {
                std::vector<uint8_t> m = t;
                put(&m, at, get64(t, at) + uint64_t(d), 8);
                must_refuse(m, m.size(), "shifted frame offset", at);
                m = t;
                put(&m, at + 8, get64(t, at + 8) + uint64_t(d), 8);
                if (d == -16 || d == 16) {
                    must_refuse(m, m.size(), "bit count moved by a word", at + 8);
                } else {
                    any(m);
                }
            }
            std::vector<uint8_t> m = t;
            put(&m, at, ~uint64_t(0), 8);
            must_refuse(m, m.size(), "frame offset", at);
            m = t;
            put(&m, at + 8, ~uint64_t(0), 8);
            must_refuse(m, m.size(), "bit count", at + 8);
        }
        for (size_t i = 0; i < P; i += 1 + P / 61) {
            const size_t at = 32 + 16 * F + 8 * i;
            const uint64_t c = get64(t, at);
            for (const uint64_t v : {c + 8, c - 8, c ^ 1, (c & ~uint64_t(7)) | 5, (c & ~uint64_t(7)) | 7, ~uint64_t(0)}) {
                std::vector<uint8_t> m = t;
                put(&m, at, v, 8);
                if ((v & 7) > 4) {
                    must_refuse(m, m.size(), "checkpoint header state", at);
                } else {
                    any(m);
                }
            }
        }
        std::printf("%s: %zu frames, %zu checkpoints, table %zu bytes; %d variants refused, %d left to the device\n",
                    argv[a], F, P, t.size(), refused, other);
    }
    return bad ? 1 : 0;
}
