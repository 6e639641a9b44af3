// Stand-alone driver of the stream-set host code (gsc_decode_index.cpp and
// gsc_decode_set.cpp, which need no HIP), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc set_check
//   soundchunks_amd/lib/decode_set_check FILE.gsc...
// Every stream and every table is copied into a heap block of exactly its
// size, so a read past either end is a sanitizer report.  The files are laid
// out as sets of 1, of 2 and of all of them, members indexed in turn from
// their table (tables left unexpanded) and by the walk (tables dropped).  Per
// set: every member frame's rebased offsets and extents against the slab
// sizes, the packed tables' place in the byte slab, the owner of every
// stream's first checkpoint, and the tables expanded on demand against the
// walk's.  Then the per-file cut of a batch's table (index_table_split) over
// all files as one blob with an empty piece in it, and the refusals: no
// streams, a truncated stream, a table of another stream, pieces that do not
// cover the blob.  Prints one line per set; exit status 0 when nothing differed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

struct File {
    std::string name;
    std::unique_ptr<Exact> g, t;
    gsc::Index walked;
};

int bad = 0;
void fail(const std::string& where, const std::string& what) {
    std::printf("%s: %s\n", where.c_str(), what.c_str());
    ++bad;
}

// one set over files[first .. first + n)
void check_set(const std::vector<File>& files, size_t first, size_t n) {
    const std::string where = "set of " + std::to_string(n) + " from " + files[first].name;
    std::vector<gsc::Index> ixs(n);
    std::vector<const gsc::Index*> ptrs(n);
    std::string err;
    for (size_t i = 0; i < n; ++i) {
        const File& f = files[first + i];
        const int rc = i % 2 == 0 ? gsc::index_from_table(f.g->p, f.g->n, f.t->p, f.t->n, &ixs[i], &err, nullptr, false)
                                  : gsc::decode_walk(f.g->p, f.g->n, &ixs[i], &err);
        if (rc != 0) return fail(where, "member " + std::to_string(i) + " refused: " + err);
        if (i % 2 == 1) gsc::index_drop_tables(&ixs[i]);
        if (ixs[i].has_tables || !ixs[i].codebook.empty() || !ixs[i].att.empty())
            return fail(where, "a member holds host tables after the open");
        ptrs[i] = &ixs[i];
    }
    gsc::SetLayout lay;
    if (gsc::set_layout(ptrs.data(), int(n), &lay, &err) != 0) return fail(where, err);
    const gsc::SlabPos& tot = lay.total;
    if (lay.base.size() != n || lay.frame0.size() != n + 1 || lay.frames.size() != size_t(lay.frame0[n]) ||
        lay.src.size() != lay.frames.size() || lay.bits.size() != lay.frames.size())
        return fail(where, "array sizes");
    size_t frames = 0;
    for (size_t i = 0; i < n; ++i) {
        const gsc::Index& ix = ixs[i];
        const gsc::SlabPos& b = lay.base[i];
        if (size_t(lay.frame0[i]) != frames) return fail(where, "frame0");
        if (!ix.cps.empty() && gsc::set_stream_of_checkpoint(lay, b.cps) != int(i))
            return fail(where, "the owner of stream " + std::to_string(i) + "'s first checkpoint");
        if (!ix.cps.empty() && gsc::set_stream_of_checkpoint(lay, b.cps + int64_t(ix.cps.size()) - 1) != int(i))
            return fail(where, "the owner of stream " + std::to_string(i) + "'s last checkpoint");
        for (size_t k = 0; k < ix.frames.size(); ++k, ++frames) {
            const gsc::IndexFrame& f = ix.frames[k];
            const gsc::ResFrame& r = lay.frames[frames];
            const gsc::TableSrc& s = lay.src[frames];
            const int64_t slots = (int64_t(f.count) * f.cs + 7) & ~int64_t(7);
            const int64_t bs_bytes = int64_t((f.nbits + 15) / 16 * 2);
            const int64_t cb_bytes = f.bd == 8 ? int64_t(f.count) * f.cs
                                               : int64_t(f.count) * ((f.cs / 2) * 3 + (f.cs & 1) * 2);
            const bool ok =
                r.bs_off == b.bytes + int64_t(f.bs_off) && r.bs_off >= b.bytes &&
                r.bs_off + bs_bytes <= b.bytes + int64_t(ix.len) && b.bytes + int64_t(ix.len) <= tot.bytes &&
                r.cb_off >= b.cb && (r.cb_off & 7) == 0 && r.cb_off + slots <= tot.cb && r.att_off >= b.att &&
                r.att_off + f.count <= tot.att && r.cp_first >= b.cps &&
                r.cp_first + int64_t(f.cp_count) <= b.cps + int64_t(ix.cps.size()) &&
                b.cps + int64_t(ix.cps.size()) <= tot.cps && r.first_sample == f.first_sample && r.nsym == f.nsym &&
                r.count == f.count && r.cs == f.cs && r.ch == f.ch && r.ver == f.ver &&
                std::memcmp(r.lut, f.lut, sizeof(r.lut)) == 0 && lay.bits[frames] == f.nbits && s.bd == f.bd &&
                s.att_byte == b.bytes + int64_t(f.att_off) && s.att_byte + (f.count + 1) / 2 == s.cb_byte &&
                s.cb_byte + cb_bytes + 4 == r.bs_off;
            if (!ok) return fail(where, "stream " + std::to_string(i) + " frame " + std::to_string(k));
            if (frames + 1 < lay.frames.size() && lay.frames[frames + 1].cb_off != r.cb_off + slots)
                return fail(where, "codebooks are not back to back");
        }
    }
    const gsc::Span last = gsc::span_of(ixs[n - 1], 0, int(ixs[n - 1].frames.size()));
    if (tot.bytes != lay.base[n - 1].bytes + last.count.bytes || tot.cb != lay.base[n - 1].cb + last.count.cb ||
        tot.att != lay.base[n - 1].att + last.count.att || tot.cps != lay.base[n - 1].cps + last.count.cps)
        return fail(where, "totals");
    // the tables on demand: what the walk built, and a second call changes nothing
    for (size_t i = 0; i < n; ++i) {
        const File& f = files[first + i];
        gsc::index_expand_tables(f.g->p, &ixs[i]);
        gsc::index_expand_tables(f.g->p, &ixs[i]);
        if (!ixs[i].has_tables || ixs[i].codebook != f.walked.codebook || ixs[i].att != f.walked.att)
            return fail(where, "member " + std::to_string(i) + ": tables expanded on demand differ from the walk's");
    }
    std::printf("%s: %zu frames, %lld bytes, %lld checkpoints, %lld codebook values, %lld attenuations: ok\n",
                where.c_str(), lay.frames.size(), (long long)tot.bytes, (long long)tot.cps, (long long)tot.cb,
                (long long)tot.att);
}

void check_split(const std::vector<File>& files) {
    const std::string where = "table split";
    // every file as one blob, with an empty piece after the first
    std::vector<uint8_t> blob;
    std::vector<size_t> sizes;
    gsc::Index all;
    for (size_t i = 0; i < files.size(); ++i) {
        const File& f = files[i];
        for (gsc::IndexFrame q : f.walked.frames) {
            q.off += blob.size();
            all.frames.push_back(q);
        }
        all.cps.insert(all.cps.end(), f.walked.cps.begin(), f.walked.cps.end());
        blob.insert(blob.end(), f.g->p, f.g->p + f.g->n);
        sizes.push_back(f.g->n);
        if (i == 0) sizes.push_back(0);
    }
    all.len = blob.size();
    std::vector<uint8_t> t;
    gsc::index_table_write(all, &t);
    const Exact bc(blob.data(), blob.size()), tc(t.data(), t.size());
    std::vector<std::vector<uint8_t>> per;
    std::string err;
    if (gsc::index_table_split(bc.p, bc.n, tc.p, tc.n, sizes.data(), int(sizes.size()), &per, &err) != 0)
        return fail(where, err);
    for (size_t i = 0, p = 0; i < files.size(); ++i, ++p) {
        const File& f = files[i];
        if (per[p].size() != f.t->n || std::memcmp(per[p].data(), f.t->p, f.t->n) != 0)
            return fail(where, f.name + ": the cut table is not the file's own");
        if (i == 0 && !per[++p].empty()) return fail(where, "an empty piece got a table");
    }
    int refused = 0;
    auto must_refuse = [&](const std::vector<size_t>& sz, size_t tn, const char* what) {
        std::vector<std::vector<uint8_t>> o;
        std::string e;
        const Exact cut(tc.p, tn);
        if (gsc::index_table_split(bc.p, bc.n, cut.p, cut.n, sz.data(), int(sz.size()), &o, &e) == 0 || e.empty()) {
            fail(where, std::string(what) + " accepted");
        } else {
            ++refused;
        }
    };
    std::vector<size_t> sz = sizes;
    sz.back() -= 2;
    must_refuse(sz, tc.n, "pieces shorter than the blob");
    sz = sizes;
    sz.back() += 2;
    must_refuse(sz, tc.n, "pieces longer than the blob");
    sz = sizes;
    sz[0] += 2;
    sz.back() -= 2;
    must_refuse(sz, tc.n, "a frame across two pieces");
    for (const size_t tn : {size_t(0), size_t(31), tc.n - 8, tc.n - 1}) must_refuse(sizes, tn, "a cut table");
    for (const size_t at : {size_t(4), size_t(8)}) {  // another version, another S
        std::vector<uint8_t> m(tc.p, tc.p + tc.n);
        m[at] ^= 2;
        std::vector<std::vector<uint8_t>> o;
        std::string e;
        const Exact mc(m.data(), m.size());
        if (gsc::index_table_split(bc.p, bc.n, mc.p, mc.n, sizes.data(), int(sizes.size()), &o, &e) == 0 || e.empty()) {
            fail(where, "a table of another version or S accepted");
        } else {
            ++refused;
        }
    }
    std::printf("%s: %zu files, %zu pieces; %d variants refused: ok\n", where.c_str(), files.size(), sizes.size(),
                refused);
}

void check_refusals(const std::vector<File>& files) {
    const std::string where = "refusals";
    gsc::SetLayout lay;
    std::string err;
    const gsc::Index* one[1] = {&files[0].walked};
    if (gsc::set_layout(one, 0, &lay, &err) == 0 || err.empty()) fail(where, "count 0 accepted");
    err.clear();
    if (gsc::set_layout(nullptr, 1, &lay, &err) == 0 || err.empty()) fail(where, "no streams accepted");
    for (const File& f : files) {
        // truncated, without a table: the walk refuses; with its table: the host half does
        gsc::Index ix;
        const Exact cut(f.g->p, f.g->n - 1);
        err.clear();
        if (gsc::decode_walk(cut.p, cut.n, &ix, &err) == 0 || err.empty()) fail(where, f.name + ": truncated, walked");
        err.clear();
        if (gsc::index_from_table(cut.p, cut.n, f.t->p, f.t->n, &ix, &err, nullptr, false) == 0 || err.empty())
            fail(where, f.name + ": truncated, with its table");
    }
    for (size_t i = 0; i + 1 < files.size(); ++i) {
        // a table of another stream: refused by the host half, or left to the device when the layouts agree
        gsc::Index ix;
        err.clear();
        const File &a = files[i], &b = files[i + 1];
        if (gsc::index_from_table(a.g->p, a.g->n, b.t->p, b.t->n, &ix, &err, nullptr, false) == 0 && a.g->n != b.g->n)
            fail(where, a.name + " with the table of " + b.name);
    }
    std::printf("%s: ok\n", where.c_str());
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<File> files;
    for (int a = 1; a < argc; ++a) {
        std::FILE* fp = std::fopen(argv[a], "rb");
        if (!fp) {
            fail(argv[a], "cannot open");
            continue;
        }
        std::vector<uint8_t> g;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, fp)) > 0;) g.insert(g.end(), buf, buf + n);
        std::fclose(fp);
        File f;
        f.name = argv[a];
        f.g.reset(new Exact(g.data(), g.size()));
        std::string err;
        if (gsc::decode_walk(f.g->p, f.g->n, &f.walked, &err) != 0) {
            fail(argv[a], "the walk refused it: " + err);
            continue;
        }
        std::vector<uint8_t> t;
        gsc::index_table_write(f.walked, &t);
        f.t.reset(new Exact(t.data(), t.size()));
        files.push_back(std::move(f));
    }
    if (files.empty()) {
        std::printf("no streams\n");
        return 1;
    }
    for (size_t i = 0; i < files.size(); ++i) check_set(files, i, 1);
    for (size_t i = 0; i + 1 < files.size(); ++i) check_set(files, i, 2);
    check_set(files, 0, files.size());
    check_split(files);
    check_refusals(files);
    return bad ? 1 : 0;
}
