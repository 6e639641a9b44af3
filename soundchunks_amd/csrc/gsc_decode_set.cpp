// .gsc decoder, the layout of what goes to the device: what
// a range of frames occupies of its stream (span_of), a frame's descriptor
// once its stream has a place in the slabs (frame_tables), and the layout of
// a whole stream set (set_layout).  Plain C++, no device needed;
// gsc_decode_abi.cpp allocates, uploads and launches by it.
#include "gsc_decode.h"

#include <algorithm>
#include <cstring>

namespace gsc {

Span span_of(const Index& ix, int b, int e) {
    if (b >= e) return Span{};
    const IndexFrame& fb = ix.frames[size_t(b)];
    const IndexFrame& fe = ix.frames[size_t(e) - 1];
    const SlabPos first{int64_t(fb.off), int64_t(fb.cp_first), int64_t(fb.cb_first), int64_t(fb.att_first)};
    const SlabPos end{int64_t(fe.end_off), int64_t(fe.cp_first + fe.cp_count),
                      int64_t(fe.cb_first + ((size_t(fe.count) * size_t(fe.cs) + 7) & ~size_t(7))),
                      int64_t(fe.att_first + size_t(fe.count))};
    return Span{first, end - first};
}

FrameTables frame_tables(const IndexFrame& f, const SlabPos& rebase) {
    FrameTables d{};
    d.bs_off = rebase.bytes + int64_t(f.bs_off);
    d.cb_off = rebase.cb + int64_t(f.cb_first);
    d.att_off = rebase.att + int64_t(f.att_first);
    d.nsym = f.nsym;
    d.cp_first = rebase.cps + int64_t(f.cp_first);
    d.ver = f.ver;
    d.ch = f.ch;
    d.cs = f.cs;
    d.count = f.count;
    std::memcpy(d.lut, f.lut, sizeof(d.lut));
    return d;
}

int set_layout(const Index* const* ixs, int count, SetLayout* out, std::string* err) {
    *out = SetLayout();
    if (!ixs || count <= 0) {
        if (err) *err = "gsc stream set: no streams";
        return -1;
    }
    out->base.resize(size_t(count));
    out->frame0.assign(size_t(count) + 1, 0);
    int64_t nframes = 0, ncps = 0;
    for (int i = 0; i < count; ++i) {
        nframes += int64_t(ixs[i]->frames.size());
        ncps += int64_t(ixs[i]->cps.size());
        if (nframes >= (int64_t(1) << 31) || ncps >= (int64_t(1) << 31)) {
            if (err) *err = "gsc stream set: 2^31 or more frames or checkpoints in one set";
            return -1;
        }
        out->frame0[size_t(i) + 1] = nframes;
    }
    out->frames.reserve(size_t(nframes));
    out->src.reserve(size_t(nframes));
    out->bits.reserve(size_t(nframes));
    for (int i = 0; i < count; ++i) {
        const Index& ix = *ixs[i];
        const Span sp = span_of(ix, 0, int(ix.frames.size()));  // the whole stream: sp.first is all zero
        const SlabPos base = out->base[size_t(i)] = out->total;
        out->total = out->total + sp.count;
        for (const IndexFrame& f : ix.frames) {
            ResFrame r{};
            static_cast<FrameTables&>(r) = frame_tables(f, base - sp.first);
            r.first_sample = f.first_sample;
            out->frames.push_back(r);
            out->src.push_back(TableSrc{base.bytes + int64_t(f.att_off), base.bytes + int64_t(f.cb_off), f.bd, 0});
            out->bits.push_back(f.nbits);
        }
    }
    return 0;
}

int set_stream_of_checkpoint(const SetLayout& lay, int64_t c) {
    int lo = 0, hi = int(lay.base.size()) - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (lay.base[size_t(mid)].cps <= c) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

}  // namespace gsc
