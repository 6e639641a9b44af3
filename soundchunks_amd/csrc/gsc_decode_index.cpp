// .gsc decoder, the host index (decoder/decoder.lpr:37-220):
// the sequential walk, seek tables and the sample locator.  Plain C++,
// no device needed; gsc_decode_abi.cpp holds the HIP runtime side.
//
// A .gsc is a concatenation of frames: 12-byte header, attenuation nibbles,
// codebook, u32 FrameLength, then FrameLength x ChannelCount variable-length
// symbols, LSB first in 16-bit words.  Two chains are sequential by format:
// frame k + 1 starts where frame k's bitstream ends, and symbol j's bit offset
// and header state depend on every earlier symbol of its frame.  decode_walk
// follows both chains once, validates every field and index on the way, and
// leaves a checkpoint (bit offset, header state) every kDecodeS symbols; from
// there on everything is parallel: one device lane unpacks one checkpoint
// segment, one lane writes one output sample (gsc_decode.hip).
//
// For sample ranges of a resident stream, index_locate finds the checkpoint
// at or before a sample; a batch of ranges is planned by plan_crops
// (gsc_resample.cpp) for gsc_decode_crops.hip.
#include "gsc_decode.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace gsc {
namespace {

// FPC round(): round half to even (the default rounding mode)
inline int64_t fpc_round(double x) { return int64_t(std::nearbyint(x)); }

inline uint32_t rd16(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | rd16(p + 2) << 16; }

int walk_fail(std::string* err, size_t frame, const std::string& what) {
    if (err) *err = "gsc decode: frame " + std::to_string(frame) + ": " + what;
    return -1;
}

inline uint64_t rd64(const uint8_t* p) { return uint64_t(rd32(p)) | uint64_t(rd32(p + 4)) << 32; }
inline void wr32(uint8_t* p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = uint8_t(v >> (8 * i));
}
inline void wr64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = uint8_t(v >> (8 * i));
}

// The header of frame k at byte `off`, for the walk and for index_from_table:
// every field validation, CAttrLookup, the offsets of the attenuations, the
// codebook and the bitstream, and nsym.  Nothing is sized by FrameLength
// before nsym > avail / 2 is refused.  `first`: frame 0, nullptr for k = 0.
int frame_head(const uint8_t* g, size_t len, size_t off, size_t k, const IndexFrame* first, IndexFrame* out,
               std::string* err) {
    IndexFrame& f = *out;
    size_t pos = off;
    f.off = pos;
    if (pos > len || len - pos < 12) return walk_fail(err, k, "truncated header");
    f.ver = g[pos];
    f.ch = g[pos + 1];
    f.count = int(rd16(g + pos + 2) & 0x1fff);
    f.bd = g[pos + 4];
    f.cs = g[pos + 5];
    const uint32_t srw = rd32(g + pos + 6);
    f.rate = int(srw & 0xffffff);
    f.adiv = int(rd16(g + pos + 10));
    pos += 12;
    if ((srw >> 24) != 0) return walk_fail(err, k, "ChunkBlend not supported");
    if (f.bd != 8 && f.bd != 12) return walk_fail(err, k, "ChunkBitDepth " + std::to_string(f.bd) + " not supported");
    if (f.cs == 0) return walk_fail(err, k, "ChunkSize 0");
    if (f.ch == 0) return walk_fail(err, k, "ChannelCount 0");
    if (f.adiv == 0) return walk_fail(err, k, "AttenuationDivider 0");
    if (first && (f.ch != first->ch || f.rate != first->rate))
        return walk_fail(err, k, "ChannelCount / SampleRate differ from frame 0");
    // CAttrLookup (decoder.lpr:88-96); CAttrMul (decoder.lpr:6)
    {
        const double attr_mul = double(fpc_round(32768.0 * (32767.0 / 2047.0)));
        const double law = 1.0 / double(f.adiv);
        double acc = 1.0;
        for (int i = 0; i <= 15; ++i) {
            acc += law * double(i);
            const int32_t v = int32_t(fpc_round(attr_mul / acc));
            f.lut[i] = v;
            f.lut[16 + i] = -v;
        }
    }
    const size_t count = size_t(f.count), cs = size_t(f.cs);
    const size_t att_bytes = (count + 1) / 2;
    const size_t cb_bytes = f.bd == 8 ? count * cs : count * ((cs / 2) * 3 + (cs & 1) * 2);
    if (len - pos < att_bytes) return walk_fail(err, k, "truncated attenuations");
    f.att_off = pos;
    pos += att_bytes;
    if (len - pos < cb_bytes) return walk_fail(err, k, "truncated codebook");
    f.cb_off = pos;
    pos += cb_bytes;
    if (len - pos < 4) return walk_fail(err, k, "truncated FrameLength");
    f.flen = rd32(g + pos);
    pos += 4;
    f.bs_off = pos;
    const uint64_t avail = uint64_t(len - pos) * 8;
    const uint64_t nsym = uint64_t(f.flen) * uint64_t(f.ch);
    // a symbol has at least 2 bits: refuse before sizing anything by FrameLength
    if (nsym > avail / 2) return walk_fail(err, k, "FrameLength needs bits past the end of the stream");
    f.nsym = int64_t(nsym);
    return 0;
}

// int16 values a frame's codebook occupies in Index::codebook (padded to 8)
inline size_t codebook_slots(const IndexFrame& f) { return (size_t(f.count) * size_t(f.cs) + 7) & ~size_t(7); }

// The tables of a frame whose head was read: `count` attenuations to a and
// count * cs codebook values to c (Attenuations and Chunks, decoder.lpr:115-158).
void frame_tables_expand(const uint8_t* g, const IndexFrame& f, uint8_t* a, int16_t* c) {
    const size_t count = size_t(f.count), cs = size_t(f.cs);
    const uint8_t* pa = g + f.att_off;
    for (size_t i = 0; i < count / 2; ++i) {
        const uint8_t b = pa[i];
        a[2 * i] = b >> 4;
        a[2 * i + 1] = b & 0x0f;
    }
    if (count & 1) a[count - 1] = pa[count / 2] >> 4;
    const uint8_t* p = g + f.cb_off;
    if (f.bd == 8) {
        // Pascal div truncates toward zero, as C's /
        for (size_t i = 0; i < count * cs; ++i) c[i] = int16_t((int(p[i]) - 128) * 2047 / 127);
    } else {
        for (size_t i = 0; i < count; ++i) {
            for (size_t j = 0; j < cs / 2; ++j) {
                const int b = p[0];
                c[i * cs + 2 * j] = int16_t((int(p[1]) | (b & 0xf0) << 4) - 2048);
                c[i * cs + 2 * j + 1] = int16_t((int(p[2]) | (b & 0x0f) << 8) - 2048);
                p += 3;
            }
            if (cs & 1) {
                const int b = p[0];
                c[i * cs + cs - 1] = int16_t((int(p[1]) | (b & 0xf0) << 4) - 2048);
                p += 2;
            }
        }
    }
}

int table_fail(std::string* err, const std::string& what) {
    if (err) *err = "gsc seek table: " + what;
    return -1;
}

}  // namespace

int decode_walk(const uint8_t* g, size_t len, Index* ix, std::string* err) {
    *ix = Index();
    if (!g || len == 0) {
        if (err) *err = "gsc decode: empty stream";
        return -1;
    }
    size_t pos = 0;
    while (pos < len) {
        const size_t k = ix->frames.size();
        IndexFrame f;
        if (frame_head(g, len, pos, k, k ? &ix->frames[0] : nullptr, &f, err) != 0) return -1;
        if (k == 0) {
            ix->channels = f.ch;
            ix->rate = f.rate;
        }
        f.att_first = ix->att.size();
        ix->att.resize(f.att_first + size_t(f.count));
        f.cb_first = ix->codebook.size();
        ix->codebook.resize(f.cb_first + codebook_slots(f), 0);
        frame_tables_expand(g, f, ix->att.data() + f.att_first, ix->codebook.data() + f.cb_first);
        pos = f.bs_off;
        const uint8_t* bs = g + pos;
        const size_t bl = len - pos;
        const uint64_t avail = uint64_t(bl) * 8;
        const uint64_t nsym = uint64_t(f.nsym);
        f.first_sample = ix->samples;
        f.cp_first = ix->cps.size();
        const int rev_bit = f.ver > 0 ? 1 : 0;
        uint64_t p = 0;
        int hdr = -1;  // variableCodingHeader (decoder.lpr:173)
        int until_cp = 0;
        for (uint64_t s = 0; s < nsym; ++s) {
            if (until_cp == 0) {
                ix->cps.push_back(make_checkpoint(p, hdr));
                until_cp = kDecodeS;
            }
            --until_cp;
            const size_t by = size_t(p >> 3);
            uint64_t v = 0;
            if (by + 8 <= bl) {
                for (int i = 7; i >= 0; --i) v = v << 8 | bs[by + size_t(i)];
            } else {
                for (size_t i = 0; i < 8 && by + i < bl; ++i) v |= uint64_t(bs[by + i]) << (8 * i);
            }
            v >>= (p & 7);  // 57 bits or more; a symbol has at most 17
            // neg, rev (StreamVersion > 0), hasHeader, header, index blocks (decoder.lpr:178-193),
            // branch-free: this loop is the decode's sequential chain
            int used = 1 + rev_bit;
            const int has = int((v >> used) & 1);
            const int nh = int((v >> (used + 1)) & 3);
            hdr = has ? nh : hdr;
            used += 1 + 2 * has;
            // the next four 3-bit blocks, first block most significant; the hdr + 1 leading ones are the index
            const uint32_t blk = uint32_t(v >> used);
            const uint32_t r4 = (blk & 7) << 9 | ((blk >> 3) & 7) << 6 | ((blk >> 6) & 7) << 3 | ((blk >> 9) & 7);
            const int idx = int(r4 >> (3 * (3 - hdr)));
            used += 3 * (hdr + 1);
            if (p + uint64_t(used) > avail) return walk_fail(err, k, "a symbol needs bits past the end of the stream");
            if (idx >= f.count)
                return walk_fail(err, k, "chunk index " + std::to_string(idx) + " >= ChunkCount " +
                                             std::to_string(f.count));
            p += uint64_t(used);
        }
        f.nbits = p;
        f.cp_count = ix->cps.size() - f.cp_first;
        // the stream ends on a 16-bit word boundary of its own (decoder.lpr:205-211)
        const uint64_t bs_bytes = (p + 15) / 16 * 2;
        if (bs_bytes > uint64_t(bl)) return walk_fail(err, k, "truncated bitstream (last word)");
        pos += size_t(bs_bytes);
        f.end_off = pos;
        ix->samples += int64_t(f.flen) * int64_t(f.cs);
        ix->symbols += f.nsym;
        ix->frames.push_back(f);
    }
    ix->len = len;
    return 0;
}

void index_table_write(const Index& ix, std::vector<uint8_t>* out) {
    const size_t F = ix.frames.size(), P = ix.cps.size();
    out->assign(kTableHeaderBytes + 16 * F + 8 * P, 0);
    uint8_t* t = out->data();
    std::memcpy(t, "GSCT", 4);
    wr32(t + 4, kTableVersion);
    wr32(t + 8, uint32_t(kDecodeS));
    wr32(t + 12, uint32_t(F));
    wr64(t + 16, uint64_t(ix.len));
    wr64(t + 24, uint64_t(P));
    uint8_t* q = t + kTableHeaderBytes;
    for (const IndexFrame& f : ix.frames) {
        wr64(q, uint64_t(f.off));
        wr64(q + 8, f.nbits);
        q += 16;
    }
    for (const uint64_t c : ix.cps) {
        wr64(q, c);
        q += 8;
    }
}

int index_from_table(const uint8_t* g, size_t len, const uint8_t* table, size_t tlen, Index* ix, std::string* err,
                     const ParallelRunner* par, bool expand) {
    *ix = Index();
    if (!g || len == 0) {
        if (err) *err = "gsc decode: empty stream";
        return -1;
    }
    if (!table || tlen < kTableHeaderBytes) return table_fail(err, "shorter than its 32-byte header");
    if (std::memcmp(table, "GSCT", 4) != 0) return table_fail(err, "bad magic");
    if (rd32(table + 4) != kTableVersion)
        return table_fail(err, "version " + std::to_string(rd32(table + 4)) + ", this library reads version " +
                                   std::to_string(kTableVersion));
    if (rd32(table + 8) != uint32_t(kDecodeS))
        return table_fail(err, "written with " + std::to_string(rd32(table + 8)) +
                                   " symbols per checkpoint, this library uses " + std::to_string(kDecodeS));
    const uint64_t F = rd32(table + 12), tl = rd64(table + 16), P = rd64(table + 24);
    if (tl != uint64_t(len))
        return table_fail(err, "made for a stream of " + std::to_string(tl) + " bytes, this one has " +
                                   std::to_string(len));
    const uint64_t body = uint64_t(tlen - kTableHeaderBytes);
    if (16 * F > body || P > (body - 16 * F) / 8 || kTableHeaderBytes + 16 * F + 8 * P != uint64_t(tlen))
        return table_fail(err, std::to_string(tlen) + " bytes, but " + std::to_string(F) + " frames and " +
                                   std::to_string(P) + " checkpoints need 32 + 16 F + 8 P");
    if (F == 0) return table_fail(err, "no frames");
    const uint8_t* tf = table + kTableHeaderBytes;
    const uint8_t* tc = tf + 16 * F;
    if (rd64(tf) != 0) return table_fail(err, "frame 0 is not at offset 0");
    ix->frames.resize(size_t(F));
    uint64_t cp = 0;
    size_t natt = 0, ncb = 0;
    for (size_t k = 0; k < size_t(F); ++k) {
        IndexFrame& f = ix->frames[k];
        const uint64_t off = rd64(tf + 16 * k), nbits = rd64(tf + 16 * k + 8);
        if (off >= uint64_t(len)) return walk_fail(err, k, "seek table: offset past the end of the stream");
        if (frame_head(g, len, size_t(off), k, k ? &ix->frames[0] : nullptr, &f, err) != 0) return -1;
        if (nbits > uint64_t(len - f.bs_off) * 8)
            return walk_fail(err, k, "seek table: more bits than the stream has left");
        if (f.nsym == 0 && nbits != 0) return walk_fail(err, k, "seek table: bits in a frame without symbols");
        f.nbits = nbits;
        const uint64_t end = uint64_t(f.bs_off) + (nbits + 15) / 16 * 2;
        const uint64_t next = k + 1 < size_t(F) ? rd64(tf + 16 * (k + 1)) : uint64_t(len);
        if (end != next)
            return walk_fail(err, k, "seek table: the bitstream ends at byte " + std::to_string(end) + ", " +
                                         (k + 1 < size_t(F) ? "the next frame is claimed at "
                                                            : "the stream has ") +
                                         std::to_string(next));
        f.end_off = size_t(end);
        const uint64_t ncp = (uint64_t(f.nsym) + uint64_t(kDecodeS) - 1) / uint64_t(kDecodeS);
        if (ncp > P - cp) return table_fail(err, "fewer checkpoints than the frames' symbols need");
        for (uint64_t i = 0; i < ncp; ++i) {
            const uint64_t c = rd64(tc + 8 * (cp + i));
            const char* bad = (c & 7) > 4                              ? "header state out of range"
                              : (c >> 3) > nbits                       ? "bit offset past the frame's bits"
                              : i == 0 && c != make_checkpoint(0, -1) ? "a frame's first checkpoint is not (0, -1)"
                                                                       : nullptr;
            if (bad)
                return walk_fail(err, k, "seek table: checkpoint " + std::to_string(i) + ": " + bad);
        }
        f.cp_first = size_t(cp);
        f.cp_count = size_t(ncp);
        cp += ncp;
        f.att_first = natt;
        f.cb_first = ncb;
        natt += size_t(f.count);
        ncb += codebook_slots(f);
        f.first_sample = ix->samples;
        ix->samples += int64_t(f.flen) * int64_t(f.cs);
        ix->symbols += f.nsym;
    }
    if (cp != P) return table_fail(err, "more checkpoints than the frames' symbols need");
    ix->channels = ix->frames[0].ch;
    ix->rate = ix->frames[0].rate;
    ix->len = len;
    ix->cps.resize(size_t(P));
    for (size_t i = 0; i < size_t(P); ++i) ix->cps[i] = rd64(tc + 8 * i);
    if (!expand) {
        ix->has_tables = false;
        return 0;
    }
    ix->att.resize(natt);
    ix->codebook.assign(ncb, 0);
    auto tables = [&](int k) {
        const IndexFrame& f = ix->frames[size_t(k)];
        frame_tables_expand(g, f, ix->att.data() + f.att_first, ix->codebook.data() + f.cb_first);
    };
    if (par && F > 1 && F < (uint64_t(1) << 31)) {
        (*par)(int(F), tables);
    } else {
        for (size_t k = 0; k < size_t(F); ++k) tables(int(k));
    }
    return 0;
}

void index_expand_tables(const uint8_t* g, Index* ix) {
    if (ix->has_tables) return;
    size_t natt = 0, ncb = 0;
    for (const IndexFrame& f : ix->frames) {
        natt = std::max(natt, f.att_first + size_t(f.count));
        ncb = std::max(ncb, f.cb_first + codebook_slots(f));
    }
    ix->att.assign(natt, 0);
    ix->codebook.assign(ncb, 0);
    for (const IndexFrame& f : ix->frames)
        frame_tables_expand(g, f, ix->att.data() + f.att_first, ix->codebook.data() + f.cb_first);
    ix->has_tables = true;
}

void index_drop_tables(Index* ix) {
    std::vector<int16_t>().swap(ix->codebook);
    std::vector<uint8_t>().swap(ix->att);
    ix->has_tables = false;
}

int index_table_split(const uint8_t* g, size_t len, const uint8_t* table, size_t tlen, const size_t* part_bytes,
                      int nparts, std::vector<std::vector<uint8_t>>* out, std::string* err) {
    out->assign(size_t(std::max(nparts, 0)), std::vector<uint8_t>());
    if (!g || !table || tlen < kTableHeaderBytes || std::memcmp(table, "GSCT", 4) != 0)
        return table_fail(err, "shorter than its 32-byte header, or bad magic");
    if (rd32(table + 4) != kTableVersion || rd32(table + 8) != uint32_t(kDecodeS))
        return table_fail(err, "version " + std::to_string(rd32(table + 4)) + " with " + std::to_string(rd32(table + 8)) +
                                   " symbols per checkpoint, this library writes version " +
                                   std::to_string(kTableVersion) + " with " + std::to_string(kDecodeS));
    const uint64_t F = rd32(table + 12), P = rd64(table + 24), body = uint64_t(tlen - kTableHeaderBytes);
    if (16 * F > body || P > (body - 16 * F) / 8 || kTableHeaderBytes + 16 * F + 8 * P != uint64_t(tlen) ||
        rd64(table + 16) != uint64_t(len))
        return table_fail(err, "not the table of these " + std::to_string(len) + " bytes");
    const uint8_t* tf = table + kTableHeaderBytes;
    const uint8_t* tc = tf + 16 * F;
    // the files of a batch may differ in ChannelCount and SampleRate: every frame is read on its own
    uint64_t k = 0, cp = 0, start = 0;
    for (int p = 0; p < nparts; ++p) {
        const uint64_t end = start + uint64_t(part_bytes[p]);
        if (end < start || end > uint64_t(len)) return table_fail(err, "the pieces are longer than the stream");
        Index part;
        for (; k < F && rd64(tf + 16 * k) < end; ++k) {
            const uint64_t off = rd64(tf + 16 * k), next = k + 1 < F ? rd64(tf + 16 * (k + 1)) : uint64_t(len);
            if (off < start || next > end || next < off) return table_fail(err, "a frame lies across two pieces");
            IndexFrame f;
            if (frame_head(g, len, size_t(off), size_t(k), nullptr, &f, err) != 0) return -1;
            const uint64_t ncp = (uint64_t(f.nsym) + uint64_t(kDecodeS) - 1) / uint64_t(kDecodeS);
            if (ncp > P - cp) return table_fail(err, "fewer checkpoints than the frames' symbols need");
            IndexFrame q;
            q.off = size_t(off - start);
            q.nbits = rd64(tf + 16 * k + 8);
            part.frames.push_back(q);
            for (uint64_t i = 0; i < ncp; ++i) part.cps.push_back(rd64(tc + 8 * (cp + i)));
            cp += ncp;
        }
        part.len = part_bytes[p];
        if (!part.frames.empty()) index_table_write(part, &(*out)[size_t(p)]);
        start = end;
    }
    if (start != uint64_t(len) || k != F || cp != P) return table_fail(err, "the pieces do not cover the stream");
    return 0;
}

std::string verify_message(const Index& ix, unsigned long long status) {
    const uint64_t c = status >> 8;
    const int reason = int(status & 0xff);
    // the last frame whose first checkpoint is <= c and that owns checkpoints
    size_t k = 0;
    for (size_t lo = 0, hi = ix.frames.size(); lo < hi;) {
        const size_t mid = (lo + hi) / 2;
        if (uint64_t(ix.frames[mid].cp_first) <= c) {
            k = mid;
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    const uint64_t seg = c - uint64_t(ix.frames.empty() ? 0 : ix.frames[k].cp_first);
    const char* what = reason == kVerifyIndex    ? "a chunk index >= ChunkCount in its segment"
                       : reason == kVerifyBit    ? "its segment ends at another bit offset than the table claims"
                       : reason == kVerifyHeader ? "its segment ends in another header state than the table claims"
                                                 : "its segment lies outside the uploaded stream";
    return "gsc decode: frame " + std::to_string(k) + ": seek table: checkpoint " + std::to_string(seg) + ": " + what;
}

int index_locate(const Index& ix, int64_t sample, int* frame, int64_t* row, int* within, int64_t* checkpoint,
                 std::string* err) {
    if (sample < 0 || sample >= ix.samples) {
        if (err)
            *err = "gsc locate: sample " + std::to_string(sample) + " outside [0, " + std::to_string(ix.samples) + ")";
        return -1;
    }
    // the last frame whose first sample is <= sample: of a run of frames that
    // start at the same sample, all but the last are empty
    size_t lo = 0, hi = ix.frames.size() - 1;
    while (lo < hi) {
        const size_t mid = (lo + hi + 1) / 2;
        if (ix.frames[mid].first_sample <= sample) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    const IndexFrame& f = ix.frames[lo];
    const int64_t local = sample - f.first_sample;
    const int64_t r = local / f.cs;
    if (frame) *frame = int(lo);
    if (row) *row = r;
    if (within) *within = int(local - r * f.cs);
    if (checkpoint) *checkpoint = int64_t(f.cp_first) + r * f.ch / kDecodeS;
    return 0;
}

}  // namespace gsc
