// .gsc decoder, the host index (decoder/decoder.lpr:37-220):
// the sequential walk, the sample locator and the crop planner.  Plain C++,
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
// at or before a sample and plan_crops lays out what a batch of ranges has to
// unpack (gsc_decode_crops.hip).
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

}  // namespace

int decode_walk(const uint8_t* g, size_t len, Index* ix, std::string* err) {
    *ix = Index();
    if (!g || len == 0) {
        if (err) *err = "gsc decode: empty stream";
        return -1;
    }
    // CAttrMul (decoder.lpr:6)
    const double attr_mul = double(fpc_round(32768.0 * (32767.0 / 2047.0)));
    size_t pos = 0;
    while (pos < len) {
        const size_t k = ix->frames.size();
        IndexFrame f;
        f.off = pos;
        if (len - pos < 12) return walk_fail(err, k, "truncated header");
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
        if (k == 0) {
            ix->channels = f.ch;
            ix->rate = f.rate;
        } else if (f.ch != ix->channels || f.rate != ix->rate) {
            return walk_fail(err, k, "ChannelCount / SampleRate differ from frame 0");
        }
        // CAttrLookup (decoder.lpr:88-96)
        {
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
        f.att_first = ix->att.size();
        ix->att.resize(f.att_first + count);
        {
            uint8_t* a = ix->att.data() + f.att_first;
            for (size_t i = 0; i < count / 2; ++i) {
                const uint8_t b = g[pos + i];
                a[2 * i] = b >> 4;
                a[2 * i + 1] = b & 0x0f;
            }
            if (count & 1) a[count - 1] = g[pos + count / 2] >> 4;
        }
        pos += att_bytes;
        if (len - pos < cb_bytes) return walk_fail(err, k, "truncated codebook");
        f.cb_off = pos;
        f.cb_first = ix->codebook.size();
        ix->codebook.resize(f.cb_first + ((count * cs + 7) & ~size_t(7)), 0);
        {
            int16_t* c = ix->codebook.data() + f.cb_first;
            const uint8_t* p = g + pos;
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
        pos += cb_bytes;
        if (len - pos < 4) return walk_fail(err, k, "truncated FrameLength");
        f.flen = rd32(g + pos);
        pos += 4;
        f.bs_off = pos;
        const uint8_t* bs = g + pos;
        const size_t bl = len - pos;
        const uint64_t avail = uint64_t(bl) * 8;
        const uint64_t nsym = uint64_t(f.flen) * uint64_t(f.ch);
        // a symbol has at least 2 bits: refuse before sizing anything by FrameLength
        if (nsym > avail / 2) return walk_fail(err, k, "FrameLength needs bits past the end of the stream");
        f.nsym = int64_t(nsym);
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

int plan_crops(const Index* const* ixs, int nstreams, const Crop* crops, int ncrops, int64_t length, CropPlan* plan,
               std::string* err) {
    *plan = CropPlan();
    auto refuse = [&](int i, const std::string& what) {
        if (err) *err = "gsc crops: crop " + std::to_string(i) + ": " + what;
        return -1;
    };
    if (!ixs || nstreams <= 0 || ncrops < 0 || (ncrops > 0 && !crops) || length < 0) {
        if (err) *err = "gsc crops: invalid argument";
        return -1;
    }
    for (int s = 0; s < nstreams; ++s) {
        if (!ixs[s]) {
            if (err) *err = "gsc crops: stream " + std::to_string(s) + " is null";
            return -1;
        }
        if (ixs[s]->channels != ixs[0]->channels) {
            if (err)
                *err = "gsc crops: stream " + std::to_string(s) + " has " + std::to_string(ixs[s]->channels) +
                       " channels, stream 0 has " + std::to_string(ixs[0]->channels);
            return -1;
        }
    }
    plan->channels = ixs[0]->channels;
    plan->crops.reserve(size_t(ncrops));
    for (int i = 0; i < ncrops; ++i) {
        const Crop& c = crops[i];
        if (c.stream < 0 || c.stream >= nstreams) return refuse(i, "stream index " + std::to_string(c.stream));
        const Index& ix = *ixs[c.stream];
        if (c.begin < 0 || c.begin > ix.samples)
            return refuse(i, "begin " + std::to_string(c.begin) + " outside [0, " + std::to_string(ix.samples) + "]");
        if (c.count < 0 || c.count > length)
            return refuse(i, "count " + std::to_string(c.count) + " outside [0, length " + std::to_string(length) + "]");
        PlanCrop pc{c.stream, c.begin, std::min<int64_t>(c.count, ix.samples - c.begin), 0, 0, int(plan->pieces.size())};
        if (pc.count > 0) {
            int fa = 0, fb = 0;
            int64_t ra = 0, rb = 0;
            if (index_locate(ix, pc.begin, &fa, &ra, nullptr, nullptr, err) != 0 ||
                index_locate(ix, pc.begin + pc.count - 1, &fb, &rb, nullptr, nullptr, err) != 0)
                return -1;
            pc.f0 = fa;
            pc.f1 = fb + 1;
            for (int fi = fa; fi <= fb; ++fi) {
                const IndexFrame& f = ix.frames[size_t(fi)];
                CropPiece p{plan->slots, 0, 0, i, fi, 0};
                if (f.nsym > 0) {
                    // symbol rows [r0, r1] of this frame, whole checkpoint segments around them
                    const int64_t r0 = fi == fa ? ra : 0, r1 = fi == fb ? rb : int64_t(f.flen) - 1;
                    p.seg0 = r0 * f.ch / kDecodeS;
                    p.nseg = int32_t(((r1 + 1) * f.ch - 1) / kDecodeS - p.seg0 + 1);
                }
                plan->slots += p.nseg;
                plan->pieces.push_back(p);
            }
        }
        plan->crops.push_back(pc);
    }
    if (plan->pieces.size() >= (size_t(1) << 31) || plan->slots >= (int64_t(1) << 40)) {
        if (err) *err = "gsc crops: too many frames or symbols for one call";
        return -1;
    }
    return 0;
}

}  // namespace gsc
