// .gsc decoder, host side (decoder/decoder.lpr:37-220).
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
// A resident stream (gsc_stream_open) keeps the walk's result and the bytes
// on the device; gsc_decode_crops then decodes batches of sample ranges from
// the checkpoints at or before them (index_locate, plan_crops here;
// gsc_decode_crops.hip) into caller-owned device memory.
//
// GSC_DECODE_WALK_ONLY builds the walk, the sample locator and the crop
// planner alone (no HIP), for host-side checks.
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

#ifndef GSC_DECODE_WALK_ONLY
// ============================================================================
// device decode + C ABI
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>

#include "../../include/soundchunks.h"
#include "gsc_device.h"

extern "C" hipError_t gsc_launch_decode_unpack(const gsc::DecFrame* frames, int nframes, const uint64_t* cps,
                                               int64_t ncp, const uint32_t* words, int64_t nwords, uint16_t* sym,
                                               int64_t nsym, hipStream_t st);
extern "C" hipError_t gsc_launch_decode_synth(const gsc::DecFrame* frames, int nframes, const gsc::DecJob* jobs,
                                              int njobs, int lds_bytes, const uint16_t* sym, int64_t nsym,
                                              const int16_t* cb, int64_t ncb, const uint8_t* att, int64_t natt,
                                              int16_t* out, int64_t nout, hipStream_t st);

extern "C" hipError_t gsc_launch_crop_unpack(const gsc::CropJob* jobs, int ncrops, const gsc::CropPiece* pieces,
                                             int npieces, uint16_t* sym, int64_t nslots, hipStream_t st);
extern "C" hipError_t gsc_launch_crop_synth(const gsc::CropJob* jobs, int ncrops, const gsc::CropPiece* pieces,
                                            int npieces, const uint16_t* sym, int64_t nslots, int64_t length,
                                            int channels, int is_float, int planar, int lds_bytes, int tile_len,
                                            void* out, hipStream_t st);
extern "C" hipError_t gsc_launch_crop_fused(const gsc::CropJob* jobs, int ncrops, int64_t length, int channels,
                                            int is_float, int planar, int tile_len, void* out, hipStream_t st);

struct gsc_index {
    gsc::Index ix;
};

// A stream resident on one device: the index, and on the device the byte slab
// (whole words, zero tail), every checkpoint, the int16 codebooks, the
// attenuations and the frame table, until gsc_stream_free.
struct gsc_stream {
    gsc_index idx;
    int device = 0;
    int lds_bytes = 0;  // the largest staged codebook + attenuations of a frame
    uint8_t* d_bytes = nullptr;
    uint8_t* d_att = nullptr;
    uint64_t* d_cps = nullptr;
    int16_t* d_cb = nullptr;
    gsc::ResFrame* d_frames = nullptr;
    int64_t nwords = 0, ncp = 0, ncb = 0, natt = 0;
};

namespace gsc {

int set_last_error(const std::string& m);
int require_device();

namespace {

thread_local gsc_decode_timing t_dtim;
// crop decode: 0 unpack, then synthesis with the codebook from global memory; 1 the same with the codebook
// staged in LDS; 2 unpack and synthesis fused in one launch (DESIGN.md "f5 decoder" has the A/B)
thread_local int t_crop_variant = 2;

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

#define DEC_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <typename T>
struct Dev {
    T* p = nullptr;
    ~Dev() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * std::max<size_t>(n, 1)); }
};

struct Event {
    hipEvent_t e = nullptr;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
};

// frames [b, e) of one stream
struct Part {
    const uint8_t* g;
    const Index* ix;
    int b, e;
};

void clamp_range(const Index& ix, int* b, int* e) {
    const int n = int(ix.frames.size());
    *b = std::max(*b, 0);
    *e = *e < 0 ? n : std::min(*e, n);
    if (*e < *b) *e = *b;
}

// Every frame of every part in one launch per stage.  *pcm: the parts' samples
// back to back (malloc), part_values[i] int16 values each.
int decode_parts(const std::vector<Part>& parts, int16_t** pcm, size_t* pcm_len, size_t* part_values,
                 gsc_decode_timing* tim) {
    const double t_begin = now_ms();
    std::vector<DecFrame> frames;
    std::vector<DecJob> jobs;
    struct Span {
        size_t byte0, bytes, byte_base, cp0, cps, cp_base, cb0, cbs, cb_base, att0, atts, att_base;
    };
    std::vector<Span> spans(parts.size());
    size_t nbytes = 0, ncp = 0, ncb = 0, natt = 0;
    int64_t nsym = 0, nout = 0;
    int lds_bytes = 0;
    for (size_t pi = 0; pi < parts.size(); ++pi) {
        const Part& pt = parts[pi];
        Span& sp = spans[pi];
        sp = Span{};
        const int64_t out_before = nout;
        if (pt.b < pt.e) {
            const IndexFrame& fb = pt.ix->frames[size_t(pt.b)];
            const IndexFrame& fe = pt.ix->frames[size_t(pt.e) - 1];
            sp.byte0 = fb.off;
            sp.bytes = fe.end_off - fb.off;
            sp.byte_base = nbytes;
            sp.cp0 = fb.cp_first;
            sp.cps = fe.cp_first + fe.cp_count - fb.cp_first;
            sp.cp_base = ncp;
            sp.cb0 = fb.cb_first;
            sp.cbs = fe.cb_first + ((size_t(fe.count) * size_t(fe.cs) + 7) & ~size_t(7)) - fb.cb_first;
            sp.cb_base = ncb;  // a multiple of 8, as every cb_first
            sp.att0 = fb.att_first;
            sp.atts = fe.att_first + size_t(fe.count) - fb.att_first;
            sp.att_base = natt;
            nbytes += sp.bytes;
            ncp += sp.cps;
            ncb += sp.cbs;
            natt += sp.atts;
        }
        for (int i = pt.b; i < pt.e; ++i) {
            const IndexFrame& f = pt.ix->frames[size_t(i)];
            DecFrame d{};
            d.bs_off = int64_t(sp.byte_base + (f.bs_off - sp.byte0));
            d.sym_off = nsym;
            d.out_off = nout;
            d.cb_off = int64_t(sp.cb_base + (f.cb_first - sp.cb0));
            d.att_off = int64_t(sp.att_base + (f.att_first - sp.att0));
            d.nsym = f.nsym;
            d.cp_first = int32_t(sp.cp_base + (f.cp_first - sp.cp0));
            d.ver = f.ver;
            d.ch = f.ch;
            d.cs = f.cs;
            d.count = f.count;
            std::memcpy(d.lut, f.lut, sizeof(d.lut));
            const int64_t row = int64_t(f.cs) * f.ch;  // int16 values per symbol row
            const int64_t cbn = int64_t(f.count) * f.cs;
            if (f.flen > 0) {
                const int64_t need = ((cbn * 2 + 3) & ~int64_t(3)) + f.count;
                if (need <= kDecodeLdsBytes) lds_bytes = std::max(lds_bytes, int(need));
                // a workgroup stages the codebook once: give it at least 4 codebooks' worth of output
                const int64_t target = std::min<int64_t>(std::max<int64_t>(4 * cbn, 64 * 1024), int64_t(1) << 30);
                const int64_t rows_per = std::max<int64_t>(1, target / row);
                for (int64_t r = 0; r < int64_t(f.flen); r += rows_per)
                    jobs.push_back(DecJob{r, int32_t(std::min<int64_t>(rows_per, int64_t(f.flen) - r)),
                                          int32_t(frames.size())});
            }
            nsym += f.nsym;
            nout += int64_t(f.flen) * row;
            frames.push_back(d);
        }
        if (part_values) part_values[pi] = size_t(nout - out_before);
    }
    if (ncp >= (size_t(1) << 31) || frames.size() >= (size_t(1) << 31) || jobs.size() >= (size_t(1) << 31))
        return set_last_error("gsc decode: stream too large for one call");
    int16_t* host_out = static_cast<int16_t*>(std::malloc(std::max<size_t>(size_t(nout) * 2, 2)));
    if (!host_out) return set_last_error("gsc decode: out of memory");
    struct FreeOnFail {
        int16_t* p;
        ~FreeOnFail() { std::free(p); }
    } guard{host_out};
    tim->frames = int(frames.size());
    tim->symbols = nsym;
    tim->samples = nout;
    if (nout > 0) {
        if (require_device() != 0) return -1;
        const size_t byte_alloc = ((nbytes + 3) & ~size_t(3)) + 16;  // whole words, zero tail
        Dev<uint8_t> d_bytes, d_att;
        Dev<DecFrame> d_frames;
        Dev<DecJob> d_jobs;
        Dev<uint64_t> d_cps;
        Dev<int16_t> d_cb, d_out;
        Dev<uint16_t> d_sym;
        Event e0, e1, e2;
        const double t0 = now_ms();
        DEC_TRY(d_bytes.alloc(byte_alloc));
        DEC_TRY(d_att.alloc(natt + 1));
        DEC_TRY(d_frames.alloc(frames.size()));
        DEC_TRY(d_jobs.alloc(jobs.size()));
        DEC_TRY(d_cps.alloc(ncp));
        DEC_TRY(d_cb.alloc(ncb + 16));
        DEC_TRY(d_out.alloc(size_t(nout)));
        DEC_TRY(d_sym.alloc(size_t(nsym)));
        DEC_TRY(hipEventCreate(&e0.e));
        DEC_TRY(hipEventCreate(&e1.e));
        DEC_TRY(hipEventCreate(&e2.e));
        DEC_TRY(hipMemset(d_bytes.p + (nbytes & ~size_t(3)), 0, byte_alloc - (nbytes & ~size_t(3))));
        DEC_TRY(hipMemset(d_cb.p + ncb, 0, 16 * sizeof(int16_t)));
        DEC_TRY(hipMemset(d_att.p + natt, 0, 1));
        for (size_t pi = 0; pi < parts.size(); ++pi) {
            const Span& sp = spans[pi];
            const Index& ix = *parts[pi].ix;
            if (sp.bytes)
                DEC_TRY(hipMemcpy(d_bytes.p + sp.byte_base, parts[pi].g + sp.byte0, sp.bytes, hipMemcpyHostToDevice));
            if (sp.cps)
                DEC_TRY(hipMemcpy(d_cps.p + sp.cp_base, ix.cps.data() + sp.cp0, sp.cps * sizeof(uint64_t),
                                  hipMemcpyHostToDevice));
            if (sp.cbs)
                DEC_TRY(hipMemcpy(d_cb.p + sp.cb_base, ix.codebook.data() + sp.cb0, sp.cbs * sizeof(int16_t),
                                  hipMemcpyHostToDevice));
            if (sp.atts)
                DEC_TRY(hipMemcpy(d_att.p + sp.att_base, ix.att.data() + sp.att0, sp.atts, hipMemcpyHostToDevice));
        }
        DEC_TRY(hipMemcpy(d_frames.p, frames.data(), frames.size() * sizeof(DecFrame), hipMemcpyHostToDevice));
        DEC_TRY(hipMemcpy(d_jobs.p, jobs.data(), jobs.size() * sizeof(DecJob), hipMemcpyHostToDevice));
        DEC_TRY(hipDeviceSynchronize());
        tim->h2d_bytes = (long long)(nbytes + ncp * sizeof(uint64_t) + ncb * sizeof(int16_t) + natt +
                                     frames.size() * sizeof(DecFrame) + jobs.size() * sizeof(DecJob));
        const double t1 = now_ms();
        DEC_TRY(hipEventRecord(e0.e, nullptr));
        DEC_TRY(gsc_launch_decode_unpack(d_frames.p, int(frames.size()), d_cps.p, int64_t(ncp),
                                         reinterpret_cast<const uint32_t*>(d_bytes.p), int64_t(byte_alloc / 4),
                                         d_sym.p, nsym, nullptr));
        DEC_TRY(hipEventRecord(e1.e, nullptr));
        DEC_TRY(gsc_launch_decode_synth(d_frames.p, int(frames.size()), d_jobs.p, int(jobs.size()), lds_bytes, d_sym.p,
                                        nsym, d_cb.p, int64_t(ncb + 16), d_att.p, int64_t(natt + 1), d_out.p, nout,
                                        nullptr));
        DEC_TRY(hipEventRecord(e2.e, nullptr));
        DEC_TRY(hipEventSynchronize(e2.e));
        float ms_u = 0, ms_s = 0;
        DEC_TRY(hipEventElapsedTime(&ms_u, e0.e, e1.e));
        DEC_TRY(hipEventElapsedTime(&ms_s, e1.e, e2.e));
        const double t2 = now_ms();
        DEC_TRY(hipMemcpy(host_out, d_out.p, size_t(nout) * 2, hipMemcpyDeviceToHost));
        tim->h2d_ms = t1 - t0;
        tim->gpu_unpack_ms = ms_u;
        tim->gpu_synth_ms = ms_s;
        tim->d2h_ms = now_ms() - t2;
    }
    guard.p = nullptr;
    *pcm = host_out;
    *pcm_len = size_t(nout);
    tim->total_ms += now_ms() - t_begin;
    return 0;
}

}  // namespace
}  // namespace gsc

using namespace gsc;

extern "C" {

gsc_index* gsc_index_create(const uint8_t* gsc, size_t len) {
    gsc_index* h = new gsc_index();
    std::string err;
    if (decode_walk(gsc, len, &h->ix, &err) != 0) {
        delete h;
        set_last_error(err);
        return nullptr;
    }
    return h;
}

int gsc_index_frame_count(const gsc_index* ix) { return ix ? int(ix->ix.frames.size()) : set_last_error("null index"); }

int gsc_index_info(const gsc_index* ix, int* channels, int* sample_rate, long long* samples_per_channel) {
    if (!ix) return set_last_error("null index");
    if (channels) *channels = ix->ix.channels;
    if (sample_rate) *sample_rate = ix->ix.rate;
    if (samples_per_channel) *samples_per_channel = ix->ix.samples;
    return 0;
}

int gsc_index_frames(const gsc_index* ix, size_t* byte_offset, int* frame_length, int* chunk_size, int* chunk_count,
                     long long* first_sample) {
    if (!ix) return set_last_error("null index");
    const auto& fr = ix->ix.frames;
    for (size_t i = 0; i < fr.size(); ++i) {
        if (byte_offset) byte_offset[i] = fr[i].off;
        if (frame_length) frame_length[i] = int(fr[i].flen);
        if (chunk_size) chunk_size[i] = fr[i].cs;
        if (chunk_count) chunk_count[i] = fr[i].count;
        if (first_sample) first_sample[i] = fr[i].first_sample;
    }
    if (byte_offset) byte_offset[fr.size()] = ix->ix.len;
    if (first_sample) first_sample[fr.size()] = ix->ix.samples;
    return 0;
}

void gsc_index_free(gsc_index* ix) { delete ix; }

int gsc_decode_checkpoint_symbols(void) { return kDecodeS; }

int gsc_decode_indexed(const uint8_t* gsc, size_t len, const gsc_index* ix, int frame_begin, int frame_end,
                       int16_t** pcm, size_t* pcm_len) {
    if (!gsc || !ix || !pcm || !pcm_len) return set_last_error("gsc_decode_indexed: invalid argument");
    if (len != ix->ix.len) return set_last_error("gsc_decode_indexed: the index was built from another stream");
    t_dtim = gsc_decode_timing{};
    Part pt{gsc, &ix->ix, frame_begin, frame_end};
    clamp_range(ix->ix, &pt.b, &pt.e);
    return decode_parts({pt}, pcm, pcm_len, nullptr, &t_dtim);
}

int gsc_decode(const uint8_t* gsc, size_t len, int16_t** pcm, size_t* pcm_len, int* channels, int* sample_rate) {
    if (!pcm || !pcm_len) return set_last_error("gsc_decode: invalid argument");
    t_dtim = gsc_decode_timing{};
    const double t0 = now_ms();
    Index ix;
    std::string err;
    if (decode_walk(gsc, len, &ix, &err) != 0) return set_last_error(err);
    t_dtim.host_index_ms = now_ms() - t0;
    t_dtim.total_ms = t_dtim.host_index_ms;
    if (channels) *channels = ix.channels;
    if (sample_rate) *sample_rate = ix.rate;
    return decode_parts({Part{gsc, &ix, 0, int(ix.frames.size())}}, pcm, pcm_len, nullptr, &t_dtim);
}

int gsc_decode_many(const uint8_t* const* gscs, const size_t* lens, int file_count, int16_t** pcm,
                    size_t* file_samples, int* channels, int* sample_rate) {
    if (!gscs || !lens || file_count <= 0 || !pcm || !file_samples)
        return set_last_error("gsc_decode_many: invalid argument");
    t_dtim = gsc_decode_timing{};
    const double t0 = now_ms();
    std::vector<Index> ixs(static_cast<size_t>(file_count));
    std::vector<Part> parts;
    for (int i = 0; i < file_count; ++i) {
        std::string err;
        if (decode_walk(gscs[i], lens[i], &ixs[size_t(i)], &err) != 0)
            return set_last_error("file " + std::to_string(i) + ": " + err);
        if (ixs[size_t(i)].channels != ixs[0].channels || ixs[size_t(i)].rate != ixs[0].rate)
            return set_last_error("gsc_decode_many: file " + std::to_string(i) +
                                  " differs from file 0 in ChannelCount / SampleRate");
        parts.push_back(Part{gscs[i], &ixs[size_t(i)], 0, int(ixs[size_t(i)].frames.size())});
    }
    t_dtim.host_index_ms = now_ms() - t0;
    t_dtim.total_ms = t_dtim.host_index_ms;
    if (channels) *channels = ixs[0].channels;
    if (sample_rate) *sample_rate = ixs[0].rate;
    size_t total = 0;
    return decode_parts(parts, pcm, &total, file_samples, &t_dtim);
}

void gsc_last_decode_timing(gsc_decode_timing* t) {
    if (t) *t = t_dtim;
}

int gsc_index_locate(const gsc_index* ix, long long sample, int* frame, long long* row, int* within,
                     long long* checkpoint) {
    if (!ix) return set_last_error("null index");
    std::string err;
    int64_t r = 0, c = 0;
    if (index_locate(ix->ix, sample, frame, &r, within, &c, &err) != 0) return set_last_error(err);
    if (row) *row = r;
    if (checkpoint) *checkpoint = c;
    return 0;
}

void gsc_stream_free(gsc_stream* st) {
    if (!st) return;
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != st->device;
    if (sw) (void)hipSetDevice(st->device);
    (void)hipDeviceSynchronize();  // queued crop decodes still read the slabs
    (void)hipFree(st->d_bytes);
    (void)hipFree(st->d_att);
    (void)hipFree(st->d_cps);
    (void)hipFree(st->d_cb);
    (void)hipFree(st->d_frames);
    if (sw) (void)hipSetDevice(cur);
    delete st;
}

#define STREAM_TRY(expr)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_));             \
            gsc_stream_free(h);                                                            \
            return nullptr;                                                                \
        }                                                                                  \
    } while (0)

gsc_stream* gsc_stream_open(const uint8_t* gsc, size_t len) {
    t_dtim = gsc_decode_timing{};
    const double t0 = now_ms();
    gsc_stream* h = new gsc_stream();
    std::string err;
    if (decode_walk(gsc, len, &h->idx.ix, &err) != 0) {
        delete h;
        set_last_error(err);
        return nullptr;
    }
    const Index& ix = h->idx.ix;
    t_dtim.host_index_ms = now_ms() - t0;
    if (require_device() != 0) {
        delete h;
        return nullptr;
    }
    STREAM_TRY(hipGetDevice(&h->device));
    std::vector<ResFrame> frames(ix.frames.size());
    for (size_t i = 0; i < frames.size(); ++i) {
        const IndexFrame& f = ix.frames[i];
        ResFrame& d = frames[i];
        d = ResFrame{};
        d.bs_off = int64_t(f.bs_off);
        d.cb_off = int64_t(f.cb_first);
        d.att_off = int64_t(f.att_first);
        d.nsym = f.nsym;
        d.first_sample = f.first_sample;
        d.cp_first = int64_t(f.cp_first);
        d.ver = f.ver;
        d.ch = f.ch;
        d.cs = f.cs;
        d.count = f.count;
        std::memcpy(d.lut, f.lut, sizeof(d.lut));
        const int64_t need = ((int64_t(f.count) * f.cs * 2 + 3) & ~int64_t(3)) + f.count;
        if (f.flen > 0 && need <= kDecodeLdsBytes) h->lds_bytes = std::max(h->lds_bytes, int(need));
    }
    const double t1 = now_ms();
    const size_t byte_alloc = ((len + 3) & ~size_t(3)) + 16;  // whole words, zero tail
    h->nwords = int64_t(byte_alloc / 4);
    h->ncp = int64_t(ix.cps.size());
    h->ncb = int64_t(ix.codebook.size() + 16);
    h->natt = int64_t(ix.att.size() + 1);
    STREAM_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_bytes), byte_alloc));
    STREAM_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_att), size_t(h->natt)));
    STREAM_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_cps), std::max<size_t>(ix.cps.size(), 1) * sizeof(uint64_t)));
    STREAM_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_cb), size_t(h->ncb) * sizeof(int16_t)));
    STREAM_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_frames), std::max<size_t>(frames.size(), 1) * sizeof(ResFrame)));
    STREAM_TRY(hipMemset(h->d_bytes + (len & ~size_t(3)), 0, byte_alloc - (len & ~size_t(3))));
    STREAM_TRY(hipMemset(h->d_cb + ix.codebook.size(), 0, 16 * sizeof(int16_t)));
    STREAM_TRY(hipMemset(h->d_att + ix.att.size(), 0, 1));
    STREAM_TRY(hipMemcpy(h->d_bytes, gsc, len, hipMemcpyHostToDevice));
    if (!ix.cps.empty())
        STREAM_TRY(hipMemcpy(h->d_cps, ix.cps.data(), ix.cps.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (!ix.codebook.empty())
        STREAM_TRY(hipMemcpy(h->d_cb, ix.codebook.data(), ix.codebook.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    if (!ix.att.empty()) STREAM_TRY(hipMemcpy(h->d_att, ix.att.data(), ix.att.size(), hipMemcpyHostToDevice));
    STREAM_TRY(hipMemcpy(h->d_frames, frames.data(), frames.size() * sizeof(ResFrame), hipMemcpyHostToDevice));
    STREAM_TRY(hipDeviceSynchronize());
    t_dtim.h2d_ms = now_ms() - t1;
    t_dtim.h2d_bytes = (long long)(len + ix.cps.size() * sizeof(uint64_t) + ix.codebook.size() * sizeof(int16_t) +
                                   ix.att.size() + frames.size() * sizeof(ResFrame));
    t_dtim.frames = int(frames.size());
    t_dtim.total_ms = now_ms() - t0;
    return h;
}

int gsc_stream_info(const gsc_stream* st, int* channels, int* sample_rate, long long* samples_per_channel,
                    int* frames) {
    if (!st) return set_last_error("null stream");
    if (channels) *channels = st->idx.ix.channels;
    if (sample_rate) *sample_rate = st->idx.ix.rate;
    if (samples_per_channel) *samples_per_channel = st->idx.ix.samples;
    if (frames) *frames = int(st->idx.ix.frames.size());
    return 0;
}

const gsc_index* gsc_stream_index(const gsc_stream* st) {
    if (!st) {
        set_last_error("null stream");
        return nullptr;
    }
    return &st->idx;
}

int gsc_stream_device(const gsc_stream* st) { return st ? st->device : set_last_error("null stream"); }

int gsc_decode_crops_variant(int variant) {
    const int prev = t_crop_variant;
    if (variant >= 0 && variant <= 2) t_crop_variant = variant;
    return prev;
}

int gsc_decode_crops(gsc_stream* const* streams, int nstreams, const gsc_crop* crops, int ncrops, int dtype,
                     int layout, long long length, void* dst_device, void* hip_stream, long long* written) {
    const double t_begin = now_ms();
    t_dtim = gsc_decode_timing{};
    if (!streams || nstreams <= 0) return set_last_error("gsc_decode_crops: no streams");
    if (dtype != GSC_PCM_INT16 && dtype != GSC_PCM_FLOAT32) return set_last_error("gsc_decode_crops: unknown dtype");
    if (layout != GSC_LAYOUT_TC && layout != GSC_LAYOUT_CT) return set_last_error("gsc_decode_crops: unknown layout");
    if (!dst_device) return set_last_error("gsc_decode_crops: dst_device is null");
    std::vector<const Index*> ixs(static_cast<size_t>(nstreams), nullptr);
    for (int s = 0; s < nstreams; ++s) {
        if (!streams[s]) return set_last_error("gsc_decode_crops: stream " + std::to_string(s) + " is null");
        ixs[size_t(s)] = &streams[s]->idx.ix;
    }
    std::vector<Crop> cr(static_cast<size_t>(std::max(ncrops, 0)));
    if (ncrops > 0 && !crops) return set_last_error("gsc_decode_crops: crops is null");
    for (int i = 0; i < ncrops; ++i) cr[size_t(i)] = Crop{crops[i].stream, crops[i].begin, crops[i].count};
    CropPlan plan;
    std::string err;
    if (plan_crops(ixs.data(), nstreams, cr.data(), ncrops, length, &plan, &err) != 0) return set_last_error(err);
    if (require_device() != 0) return -1;
    int dev = 0;
    DEC_TRY(hipGetDevice(&dev));
    for (int s = 0; s < nstreams; ++s)
        if (streams[s]->device != dev)
            return set_last_error("gsc_decode_crops: stream " + std::to_string(s) + " lives on device " +
                                  std::to_string(streams[s]->device) + ", the calling thread is bound to device " +
                                  std::to_string(dev));
    auto report = [&] {  // only once everything is enqueued: a failed call reports no output
        for (int i = 0; i < ncrops; ++i)
            if (written) written[i] = plan.crops[size_t(i)].count;
        return 0;
    };
    if (ncrops == 0 || length == 0) return report();
    const int C = plan.channels;
    if (C <= 0 || length > (int64_t(1) << 40) / (int64_t(ncrops) * C))
        return set_last_error("gsc_decode_crops: output too large for one call");
    hipStream_t hs = static_cast<hipStream_t>(hip_stream);
    // the call's own block: job descriptors, then the symbol scratch; stream-ordered, so calls on other
    // streams never share it
    const size_t njob = size_t(ncrops), npc = plan.pieces.size();
    const size_t desc_bytes = (njob * sizeof(CropJob) + npc * sizeof(CropPiece) + 15) & ~size_t(15);
    const bool fused = t_crop_variant == 2;  // no symbol scratch
    const size_t sym_bytes = fused ? 0 : size_t(plan.slots) * kDecodeS * sizeof(uint16_t);
    std::vector<unsigned char> host(desc_bytes, 0);
    CropJob* hj = reinterpret_cast<CropJob*>(host.data());
    int lds_bytes = 0;
    for (size_t i = 0; i < njob; ++i) {
        const PlanCrop& pc = plan.crops[i];
        const gsc_stream& st = *streams[pc.stream];
        hj[i] = CropJob{st.d_frames, st.d_cps,   reinterpret_cast<const uint32_t*>(st.d_bytes),
                        st.d_cb,     st.d_att,   st.ncp,
                        st.nwords,   st.ncb,     st.natt,
                        pc.begin,    pc.count,   int32_t(st.idx.ix.frames.size()),
                        pc.f0,       pc.f1,      pc.piece0};
        lds_bytes = std::max(lds_bytes, st.lds_bytes);
    }
    if (npc) std::memcpy(host.data() + njob * sizeof(CropJob), plan.pieces.data(), npc * sizeof(CropPiece));
    unsigned char* d_block = nullptr;
    DEC_TRY(hipMallocAsync(reinterpret_cast<void**>(&d_block), desc_bytes + std::max<size_t>(sym_bytes, 16), hs));
    struct FreeAsync {
        unsigned char* p;
        hipStream_t s;
        ~FreeAsync() { (void)hipFreeAsync(p, s); }
    } guard{d_block, hs};
    // pageable source: the runtime has taken the bytes when the call returns (it stages a small copy;
    // one it cannot stage it completes first, and then this call waits for the stream's earlier work)
    DEC_TRY(hipMemcpyAsync(d_block, host.data(), desc_bytes, hipMemcpyHostToDevice, hs));
    const CropJob* d_jobs = reinterpret_cast<const CropJob*>(d_block);
    const CropPiece* d_pieces = reinterpret_cast<const CropPiece*>(d_block + njob * sizeof(CropJob));
    uint16_t* d_sym = reinterpret_cast<uint16_t*>(d_block + desc_bytes);
    const int is_float = dtype == GSC_PCM_FLOAT32, planar = layout == GSC_LAYOUT_CT;
    if (fused) {
        // a workgroup per 4 Ki samples of a crop: 8 or 9 segments of a stereo ChunkSize-8 stream
        DEC_TRY(gsc_launch_crop_fused(d_jobs, ncrops, length, C, is_float, planar, int(std::min<int64_t>(length, 4096)),
                                      dst_device, hs));
    } else {
        DEC_TRY(gsc_launch_crop_unpack(d_jobs, ncrops, d_pieces, int(npc), d_sym, plan.slots, hs));
        // LDS variant: a workgroup per 16 Ki samples of a crop
        DEC_TRY(gsc_launch_crop_synth(d_jobs, ncrops, d_pieces, int(npc), d_sym, plan.slots, length, C, is_float,
                                      planar, t_crop_variant == 1 ? lds_bytes : -1,
                                      int(std::min<int64_t>(length, 16384)), dst_device, hs));
    }
    t_dtim.h2d_bytes = (long long)desc_bytes;
    t_dtim.frames = int(npc);
    t_dtim.symbols = plan.slots * kDecodeS;
    t_dtim.samples = int64_t(ncrops) * length * C;
    t_dtim.total_ms = now_ms() - t_begin;
    return report();
}

int gsc_stream_decode_samples(gsc_stream* st, long long begin, long long count, int16_t* pcm) {
    if (!st || (!pcm && count > 0)) return set_last_error("gsc_stream_decode_samples: invalid argument");
    if (begin < 0 || count < 0 || begin > st->idx.ix.samples || count > st->idx.ix.samples - begin)
        return set_last_error("gsc_stream_decode_samples: [" + std::to_string(begin) + ", " +
                              std::to_string(begin) + " + " + std::to_string(count) + ") outside the stream's " +
                              std::to_string(st->idx.ix.samples) + " samples");
    if (count == 0) return 0;
    if (require_device() != 0) return -1;
    const size_t n = size_t(count) * size_t(st->idx.ix.channels);
    Dev<int16_t> d_out;
    DEC_TRY(d_out.alloc(n));
    gsc_crop c{0, begin, count};
    gsc_stream* one[1] = {st};
    if (gsc_decode_crops(one, 1, &c, 1, GSC_PCM_INT16, GSC_LAYOUT_TC, count, d_out.p, nullptr, nullptr) != 0)
        return -1;
    const double t0 = now_ms();
    DEC_TRY(hipMemcpy(pcm, d_out.p, n * sizeof(int16_t), hipMemcpyDeviceToHost));  // after the default stream's work
    t_dtim.d2h_ms = now_ms() - t0;
    t_dtim.total_ms += t_dtim.d2h_ms;
    return 0;
}

}  // extern "C"
#endif  // GSC_DECODE_WALK_ONLY
