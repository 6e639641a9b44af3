// .gsc decoder: the host index of a stream
// (gsc_decode_index.cpp) and the device descriptors of the unpack and
// synthesis kernels (gsc_decode.hip, gsc_decode_crops.hip), which
// gsc_decode_abi.cpp fills.  The format is decoder/decoder.lpr:37-220.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

// symbols per checkpoint segment (one unpack lane walks one segment); the A/B
// behind the value is in DESIGN.md "f5 decoder"
#ifndef GSC_DECODE_S
#define GSC_DECODE_S 128
#endif

namespace gsc {

constexpr int kDecodeS = GSC_DECODE_S;
// LDS of one synthesis workgroup: codebook (int16) + attenuations (bytes) of
// a frame are staged when they fit, 4096 x 16 entries do (128 KiB + 4 KiB)
constexpr int kDecodeLdsBytes = 136 * 1024;
constexpr int kDecodeSynthThreads = 1024;

// A frame's tables as a synthesis workgroup stages them in LDS: the codebook
// (int16), the attenuations (bytes) from the next whole word on, `bytes` in all.
struct StagedSize {
    int64_t att_at, bytes;
};
constexpr StagedSize staged_size(int64_t count, int64_t cs) {
    const int64_t att_at = (count * cs * 2 + 3) & ~int64_t(3);
    return StagedSize{att_at, att_at + count};
}

// What every kernel needs of one frame.  Offsets index the slabs the frame
// was uploaded to: those of one decode call, or a resident stream's own.
struct FrameTables {
    int64_t bs_off;    // first byte of the frame's bitstream in the byte slab
    int64_t cb_off;    // codebook: count * cs int16 (a multiple of 8 elements)
    int64_t att_off;   // attenuations: count bytes
    int64_t nsym;      // FrameLength * ChannelCount
    int64_t cp_first;  // the frame's first checkpoint
    int32_t ver, ch, cs, count;
    int32_t lut[32];   // CAttrLookup[negative][attenuation] (decoder.lpr:88-96)
};

// One frame of a whole-frame decode call.
struct DecFrame : FrameTables {
    int64_t sym_off;  // first symbol word (idx << 2 | neg << 1 | rev) of the frame
    int64_t out_off;  // first int16 of the frame in the output, interleaved [sample][channel]
};

// One synthesis workgroup's share of a frame: symbol rows [row0, row0 + rows),
// a row being the ChannelCount symbols of one chunk time (cs * ch samples).
struct DecJob {
    int64_t row0;
    int32_t rows;
    int32_t frame;
};

// A checkpoint: bit offset within the frame's bitstream << 3 | (header + 1),
// header = variableCodingHeader on entry (-1 .. 3, decoder.lpr:173-186).
constexpr uint64_t make_checkpoint(uint64_t bit, int header) { return bit << 3 | uint64_t(header + 1); }

struct IndexFrame {
    size_t off = 0, att_off = 0, cb_off = 0, bs_off = 0, end_off = 0;  // byte offsets in the file
    int ver = 0, ch = 0, count = 0, bd = 0, cs = 0, rate = 0, adiv = 0;
    uint32_t flen = 0;         // FrameLength
    int64_t nsym = 0;          // FrameLength * ChannelCount
    uint64_t nbits = 0;        // bits of the bitstream (it occupies ceil(nbits / 16) words)
    int64_t first_sample = 0;  // per channel
    size_t cp_first = 0, cp_count = 0;  // into Index::cps
    size_t cb_first = 0;       // into Index::codebook, a multiple of 8
    size_t att_first = 0;      // into Index::att
    int32_t lut[32] = {};
};

struct Index {
    std::vector<IndexFrame> frames;
    std::vector<uint64_t> cps;      // one per kDecodeS symbols of every frame
    std::vector<int16_t> codebook;  // Chunks (decoder.lpr:130-158), frames padded to 8 elements
    std::vector<uint8_t> att;       // Attenuations (decoder.lpr:115-126)
    int channels = 0, rate = 0;
    int64_t samples = 0;            // per channel
    int64_t symbols = 0;
    size_t len = 0;                 // bytes of the stream the index was built from
    bool has_tables = true;         // false: codebook and att are empty until index_expand_tables
};

// The sequential pass (host only): frame offsets, checkpoints, lookup tables,
// and every validation.  0, or -1 with *err set; never reads outside [g, g + len).
int decode_walk(const uint8_t* g, size_t len, Index* ix, std::string* err);

// ---- seek tables ------------------------------------------------------------
// What the walk finds by following the two chains, as a side blob (layout:
// include/soundchunks.h): per frame its byte offset and the bits of its
// bitstream, then every checkpoint.  Little-endian, 32 + 16 F + 8 P bytes.
constexpr size_t kTableHeaderBytes = 32;
constexpr uint32_t kTableVersion = 1;
void index_table_write(const Index& ix, std::vector<uint8_t>* out);

// runs fn(0 .. n - 1), possibly on several threads; frames are independent
using ParallelRunner = std::function<void(int n, const std::function<void(int)>& fn)>;

// The host half of opening a stream with a table: the index the walk would
// have built if every claim of the table holds.  It checks what needs no
// symbol walk (sizes, magic, version, S, the stream's length, every frame
// header at its claimed offset, checkpoint counts and ranges, and that the
// claimed bitstream lengths chain the frames exactly to `len`) and fills
// frames, cps, codebook, att and the totals as decode_walk does, O(frames)
// plus the tables (built through `par` when given).  Whether the checkpoints
// and bit counts are the stream's own is left to decode_verify_kernel
// (gsc_decode.hip); an index from here must not be used before that passed.
// 0, or -1 with *err set; never reads outside [g, g + len) or the table.
// expand = false leaves codebook and att empty (has_tables false): a stream
// set expands them on the device, the host only on demand.
int index_from_table(const uint8_t* g, size_t len, const uint8_t* table, size_t tlen, Index* ix, std::string* err,
                     const ParallelRunner* par = nullptr, bool expand = true);

// codebook and att of an index that has none (has_tables false), from the
// stream it was built from, as the walk fills them; nothing when it has them.
void index_expand_tables(const uint8_t* g, Index* ix);
// the reverse: an index gives up its host copy of the tables
void index_drop_tables(Index* ix);

// The table of stream g (index_from_table's host checks apply) cut into the
// tables of nparts consecutive pieces of part_bytes[i] bytes, each a stream of
// its own whose frames start at its first byte; an empty piece gets an empty
// table.  0, or -1 with *err set.
int index_table_split(const uint8_t* g, size_t len, const uint8_t* table, size_t tlen, const size_t* part_bytes,
                      int nparts, std::vector<std::vector<uint8_t>>* out, std::string* err);

// ---- decode_verify_kernel's report -----------------------------------------
// One status word: kVerifyOk, or the smallest failing checkpoint (counted over
// the whole stream) << 8 | reason, so that the report does not depend on
// which lane came first.
constexpr unsigned long long kVerifyOk = ~0ull;
enum VerifyReason : int {
    kVerifyBounds = 1,  // a descriptor points outside its slab
    kVerifyIndex = 2,   // a chunk index >= ChunkCount
    kVerifyBit = 3,     // the segment ends at another bit offset than claimed
    kVerifyHeader = 4,  // ... in another header state than claimed
};
// the text of a status word other than kVerifyOk
std::string verify_message(const Index& ix, unsigned long long status);

// ---- sample ranges of resident streams (gsc_decode_crops.hip) -------------------
// A per-channel sample position in [0, samples): the frame that contains it
// (frames of FrameLength 0 contain nothing), the symbol row inside that frame,
// the position inside the chunk, and the checkpoint the row's first symbol
// belongs to.  0, or -1 with *err set.
int index_locate(const Index& ix, int64_t sample, int* frame, int64_t* row, int* within, int64_t* checkpoint,
                 std::string* err);

// One frame of a resident stream.
struct ResFrame : FrameTables {
    int64_t first_sample;  // per channel
};

// ---- slabs: streams and frame ranges back to back on the device -------------
// A position in, or a length of, each of the four slabs: stream bytes,
// checkpoints, codebook int16 and attenuation bytes.
struct SlabPos {
    int64_t bytes = 0, cps = 0, cb = 0, att = 0;
};
inline SlabPos operator+(const SlabPos& a, const SlabPos& b) {
    return {a.bytes + b.bytes, a.cps + b.cps, a.cb + b.cb, a.att + b.att};
}
inline SlabPos operator-(const SlabPos& a, const SlabPos& b) {
    return {a.bytes - b.bytes, a.cps - b.cps, a.cb - b.cb, a.att - b.att};
}
// What frames [b, e) of a stream occupy of its bytes and of its index's arrays.
struct Span {
    SlabPos first, count;
};
Span span_of(const Index& ix, int b, int e);
// The device descriptor of a frame whose stream was uploaded so that position
// p of the stream lies at rebase + p of the slabs.
FrameTables frame_tables(const IndexFrame& f, const SlabPos& rebase);

// Where expand_tables_kernel (gsc_decode.hip) finds a frame's packed tables in
// the byte slab: the attenuation nibbles, the codebook codes, ChunkBitDepth.
struct TableSrc {
    int64_t att_byte, cb_byte;
    int32_t bd, pad_;
};

// A stream set (gsc_stream_set_open): every stream whole, back to back in one
// set of slabs, as decode_parts lays out its parts.  Host only.
struct SetLayout {
    std::vector<SlabPos> base;    // where stream i starts in the slabs
    std::vector<int64_t> frame0;  // stream i's first frame in `frames`; count + 1 entries
    SlabPos total;
    std::vector<ResFrame> frames;  // every frame of every stream, rebased
    std::vector<TableSrc> src;     // per frame
    std::vector<uint64_t> bits;    // per frame: the bits of its bitstream
};
// Refuses (-1, *err) count <= 0 and 2^31 or more frames or checkpoints in all.
int set_layout(const Index* const* ixs, int count, SetLayout* out, std::string* err);
// The stream that owns checkpoint c of the set's checkpoint slab (a status word
// of decode_verify_kernel >> 8): the last one with base.cps <= c.
int set_stream_of_checkpoint(const SetLayout& lay, int64_t c);

// One crop on the device: its stream's slabs and their sizes, the clipped
// sample range and the frames [f0, f1) it crosses.
// What follows f1 is read by crop_resample_kernel alone (gsc_decode_resample.hip):
// there `begin` is in source samples, `count` in output samples, [f0, f1) are
// the frames of the source range [src_begin, src_end) the filter reads inside
// the stream, and rate_up / rate_down, half_taps and table are the resampler
// of the stream's rate (half_taps 0: none, the samples pass as they are).
struct CropJob {
    const ResFrame* frames;
    const uint64_t* cps;
    const uint32_t* words;
    const int16_t* cb;
    const uint8_t* att;
    int64_t ncp, nwords, ncb, natt;
    int64_t begin, count;
    int32_t nframes, f0, f1;
    int64_t src_begin, src_end;
    const int32_t* table;  // [rate_up][2 * half_taps] on the device
    int32_t rate_up, rate_down, half_taps;  // Fo / g, Fi / g, T
    int32_t src_ch, out_ch;
};

// One stream of a crop binding (gsc_crop_binding_create) on the device: what
// of a CropJob does not depend on the crop.  The kernels of a bound call make
// the CropJob of a crop from its (stream, begin, count) in device memory and
// this (gsc_crop_plan.h), where the other calls load one the host planned.
struct BoundStream {
    const ResFrame* frames;
    const uint64_t* cps;
    const uint32_t* words;
    const int16_t* cb;
    const uint8_t* att;
    int64_t ncp, nwords, ncb, natt;
    int64_t samples;       // per channel
    const int32_t* table;  // the resampler of the stream's rate for the binding's; null without one
    int32_t nframes, channels;
    int32_t rate_up, rate_down, half_taps;  // 1, 1, 0: the samples pass as they are
    int32_t pad_;
};

struct Crop {
    int stream;
    int64_t begin, count;
};

// The crops of one call, clipped (host only, no device needed; plan_crops below).
struct PlanCrop {
    int stream;
    int64_t begin, count;  // count: output samples, clipped where the source position reaches the stream's end
    // The source samples the crop reads inside its stream (the filter's reach on
    // both sides of its outputs, clipped to [0, samples)), the frames [f0, f1)
    // that hold them, and the stream's resampler.  The phase of output 0 is
    // (begin * rate_up) mod rate_up = 0 for every crop: `begin` is a whole sample.
    // A crop that writes nothing (count 0) has all four spans 0 (crop_plan_one).
    int f0 = 0, f1 = 0;
    int64_t src_begin = 0, src_end = 0;
    int rate_up = 1, rate_down = 1, half_taps = 0;
};
struct CropPlan {
    std::vector<PlanCrop> crops;
    int channels = 0;
};

// ---- crops at a common rate and channel count (gsc_decode_resample.hip) ------
// The resampler of one pair of rates (include/soundchunks.h has the
// definition): phases = Fo / g rows of taps = 2 T coefficients that sum to 2^24.
constexpr int kResampleZeros = 16;       // zero crossings per side
constexpr int kResampleShift = 24;       // a row sums to 1 << kResampleShift
constexpr int kResampleMaxTaps = 512;
constexpr int64_t kResampleMaxBytes = int64_t(16) << 20;
constexpr int kResampleTile = 512;       // output samples of one workgroup
// int16 source samples (all source channels) one workgroup keeps in LDS
constexpr int kResampleSrcCap = 24 * 1024;
struct ResampleShape {
    int phases = 1, step = 1, half_taps = 0;  // Fo / g, Fi / g, T
    int taps() const { return 2 * half_taps; }
};
// Refuses (-1, *err, both rates named) a rate <= 0, more than kResampleMaxTaps
// taps and a table of more than kResampleMaxBytes.
int resample_shape(int in_rate, int out_rate, ResampleShape* shape, std::string* err);
// The table of a pair, built on first use and kept for the life of the
// process; the pointer stays valid and what it points to is never written again.
const int32_t* resample_table(int in_rate, int out_rate, ResampleShape* shape, std::string* err);
// Outputs at out_rate from source position `begin` before the source position
// reaches `samples`: ceil((samples - begin) * phases / step).
int64_t resample_outputs(int64_t samples, int64_t begin, const ResampleShape& s);

// The one host planner, of gsc_decode_crops (out_rate 0, out_channels 0) and
// gsc_decode_crops_fmt: every crop through crop_plan_one (gsc_crop_plan.h), as
// the kernels of a bound call plan theirs.  Counts are output samples at
// out_rate (0: every stream keeps its rate), clipped where the source position
// reaches the stream's end.  out_channels 0: the streams must agree; otherwise
// a stream must have out_channels channels or one, or out_channels is one.
// Refuses (-1, *err) a whole call for begin < 0, begin > samples, count < 0,
// count > length or a bad stream index in any crop, a pair of rates
// resample_shape refuses, a filter whose reach times the stream's channels
// exceeds kResampleSrcCap, and a stream of more than 2^40 samples per channel
// or a length of more than 2^40 / rate_down ("too long for one call").
int plan_crops(const Index* const* ixs, int nstreams, const Crop* crops, int ncrops, int64_t length, int out_rate,
               int out_channels, CropPlan* plan, std::string* err);

}  // namespace gsc
