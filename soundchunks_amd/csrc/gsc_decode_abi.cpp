// .gsc decoder, HIP runtime side and C ABI.
//
// decode_parts uploads the frames a call asks for, as gsc_decode_index.cpp
// indexed them (the walk, or a seek table checked on the device), and runs
// gsc_decode.hip's two stages over all of them.  A resident stream
// (gsc_stream_open, gsc_stream_open_with_table) keeps the index and the bytes on the
// device; gsc_decode_crops then decodes batches of sample ranges into
// caller-owned device memory (plan_crops; gsc_decode_crops.hip), gsc_decode_crops_fmt
// at a common rate and channel count (gsc_decode_resample.hip).  A stream set
// (gsc_stream_set_open) keeps many streams in one Slabs, laid out by
// set_layout (gsc_decode_set.cpp), their tables expanded on the device.  All
// keep their device copies in a Slabs and describe a frame with frame_tables.
// A crop binding (gsc_crop_binding_create) describes resident streams once on
// the device; gsc_crop_binding_decode then takes the crops from device memory
// and only launches: the kernels plan each crop themselves (gsc_crop_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "../../include/soundchunks.h"
#include "gsc_crop_plan.h"
#include "gsc_decode.h"
#include "gsc_device.h"
#include "gsc_envelope.h"
#include "gsc_hip_host.h"
#include "gsc_launch.h"
#include "gsc_mix.h"

struct gsc_index {
    gsc::Index ix;
    std::mutex mu;  // a set member's host tables are filled on first use (ensure_tables)
};

namespace gsc {

namespace {

thread_local gsc_decode_timing t_dtim;
thread_local gsc_open_timing t_otim;  // the last gsc_stream_open* / gsc_index_create_with_table
thread_local gsc_set_open_timing t_stim;  // the last gsc_stream_set_open
// where Dev::alloc counts its hipMalloc calls while a stream set opens (else null)
thread_local int* t_alloc_count = nullptr;

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
    hipError_t alloc(size_t n) {
        if (t_alloc_count) ++*t_alloc_count;
        return hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * std::max<size_t>(n, 1));
    }
};

// the dynamic LDS a synthesis workgroup wants for a frame: its staged tables when they fit
int frame_lds_bytes(const IndexFrame& f) {
    const int64_t need = staged_size(f.count, f.cs).bytes;
    return f.flen > 0 && need <= kDecodeLdsBytes ? int(need) : 0;
}

// The device copy of one or more spans and of their frame table, freed with
// the owner.  The byte slab is whole words plus 16 zero bytes, the codebook
// ends in 16 zero int16 and the attenuations in one zero byte; nwords, ncp,
// ncb and natt are what a kernel may index, those tails included.
template <typename Frame>
struct Slabs {
    Dev<uint8_t> bytes, att;
    Dev<uint64_t> cps;
    Dev<int16_t> cb;
    Dev<Frame> frames;
    int64_t nwords = 0, ncp = 0, ncb = 0, natt = 0;
    long long h2d_bytes = 0;  // what put and put_frames copied

    const uint32_t* words() const { return reinterpret_cast<const uint32_t*>(bytes.p); }

    int alloc(const SlabPos& n, size_t nframes) {
        const size_t whole = size_t(n.bytes) & ~size_t(3), byte_alloc = ((size_t(n.bytes) + 3) & ~size_t(3)) + 16;
        nwords = int64_t(byte_alloc / 4);
        ncp = n.cps;
        ncb = n.cb + 16;
        natt = n.att + 1;
        DEC_TRY(bytes.alloc(byte_alloc));
        DEC_TRY(att.alloc(size_t(natt)));
        DEC_TRY(cps.alloc(size_t(ncp)));
        DEC_TRY(cb.alloc(size_t(ncb)));
        DEC_TRY(frames.alloc(nframes));
        DEC_TRY(hipMemset(bytes.p + whole, 0, byte_alloc - whole));
        DEC_TRY(hipMemset(cb.p + n.cb, 0, 16 * sizeof(int16_t)));
        DEC_TRY(hipMemset(att.p + n.att, 0, 1));
        return 0;
    }
    // span sp of stream g, indexed by ix, to position `at` of the slabs
    int put(const Span& sp, const SlabPos& at, const uint8_t* g, const Index& ix) {
        const SlabPos &a = sp.first, &n = sp.count;
        if (n.bytes) DEC_TRY(hipMemcpy(bytes.p + at.bytes, g + a.bytes, size_t(n.bytes), hipMemcpyHostToDevice));
        if (n.cps)
            DEC_TRY(hipMemcpy(cps.p + at.cps, ix.cps.data() + a.cps, size_t(n.cps) * sizeof(uint64_t),
                              hipMemcpyHostToDevice));
        if (n.cb)
            DEC_TRY(hipMemcpy(cb.p + at.cb, ix.codebook.data() + a.cb, size_t(n.cb) * sizeof(int16_t),
                              hipMemcpyHostToDevice));
        if (n.att) DEC_TRY(hipMemcpy(att.p + at.att, ix.att.data() + a.att, size_t(n.att), hipMemcpyHostToDevice));
        h2d_bytes += n.bytes + n.cps * int64_t(sizeof(uint64_t)) + n.cb * int64_t(sizeof(int16_t)) + n.att;
        return 0;
    }
    int put_frames(const std::vector<Frame>& f) {
        DEC_TRY(hipMemcpy(frames.p, f.data(), f.size() * sizeof(Frame), hipMemcpyHostToDevice));
        h2d_bytes += (long long)(f.size() * sizeof(Frame));
        return 0;
    }
};

// n bytes of host staging to the device in pieces of at most kStagePiece: the
// number of copies follows the bytes, not the streams they came from.
constexpr size_t kStagePiece = size_t(64) << 20;
int copy_pieces(void* dst, const void* src, size_t n, hipStream_t st, gsc_set_open_timing* tim) {
    for (size_t at = 0; at < n; at += kStagePiece) {
        const size_t m = std::min(kStagePiece, n - at);
        DEC_TRY(hipMemcpyAsync(static_cast<unsigned char*>(dst) + at, static_cast<const unsigned char*>(src) + at, m,
                               hipMemcpyHostToDevice, st));
        ++tim->h2d_copies;
        tim->uploaded_bytes += (long long)m;
    }
    return 0;
}

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
    std::vector<Span> spans(parts.size());
    std::vector<SlabPos> bases(parts.size());
    SlabPos total;  // cb: a multiple of 8, as every cb_first
    int64_t nsym = 0, nout = 0;
    int lds_bytes = 0;
    for (size_t pi = 0; pi < parts.size(); ++pi) {
        const Part& pt = parts[pi];
        const Span& sp = spans[pi] = span_of(*pt.ix, pt.b, pt.e);
        bases[pi] = total;
        total = total + sp.count;
        const int64_t out_before = nout;
        for (int i = pt.b; i < pt.e; ++i) {
            const IndexFrame& f = pt.ix->frames[size_t(i)];
            DecFrame d{};
            static_cast<FrameTables&>(d) = frame_tables(f, bases[pi] - sp.first);
            d.sym_off = nsym;
            d.out_off = nout;
            const int64_t row = int64_t(f.cs) * f.ch;  // int16 values per symbol row
            const int64_t cbn = int64_t(f.count) * f.cs;
            if (f.flen > 0) {
                lds_bytes = std::max(lds_bytes, frame_lds_bytes(f));
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
    if (total.cps >= (int64_t(1) << 31) || frames.size() >= (size_t(1) << 31) || jobs.size() >= (size_t(1) << 31))
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
        Slabs<DecFrame> s;
        Dev<DecJob> d_jobs;
        Dev<int16_t> d_out;
        Dev<uint16_t> d_sym;
        Event e0, e1, e2;
        const double t0 = now_ms();
        if (s.alloc(total, frames.size()) != 0) return -1;
        DEC_TRY(d_jobs.alloc(jobs.size()));
        DEC_TRY(d_out.alloc(size_t(nout)));
        DEC_TRY(d_sym.alloc(size_t(nsym)));
        DEC_TRY(hipEventCreate(&e0.e));
        DEC_TRY(hipEventCreate(&e1.e));
        DEC_TRY(hipEventCreate(&e2.e));
        for (size_t pi = 0; pi < parts.size(); ++pi)
            if (s.put(spans[pi], bases[pi], parts[pi].g, *parts[pi].ix) != 0) return -1;
        if (s.put_frames(frames) != 0) return -1;
        DEC_TRY(hipMemcpy(d_jobs.p, jobs.data(), jobs.size() * sizeof(DecJob), hipMemcpyHostToDevice));
        DEC_TRY(hipDeviceSynchronize());
        tim->h2d_bytes = s.h2d_bytes + (long long)(jobs.size() * sizeof(DecJob));
        const double t1 = now_ms();
        DEC_TRY(hipEventRecord(e0.e, nullptr));
        DEC_TRY(gsc_launch_decode_unpack(s.frames.p, int(frames.size()), s.cps.p, s.ncp, s.words(), s.nwords, d_sym.p,
                                         nsym, nullptr));
        DEC_TRY(hipEventRecord(e1.e, nullptr));
        DEC_TRY(gsc_launch_decode_synth(s.frames.p, int(frames.size()), d_jobs.p, int(jobs.size()), lds_bytes, d_sym.p,
                                        nsym, s.cb.p, s.ncb, s.att.p, s.natt, d_out.p, nout, nullptr));
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

// The device copies of the resamplers' tables (resample_table): one per device
// and reduced pair of rates, uploaded on first use with a blocking copy and
// kept, never written again and never freed, for the life of the process, so
// that crop calls on any HIP stream may read them without ordering.
int device_resample_table(int in_rate, int out_rate, const int32_t** table) {
    ResampleShape sh;
    std::string err;
    const int32_t* host = resample_table(in_rate, out_rate, &sh, &err);
    if (!host) return set_last_error(err);
    if (require_device() != 0) return -1;
    int dev = 0;
    DEC_TRY(hipGetDevice(&dev));
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, const int32_t*> tables;
    std::lock_guard<std::mutex> lock(mu);
    const int32_t*& slot = tables[std::make_tuple(dev, sh.phases, sh.step)];
    if (!slot) {
        const size_t bytes = size_t(sh.phases) * size_t(sh.taps()) * sizeof(int32_t);
        int32_t* p = nullptr;
        DEC_TRY(hipMalloc(reinterpret_cast<void**>(&p), bytes));
        const hipError_t e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return set_last_error(std::string("gsc resample: table upload: ") + hipGetErrorString(e));
        }
        slot = p;
    }
    *table = slot;
    return 0;
}

// samples of a crop that one workgroup of the fused kernels takes: 8 or 9 segments of a stereo ChunkSize-8 stream
constexpr int kCropTile = 4096;

// The int16 source samples a workgroup of the resampling kernels keeps in LDS for a tile of `tile` outputs
// of one stream, all channels.
int64_t source_reach(int64_t tile, int rate_up, int rate_down, int half_taps, int channels) {
    // rounded up, so that the kernel's outputs per pass come out as the whole tile
    const int64_t reach = ((tile - 1) * rate_down + rate_up - 1) / rate_up + 2 * half_taps + 2;
    return std::min<int64_t>(reach * channels, kResampleSrcCap);
}

// 0, or the refusal of an element type or layout no crop kernel writes
int check_pcm_format(const char* who, int dtype, int layout) {
    const bool dtype_ok = dtype == GSC_PCM_INT16 || dtype == GSC_PCM_FLOAT32;
    if (dtype_ok && (layout == GSC_LAYOUT_TC || layout == GSC_LAYOUT_CT)) return 0;
    return set_last_error(std::string(who) + (dtype_ok ? ": unknown layout" : ": unknown dtype"));
}

// the refusal of `what`, whose memory is device `lives`'s, on a thread bound to device `dev`
std::string other_device(const std::string& what, int lives, int dev) {
    return what + " lives on device " + std::to_string(lives) + ", the calling thread is bound to device " +
           std::to_string(dev);
}

// 0, or `who`'s refusal of `what` at p, which is not device memory of device `dev` (where `owner` lives).
// For once-per-corpus calls: it asks the runtime.
int check_device_memory(const char* who, const std::string& what, const void* p, int dev, const char* owner) {
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged))
        return set_last_error(std::string(who) + ": " + what + " is not device memory");
    if (at.type == hipMemoryTypeDevice && at.device != dev)
        return set_last_error(std::string(who) + ": " + what + " lives on device " + std::to_string(at.device) +
                              ", " + owner + " on device " + std::to_string(dev));
    return 0;
}

// delete h on its own device, after the work queued there: crop calls still read what h owns
template <typename Handle>
void free_on_device(Handle* h) {
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != h->device;
    if (sw) (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    if (sw) (void)hipSetDevice(cur);
}

}  // namespace
}  // namespace gsc

// A stream resident on one device: the index, and on the device its slabs
// (every byte, every checkpoint, the int16 codebooks, the attenuations and
// the frame table), until gsc_stream_free.
struct gsc_stream {
    gsc_index idx;
    int device = 0;
    gsc::Slabs<gsc::ResFrame> slabs;  // its own; empty in a member of a set
    // what the kernels get: its own slabs, or the set's with `frames` at its own first frame
    const gsc::ResFrame* frames = nullptr;
    const uint64_t* cps = nullptr;
    const uint32_t* words = nullptr;
    const int16_t* cb = nullptr;
    const uint8_t* att = nullptr;
    int64_t ncp = 0, nwords = 0, ncb = 0, natt = 0;
    const gsc_stream_set* set = nullptr;  // the owner of a borrowed member

    void view(const gsc::Slabs<gsc::ResFrame>& s, int64_t frame0) {
        frames = s.frames.p + frame0;
        cps = s.cps.p;
        words = s.words();
        cb = s.cb.p;
        att = s.att.p;
        ncp = s.ncp;
        nwords = s.nwords;
        ncb = s.ncb;
        natt = s.natt;
    }
};

// Streams opened together: one set of slabs, one index and one borrowed
// gsc_stream per member.
struct gsc_stream_set {
    int device = 0;
    gsc::Slabs<gsc::ResFrame> slabs;
    std::unique_ptr<gsc_stream[]> members;
    int count = 0;
};

namespace gsc {
namespace {

// A resampler and a channel count that streams of a binding share: what the LDS of a workgroup depends on.
struct BoundShape {
    int rate_up, rate_down, half_taps, channels;
    bool operator==(const BoundShape& o) const {
        return rate_up == o.rate_up && rate_down == o.rate_down && half_taps == o.half_taps && channels == o.channels;
    }
};

thread_local gsc_crop_call_stats t_bstat;  // the last gsc_crop_binding_decode or gsc_crop_binding_mix

}  // namespace
}  // namespace gsc

// The streams of a loader, described once on the device (BoundStream): what
// gsc_crop_binding_decode needs to launch without looking at a crop.
struct gsc_crop_binding {
    int device = 0, nstreams = 0, channels = 0;
    bool fmt = false;      // an output rate or channel count was given: the resampling kernel
    int max_step = 1;      // the largest rate_down: bounds `length`
    gsc::Dev<gsc::BoundStream> streams;
    std::vector<gsc::BoundShape> shapes;  // the distinct ones of the streams
    std::vector<int64_t> samples;         // per stream, per channel: the blocks of an envelope

    // The LDS of a workgroup of the resampling kernel for a tile of `tile` outputs: the widest
    // source_reach over the binding's streams (as gsc_decode_crops_fmt takes it over a call's crops).
    int src_samples(int64_t tile) const {
        int64_t n = 1;
        for (const gsc::BoundShape& s : shapes)
            n = std::max(n, gsc::source_reach(tile, s.rate_up, s.rate_down, s.half_taps, s.channels));
        return int(n);
    }
};

using namespace gsc;

// The index of a set's member holds no codebook and no attenuations until a
// whole-frame decode asks for them (decode_parts uploads them from the host).
static void ensure_tables(const gsc_index* ix, const uint8_t* gsc) {
    gsc_index* m = const_cast<gsc_index*>(ix);
    std::lock_guard<std::mutex> lock(m->mu);
    index_expand_tables(gsc, &m->ix);
}

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
    ensure_tables(ix, gsc);
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
    if (st->set) {
        set_last_error("gsc_stream_free: the stream belongs to a stream set; free the set");
        return;
    }
    free_on_device(st);
}

// A stream's index to the device, at position 0 of `s`: the bytes and the
// checkpoints, with_tables also the codebooks and attenuations; the frame table.
static int upload_resident(const uint8_t* gsc, const Index& ix, bool with_tables, Slabs<ResFrame>* s) {
    std::vector<ResFrame> frames(ix.frames.size());
    for (size_t i = 0; i < frames.size(); ++i) {
        const IndexFrame& f = ix.frames[i];
        static_cast<FrameTables&>(frames[i]) = frame_tables(f, SlabPos{});
        frames[i].first_sample = f.first_sample;
    }
    Span all = span_of(ix, 0, int(frames.size()));  // the whole stream
    if (!with_tables) all.count.cb = all.count.att = 0;
    if (s->alloc(all.count, frames.size()) != 0 || s->put(all, SlabPos{}, gsc, ix) != 0 || s->put_frames(frames) != 0)
        return -1;
    DEC_TRY(hipDeviceSynchronize());
    return 0;
}

// decode_verify_kernel over an uploaded stream whose index came from a table:
// 0 when every claim holds, else -1 with the first failing checkpoint named.
static int verify_resident(const Index& ix, const Slabs<ResFrame>& s) {
    if (ix.cps.size() >= (size_t(1) << 31) || ix.frames.size() >= (size_t(1) << 31))
        return set_last_error("gsc decode: stream too large for one call");
    std::vector<uint64_t> bits(ix.frames.size());
    for (size_t i = 0; i < bits.size(); ++i) bits[i] = ix.frames[i].nbits;
    Dev<uint64_t> d_bits;
    Dev<unsigned long long> d_status;
    unsigned long long status = kVerifyOk;
    DEC_TRY(d_bits.alloc(bits.size()));
    DEC_TRY(d_status.alloc(1));
    DEC_TRY(hipMemcpy(d_bits.p, bits.data(), bits.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    DEC_TRY(hipMemcpy(d_status.p, &status, sizeof(status), hipMemcpyHostToDevice));
    DEC_TRY(gsc_launch_decode_verify(s.frames.p, d_bits.p, int(bits.size()), s.cps.p, s.ncp, s.words(), s.nwords,
                                     d_status.p, nullptr, nullptr));
    DEC_TRY(hipMemcpy(&status, d_status.p, sizeof(status), hipMemcpyDeviceToHost));  // after the kernel
    return status == kVerifyOk ? 0 : set_last_error(verify_message(ix, status));
}

// The index of a stream for an open: the walk, or with a table its host half
// (the device half follows the upload).
static int open_index(const uint8_t* gsc, size_t len, const uint8_t* table, size_t table_len, Index* ix) {
    const double t0 = now_ms();
    std::string err;
    const ParallelRunner par = [](int n, const std::function<void(int)>& fn) { parallel_for(n, host_threads(), fn); };
    const int rc = table ? index_from_table(gsc, len, table, table_len, ix, &err, &par) : decode_walk(gsc, len, ix, &err);
    if (rc != 0) return set_last_error(err);
    t_otim.host_ms = now_ms() - t0;
    t_otim.checkpoints = (long long)ix->cps.size();
    return 0;
}

// upload, and with a table the check on the device; the timing of both
static int open_device(const uint8_t* gsc, const Index& ix, bool with_table, bool with_tables, Slabs<ResFrame>* s) {
    if (require_device() != 0) return -1;
    const double t1 = now_ms();
    if (upload_resident(gsc, ix, with_tables, s) != 0) return -1;
    const double t2 = now_ms();
    t_otim.upload_ms = t2 - t1;
    t_otim.uploaded_bytes = s->h2d_bytes;
    if (with_table) {
        if (verify_resident(ix, *s) != 0) return -1;
        t_otim.verify_ms = now_ms() - t2;
    }
    return 0;
}

static int stream_open(const uint8_t* gsc, size_t len, const uint8_t* table, size_t table_len, gsc_stream* h) {
    const double t0 = now_ms();
    if (open_index(gsc, len, table, table_len, &h->idx.ix) != 0) return -1;
    const Index& ix = h->idx.ix;
    t_dtim.host_index_ms = t_otim.host_ms;
    if (require_device() != 0) return -1;
    DEC_TRY(hipGetDevice(&h->device));
    if (open_device(gsc, ix, table != nullptr, true, &h->slabs) != 0) return -1;
    h->view(h->slabs, 0);
    t_dtim.h2d_ms = t_otim.upload_ms;
    t_dtim.h2d_bytes = h->slabs.h2d_bytes;
    t_dtim.frames = int(ix.frames.size());
    t_dtim.total_ms = t_otim.total_ms = now_ms() - t0;
    return 0;
}

gsc_stream* gsc_stream_open(const uint8_t* gsc, size_t len) {
    t_dtim = gsc_decode_timing{};
    t_otim = gsc_open_timing{};
    std::unique_ptr<gsc_stream> h(new gsc_stream());
    return stream_open(gsc, len, nullptr, 0, h.get()) == 0 ? h.release() : nullptr;
}

gsc_stream* gsc_stream_open_with_table(const uint8_t* gsc, size_t len, const uint8_t* table, size_t table_len) {
    t_dtim = gsc_decode_timing{};
    t_otim = gsc_open_timing{};
    if (!table) {
        set_last_error("gsc_stream_open_with_table: table is null");
        return nullptr;
    }
    // a refused table frees the stream, and with it every slab it uploaded
    std::unique_ptr<gsc_stream> h(new gsc_stream());
    return stream_open(gsc, len, table, table_len, h.get()) == 0 ? h.release() : nullptr;
}

// The device half of gsc_stream_set_open: one set of slabs for every stream,
// the tables expanded and every table's claims checked there.  The runtime
// calls are counted where they are made; none of them depends on `count`.
static int set_open_device(const uint8_t* const* gscs, int count, const SetLayout& lay, gsc_stream_set* set) {
    gsc_set_open_timing& tim = t_stim;
    const double t0 = now_ms();
    if (require_device() != 0) return -1;
    DEC_TRY(hipGetDevice(&set->device));
    // The default stream.  A stream of the library's own was built and measured, non-blocking and
    // ordinary: with either one resident, crop calls on the default stream returned all-zero ranges
    // now and then; without one, never (DESIGN.md "Stream sets").  The open waits for this stream only.
    hipStream_t hs = nullptr;
    struct CountAllocs {  // every Dev::alloc of this thread until the function returns
        explicit CountAllocs(int* n) { t_alloc_count = n; }
        ~CountAllocs() { t_alloc_count = nullptr; }
    } count_allocs(&tim.device_allocations);
    const size_t nf = lay.frames.size();
    // host staging: the streams' bytes and checkpoints back to back, as the slabs hold them
    std::vector<uint8_t> bytes(size_t(lay.total.bytes));
    std::vector<uint64_t> cps(size_t(lay.total.cps));
    parallel_for(count, host_threads(), [&](int i) {
        const Index& ix = set->members[i].idx.ix;
        const SlabPos& at = lay.base[size_t(i)];
        if (ix.len) std::memcpy(bytes.data() + at.bytes, gscs[i], ix.len);
        if (!ix.cps.empty()) std::memcpy(cps.data() + at.cps, ix.cps.data(), ix.cps.size() * sizeof(uint64_t));
    });
    // what only the open's two kernels read: per frame the packed tables' place and the bit count, the status word
    const size_t src_bytes = nf * sizeof(TableSrc), bits_bytes = nf * sizeof(uint64_t);
    std::vector<unsigned char> aux(src_bytes + bits_bytes + sizeof(unsigned long long));
    unsigned long long status = kVerifyOk;
    if (nf) std::memcpy(aux.data(), lay.src.data(), src_bytes);
    if (nf) std::memcpy(aux.data() + src_bytes, lay.bits.data(), bits_bytes);
    std::memcpy(aux.data() + src_bytes + bits_bytes, &status, sizeof(status));
    Slabs<ResFrame>& s = set->slabs;
    Dev<unsigned char> d_aux;
    Event e1, e2, e3;
    // A failure below leaves work queued on hs that reads the staging vectors and d_aux: wait for
    // that stream before they go.  Declared last, so it runs first.
    struct SyncOnFailure {
        hipStream_t s;
        bool armed;
        int* waits;
        ~SyncOnFailure() {
            if (!armed) return;
            (void)hipStreamSynchronize(s);
            ++*waits;
        }
    } on_failure{hs, true, &tim.synchronisations};
    if (s.alloc(lay.total, nf) != 0) return -1;  // the five slabs
    DEC_TRY(d_aux.alloc(aux.size()));
    DEC_TRY(hipEventCreate(&e1.e));
    DEC_TRY(hipEventCreate(&e2.e));
    DEC_TRY(hipEventCreate(&e3.e));
    if (copy_pieces(s.bytes.p, bytes.data(), bytes.size(), hs, &tim) != 0 ||
        copy_pieces(s.cps.p, cps.data(), cps.size() * sizeof(uint64_t), hs, &tim) != 0 ||
        copy_pieces(s.frames.p, lay.frames.data(), nf * sizeof(ResFrame), hs, &tim) != 0 ||
        copy_pieces(d_aux.p, aux.data(), aux.size(), hs, &tim) != 0)
        return -1;
    const TableSrc* d_src = reinterpret_cast<const TableSrc*>(d_aux.p);
    const uint64_t* d_bits = reinterpret_cast<const uint64_t*>(d_aux.p + src_bytes);
    unsigned long long* d_status = reinterpret_cast<unsigned long long*>(d_aux.p + src_bytes + bits_bytes);
    tim.upload_ms = now_ms() - t0;
    DEC_TRY(hipEventRecord(e1.e, hs));
    DEC_TRY(gsc_launch_expand_tables(s.frames.p, d_src, int(nf), lay.total.cb, s.bytes.p, s.nwords * 4, s.cb.p, s.ncb,
                                     s.att.p, s.natt, hs, &tim.launches));
    DEC_TRY(hipEventRecord(e2.e, hs));
    // walked members' checkpoints pass trivially: one launch over everything
    DEC_TRY(gsc_launch_decode_verify(s.frames.p, d_bits, int(nf), s.cps.p, s.ncp, s.words(), s.nwords, d_status, hs,
                                     &tim.launches));
    DEC_TRY(hipEventRecord(e3.e, hs));
    DEC_TRY(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, hs));
    on_failure.armed = false;  // the wait is made here
    const hipError_t waited = hipStreamSynchronize(hs);  // the default stream, not the device
    ++tim.synchronisations;
    DEC_TRY(waited);
    float ms_e = 0, ms_v = 0;
    DEC_TRY(hipEventElapsedTime(&ms_e, e1.e, e2.e));
    DEC_TRY(hipEventElapsedTime(&ms_v, e2.e, e3.e));
    tim.expand_ms = ms_e;
    tim.verify_ms = ms_v;
    if (status != kVerifyOk) {
        // the smallest failing checkpoint of the slab: the lowest failing stream's first
        const int64_t c = int64_t(status >> 8);
        const int si = set_stream_of_checkpoint(lay, c);
        const unsigned long long local = (unsigned long long)(c - lay.base[size_t(si)].cps) << 8 | (status & 0xff);
        return set_last_error("gsc stream set: stream " + std::to_string(si) + ": " +
                              verify_message(set->members[si].idx.ix, local));
    }
    return 0;
}

gsc_stream_set* gsc_stream_set_open(const uint8_t* const* gscs, const size_t* lens, const uint8_t* const* tables,
                                    const size_t* table_lens, int count) {
    t_stim = gsc_set_open_timing{};
    const double t0 = now_ms();
    if (count <= 0 || !gscs || !lens || (tables && !table_lens)) {
        set_last_error(count <= 0 ? "gsc_stream_set_open: no streams" : "gsc_stream_set_open: invalid argument");
        return nullptr;
    }
    // a refused stream frees the set, and with it everything it allocated
    std::unique_ptr<gsc_stream_set> set(new gsc_stream_set());
    set->members.reset(new gsc_stream[size_t(count)]);
    set->count = count;
    std::vector<std::string> errs(static_cast<size_t>(count));
    std::vector<char> failed(static_cast<size_t>(count), 0);
    parallel_for(count, host_threads(), [&](int i) {
        Index* ix = &set->members[i].idx.ix;
        const uint8_t* t = tables ? tables[i] : nullptr;
        const int rc = t ? index_from_table(gscs[i], lens[i], t, table_lens[i], ix, &errs[size_t(i)], nullptr, false)
                         : decode_walk(gscs[i], lens[i], ix, &errs[size_t(i)]);
        if (rc != 0) {
            failed[size_t(i)] = 1;
        } else if (!t) {
            index_drop_tables(ix);  // the device expands every member's tables, the host on demand
        }
    });
    std::vector<const Index*> ixs(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) {
        if (failed[size_t(i)]) {
            set_last_error("gsc stream set: stream " + std::to_string(i) + ": " + errs[size_t(i)]);
            return nullptr;
        }
        ixs[size_t(i)] = &set->members[i].idx.ix;
    }
    SetLayout lay;
    std::string err;
    if (set_layout(ixs.data(), count, &lay, &err) != 0) {
        set_last_error(err);
        return nullptr;
    }
    t_stim.host_ms = now_ms() - t0;
    t_stim.streams = count;
    t_stim.frames = (long long)lay.frames.size();
    t_stim.checkpoints = lay.total.cps;
    if (set_open_device(gscs, count, lay, set.get()) != 0) return nullptr;
    for (int i = 0; i < count; ++i) {
        gsc_stream& m = set->members[i];
        m.device = set->device;
        m.view(set->slabs, lay.frame0[size_t(i)]);
        m.set = set.get();
    }
    t_stim.total_ms = now_ms() - t0;
    return set.release();
}

int gsc_stream_set_count(const gsc_stream_set* set) { return set ? set->count : set_last_error("null stream set"); }

gsc_stream* gsc_stream_set_stream(gsc_stream_set* set, int i) {
    if (!set || i < 0 || i >= set->count) {
        set_last_error(set ? "gsc_stream_set_stream: no stream " + std::to_string(i) : std::string("null stream set"));
        return nullptr;
    }
    return &set->members[i];
}

void gsc_stream_set_free(gsc_stream_set* set) {
    if (set) free_on_device(set);
}

void gsc_last_set_open_timing(gsc_set_open_timing* t) {
    if (t) *t = t_stim;
}

int gsc_stream_tables(const gsc_stream* st, int frame, int16_t* cb_out, uint8_t* att_out) {
    if (!st || !cb_out || !att_out) return set_last_error("gsc_stream_tables: invalid argument");
    if (frame < 0 || size_t(frame) >= st->idx.ix.frames.size())
        return set_last_error("gsc_stream_tables: no frame " + std::to_string(frame));
    ResFrame r{};
    DEC_TRY(hipMemcpy(&r, st->frames + frame, sizeof(r), hipMemcpyDeviceToHost));
    const int64_t slots = (int64_t(r.count) * r.cs + 7) & ~int64_t(7);
    if (r.count < 0 || r.cs < 0 || r.cb_off < 0 || r.cb_off + slots > st->ncb || r.att_off < 0 ||
        r.att_off + r.count > st->natt)
        return set_last_error("gsc_stream_tables: the frame's tables lie outside the slabs");
    if (slots) DEC_TRY(hipMemcpy(cb_out, st->cb + r.cb_off, size_t(slots) * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (r.count) DEC_TRY(hipMemcpy(att_out, st->att + r.att_off, size_t(r.count), hipMemcpyDeviceToHost));
    return 0;
}

gsc_index* gsc_index_create_with_table(const uint8_t* gsc, size_t len, const uint8_t* table, size_t table_len) {
    t_otim = gsc_open_timing{};
    if (!table) {
        set_last_error("gsc_index_create_with_table: table is null");
        return nullptr;
    }
    const double t0 = now_ms();
    std::unique_ptr<gsc_index> h(new gsc_index());
    Slabs<ResFrame> s;  // the bytes and the checkpoints, for the check alone
    if (open_index(gsc, len, table, table_len, &h->ix) != 0 || open_device(gsc, h->ix, true, false, &s) != 0)
        return nullptr;
    t_otim.total_ms = now_ms() - t0;
    return h.release();
}

int gsc_index_table(const gsc_index* ix, uint8_t** table, size_t* len) {
    if (!ix || !table || !len) return set_last_error("gsc_index_table: invalid argument");
    std::vector<uint8_t> t;
    index_table_write(ix->ix, &t);
    *table = static_cast<uint8_t*>(std::malloc(std::max<size_t>(t.size(), 1)));
    if (!*table) return set_last_error("gsc_index_table: out of memory");
    std::memcpy(*table, t.data(), t.size());
    *len = t.size();
    return 0;
}

void gsc_last_open_timing(gsc_open_timing* t) {
    if (t) *t = t_otim;
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

// gsc_decode_crops (has_fmt false: fmt holds its dtype, layout and length, no rate, no channels)
// and gsc_decode_crops_fmt under the name `name`: validate, plan, check the device, describe every
// crop in a CropJob, upload the jobs and launch.  One body fills one descriptor: the native
// call's jobs carry the resampler's fields too (the source range, 1 / 1 / 0, no table, both
// channel counts), which crop_fused_kernel never reads.
static int decode_crops(const char* name, gsc_stream* const* streams, int nstreams, const gsc_crop* crops,
                        int ncrops, const gsc_crop_format& fmt, bool has_fmt, void* dst_device, void* hip_stream,
                        long long* written) {
    const double t_begin = now_ms();
    const std::string who = name;
    if (!streams || nstreams <= 0) return set_last_error(who + ": no streams");
    if (check_pcm_format(name, fmt.dtype, fmt.layout) != 0) return -1;
    if (!dst_device) return set_last_error(who + ": dst_device is null");
    std::vector<const Index*> ixs(static_cast<size_t>(nstreams), nullptr);
    for (int s = 0; s < nstreams; ++s) {
        if (!streams[s]) return set_last_error(who + ": stream " + std::to_string(s) + " is null");
        ixs[size_t(s)] = &streams[s]->idx.ix;
    }
    std::vector<Crop> cr(static_cast<size_t>(std::max(ncrops, 0)));
    if (ncrops > 0 && !crops) return set_last_error(who + ": crops is null");
    for (int i = 0; i < ncrops; ++i) cr[size_t(i)] = Crop{crops[i].stream, crops[i].begin, crops[i].count};
    const int64_t length = fmt.length;
    CropPlan plan;
    std::string err;
    if (plan_crops(ixs.data(), nstreams, cr.data(), ncrops, length, fmt.out_rate, fmt.out_channels, &plan, &err) != 0)
        return set_last_error(err);
    if (require_device() != 0) return -1;
    int dev = 0;
    DEC_TRY(hipGetDevice(&dev));
    for (int s = 0; s < nstreams; ++s)
        if (streams[s]->device != dev)
            return set_last_error(other_device(who + ": stream " + std::to_string(s), streams[s]->device, dev));
    auto report = [&] {  // only once everything is enqueued: a failed call reports no output
        for (int i = 0; i < ncrops; ++i)
            if (written) written[i] = plan.crops[size_t(i)].count;
        return 0;
    };
    if (ncrops == 0 || length == 0) return report();
    const int C = plan.channels;
    if (C <= 0 || (has_fmt && C > 255) || length > (int64_t(1) << 40) / (int64_t(ncrops) * C))
        return set_last_error(who + ": output too large for one call");
    // the tables of the rates this call resamples from: the one place that may upload and block (first use)
    std::vector<const int32_t*> tables(static_cast<size_t>(nstreams), nullptr);
    for (const PlanCrop& pc : plan.crops)
        if (pc.half_taps > 0 && !tables[size_t(pc.stream)] &&
            device_resample_table(ixs[size_t(pc.stream)]->rate, fmt.out_rate, &tables[size_t(pc.stream)]) != 0)
            return -1;
    hipStream_t hs = static_cast<hipStream_t>(hip_stream);
    // the call's own block, the job descriptors: stream-ordered, so calls on other streams never share it
    const size_t njob = size_t(ncrops);
    const size_t desc_bytes = (njob * sizeof(CropJob) + 15) & ~size_t(15);
    std::vector<unsigned char> host(desc_bytes, 0);
    CropJob* hj = reinterpret_cast<CropJob*>(host.data());
    const int64_t tile = std::min<int64_t>(length, kResampleTile);
    int64_t src_samples = 1;  // the resampling kernel's LDS: the widest source span of a full tile, all channels
    int frames = 0;
    for (size_t i = 0; i < njob; ++i) {
        const PlanCrop& pc = plan.crops[i];
        const gsc_stream& st = *streams[pc.stream];
        const int sch = st.idx.ix.channels;
        hj[i] = CropJob{st.frames, st.cps,   st.words, st.cb,    st.att, st.ncp, st.nwords, st.ncb,
                        st.natt,   pc.begin, pc.count, int32_t(st.idx.ix.frames.size()),
                        pc.f0,     pc.f1,    pc.src_begin, pc.src_end, tables[size_t(pc.stream)],
                        pc.rate_up, pc.rate_down, pc.half_taps, sch, C};
        if (has_fmt)
            src_samples = std::max(src_samples, source_reach(tile, pc.rate_up, pc.rate_down, pc.half_taps, sch));
        frames += pc.f1 - pc.f0;
    }
    unsigned char* d_block = nullptr;
    DEC_TRY(hipMallocAsync(reinterpret_cast<void**>(&d_block), desc_bytes, hs));
    struct FreeAsync {
        unsigned char* p;
        hipStream_t s;
        ~FreeAsync() { (void)hipFreeAsync(p, s); }
    } guard{d_block, hs};
    // pageable source: the runtime has taken the bytes when the call returns (it stages a small copy;
    // one it cannot stage it completes first, and then this call waits for the stream's earlier work)
    DEC_TRY(hipMemcpyAsync(d_block, host.data(), desc_bytes, hipMemcpyHostToDevice, hs));
    const CropJob* d_jobs = reinterpret_cast<const CropJob*>(d_block);
    const int is_float = fmt.dtype == GSC_PCM_FLOAT32, planar = fmt.layout == GSC_LAYOUT_CT;
    if (has_fmt) {
        DEC_TRY(gsc_launch_crop_resample(d_jobs, ncrops, length, C, is_float, planar, int(src_samples), dst_device,
                                         hs));
    } else {
        DEC_TRY(gsc_launch_crop_fused(d_jobs, ncrops, length, C, is_float, planar,
                                      int(std::min<int64_t>(length, kCropTile)), dst_device, hs));
    }
    t_dtim.h2d_bytes = (long long)desc_bytes;
    t_dtim.frames = frames;
    t_dtim.samples = int64_t(ncrops) * length * C;
    t_dtim.total_ms = now_ms() - t_begin;
    return report();
}

int gsc_decode_crops(gsc_stream* const* streams, int nstreams, const gsc_crop* crops, int ncrops, int dtype,
                     int layout, long long length, void* dst_device, void* hip_stream, long long* written) {
    t_dtim = gsc_decode_timing{};
    const gsc_crop_format fmt{dtype, layout, length, 0, 0};
    return decode_crops("gsc_decode_crops", streams, nstreams, crops, ncrops, fmt, false, dst_device, hip_stream,
                        written);
}

int gsc_resample_tile(void) { return kResampleTile; }

int gsc_resample_table(int in_rate, int out_rate, int* phases, int* taps, const int32_t** coeff) {
    ResampleShape sh;
    std::string err;
    const int32_t* t = resample_table(in_rate, out_rate, &sh, &err);
    if (!t) return set_last_error(err);
    if (phases) *phases = sh.phases;
    if (taps) *taps = sh.taps();
    if (coeff) *coeff = t;
    return 0;
}

int gsc_resample_prepare(int in_rate, int out_rate) {
    const int32_t* t = nullptr;
    return in_rate == out_rate && in_rate > 0 ? 0 : device_resample_table(in_rate, out_rate, &t);
}

int gsc_decode_crops_fmt(gsc_stream* const* streams, int nstreams, const gsc_crop* crops, int ncrops,
                         const gsc_crop_format* fmt, void* dst_device, void* hip_stream, long long* written) {
    t_dtim = gsc_decode_timing{};
    if (!fmt) return set_last_error("gsc_decode_crops_fmt: format is null");
    return decode_crops("gsc_decode_crops_fmt", streams, nstreams, crops, ncrops, *fmt, true, dst_device, hip_stream,
                        written);
}

int gsc_crop_plan_model(const gsc_index* ix, int nstreams, int stream, long long begin, long long count,
                        long long length, int out_rate, long long* written, int* f0, int* f1, long long* src_begin,
                        long long* src_end) {
    if (!ix || out_rate < 0 || length < 0) return set_last_error("gsc_crop_plan_model: invalid argument");
    const Index& x = ix->ix;
    ResampleShape sh;  // a stream without samples has no rate of its own, as in plan_crops
    std::string err;
    if (out_rate != 0 && x.rate != out_rate && x.samples > 0 && resample_shape(x.rate, out_rate, &sh, &err) != 0)
        return set_last_error(err);
    if (x.samples > (int64_t(1) << 40) || length > (int64_t(1) << 40) / sh.step)
        return set_last_error("gsc_crop_plan_model: too long for one call");
    CropSpan sp{0, 0, 0, 0, 0};
    int status = crop_stream_status(stream, nstreams);
    if (status == kCropGood)
        status = crop_plan_one(begin, count, length, x.samples, int32_t(x.frames.size()), sh.phases, sh.step,
                               sh.half_taps, [&](int32_t i) { return x.frames[size_t(i)].first_sample; }, &sp);
    if (written) *written = status == kCropGood ? sp.count : -1;
    if (f0) *f0 = sp.f0;
    if (f1) *f1 = sp.f1;
    if (src_begin) *src_begin = sp.src_begin;
    if (src_end) *src_end = sp.src_end;
    return status;
}

gsc_crop_binding* gsc_crop_binding_create(gsc_stream* const* streams, int nstreams, int out_rate, int out_channels) {
    auto fail = [](const std::string& what) {
        set_last_error(what);
        return static_cast<gsc_crop_binding*>(nullptr);
    };
    auto named = [](int s) { return "gsc crop binding: stream " + std::to_string(s); };
    if (!streams || nstreams <= 0) return fail("gsc crop binding: no streams");
    if (out_rate < 0)
        return fail("gsc resample: output rate " + std::to_string(out_rate) + " Hz: a rate must be positive");
    if (out_channels < 0 || out_channels > 255) return fail("gsc crop binding: invalid argument");
    for (int s = 0; s < nstreams; ++s)
        if (!streams[s]) return fail(named(s) + " is null");
    if (require_device() != 0) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail("gsc crop binding: hipGetDevice failed");
    std::unique_ptr<gsc_crop_binding> b(new gsc_crop_binding());
    b->device = dev;
    b->nstreams = nstreams;
    b->fmt = out_rate != 0 || out_channels != 0;
    b->channels = out_channels ? out_channels : streams[0]->idx.ix.channels;
    if (b->channels <= 0 || b->channels > 255) return fail("gsc crop binding: invalid argument");
    std::vector<BoundStream> desc(static_cast<size_t>(nstreams));
    for (int s = 0; s < nstreams; ++s) {
        const gsc_stream& st = *streams[s];
        const Index& ix = st.idx.ix;
        const int cs = ix.channels;
        // plan_crops' refusals per stream, and gsc_decode_crops' of another device
        if (out_channels == 0 && cs != b->channels)
            return fail(named(s) + " has " + std::to_string(cs) + " channels, stream 0 has " +
                        std::to_string(b->channels));
        if (out_channels != 0 && cs != out_channels && cs != 1 && out_channels != 1)
            return fail(named(s) + " has " + std::to_string(cs) + " channels, which do not map to " +
                        std::to_string(out_channels) + " (equal counts, a mono stream, or a mono output)");
        ResampleShape sh;
        const int32_t* table = nullptr;
        if (out_rate != 0 && ix.rate != out_rate && ix.samples > 0) {
            std::string e;
            if (resample_shape(ix.rate, out_rate, &sh, &e) != 0) return fail(named(s) + ": " + e);
        }
        if ((int64_t(sh.taps()) + 2) * std::max(cs, 1) > kResampleSrcCap)
            return fail(named(s) + ": " + std::to_string(sh.taps()) + " taps x " + std::to_string(cs) +
                        " channels exceed the " + std::to_string(kResampleSrcCap) + " source samples of one workgroup");
        if (ix.samples > (int64_t(1) << 40) || ix.frames.size() >= (size_t(1) << 31))
            return fail(named(s) + ": too long for one call");
        if (st.device != dev)
            return fail(other_device(named(s), st.device, dev));
        // every table a call will read is on the device before the first call
        if (sh.half_taps > 0 && device_resample_table(ix.rate, out_rate, &table) != 0) {
            set_last_error(named(s) + ": " + gsc_last_error());
            return nullptr;
        }
        desc[size_t(s)] = BoundStream{st.frames, st.cps,     st.words,  st.cb,        st.att,
                                      st.ncp,    st.nwords,  st.ncb,    st.natt,      ix.samples,
                                      table,     int32_t(ix.frames.size()), cs,       sh.phases,
                                      sh.step,   sh.half_taps, 0};
        b->max_step = std::max(b->max_step, sh.step);
        b->samples.push_back(ix.samples);
        const BoundShape shape{sh.phases, sh.step, sh.half_taps, cs};
        if (std::find(b->shapes.begin(), b->shapes.end(), shape) == b->shapes.end()) b->shapes.push_back(shape);
    }
    const auto hip_failed = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) set_last_error(std::string("gsc crop binding: ") + what + ": " + hipGetErrorString(e));
        return e != hipSuccess;
    };
    if (hip_failed(b->streams.alloc(desc.size()), "hipMalloc") ||
        hip_failed(hipMemcpy(b->streams.p, desc.data(), desc.size() * sizeof(BoundStream), hipMemcpyHostToDevice),
                   "hipMemcpy") ||
        (b->fmt && hip_failed(gsc_prepare_crop_resample_bound(b->src_samples(kResampleTile)), "LDS limit")) ||
        (b->fmt && hip_failed(gsc_prepare_crop_mix(b->channels,
                                                   b->src_samples(mix_tile_len(b->channels, kResampleTile))),
                              "LDS limit")))
        return nullptr;
    return b.release();
}

int gsc_crop_binding_decode(gsc_crop_binding* b, const long long* crops_device, int ncrops, int dtype, int layout,
                            long long length, void* dst_device, long long* written_device, void* hip_stream) {
    const double t_begin = now_ms();
    gsc_crop_call_stats& stats = t_bstat = gsc_crop_call_stats{};
    if (!b) return set_last_error("gsc_crop_binding_decode: binding is null");
    if (check_pcm_format("gsc_crop_binding_decode", dtype, layout) != 0) return -1;
    if (ncrops < 0 || length < 0) return set_last_error("gsc_crop_binding_decode: invalid argument");
    if (ncrops > 0 && length > 0) {
        if (!crops_device) return set_last_error("gsc_crop_binding_decode: crops_device is null");
        if (!dst_device) return set_last_error("gsc_crop_binding_decode: dst_device is null");
        const int C = b->channels;
        if (length > (int64_t(1) << 40) / (int64_t(ncrops) * C) || length > (int64_t(1) << 40) / b->max_step)
            return set_last_error("gsc_crop_binding_decode: output too large for one call");
        int dev = 0;
        DEC_TRY(hipGetDevice(&dev));
        if (dev != b->device)
            return set_last_error(other_device("gsc_crop_binding_decode: the binding", b->device, dev));
        hipStream_t hs = static_cast<hipStream_t>(hip_stream);
        const int is_float = dtype == GSC_PCM_FLOAT32, planar = layout == GSC_LAYOUT_CT;
        const int64_t* crops = reinterpret_cast<const int64_t*>(crops_device);
        int64_t* written = reinterpret_cast<int64_t*>(written_device);
        // the launch shape comes from the binding alone: no crop is read here
        if (b->fmt) {
            DEC_TRY(gsc_launch_crop_resample_bound(b->streams.p, b->nstreams, crops, ncrops, length, C, is_float, planar,
                                                   b->src_samples(std::min<int64_t>(length, kResampleTile)),
                                                   dst_device, written, hs));
        } else {
            DEC_TRY(gsc_launch_crop_fused_bound(b->streams.p, b->nstreams, crops, ncrops, length, C, is_float, planar,
                                                int(std::min<int64_t>(length, kCropTile)), dst_device, written, hs));
        }
        ++stats.launches;
    }
    stats.host_ms = now_ms() - t_begin;
    return 0;
}

int gsc_crop_binding_mix(gsc_crop_binding* b, const long long* sources_device, int nrows, int nsrc, int dtype,
                         int layout, long long length, void* dst_device, long long* written_device,
                         void* hip_stream) {
    const double t_begin = now_ms();
    gsc_crop_call_stats& stats = t_bstat = gsc_crop_call_stats{};
    if (!b) return set_last_error("gsc_crop_binding_mix: binding is null");
    if (check_pcm_format("gsc_crop_binding_mix", dtype, layout) != 0) return -1;
    if (nrows < 0 || length < 0) return set_last_error("gsc_crop_binding_mix: invalid argument");
    if (nsrc < 1 || nsrc > kMixMaxSources)
        return set_last_error("gsc_crop_binding_mix: " + std::to_string(nsrc) + " sources per row, 1 to " +
                              std::to_string(kMixMaxSources) + " are possible");
    if (nrows > 0 && length > 0) {
        if (!sources_device) return set_last_error("gsc_crop_binding_mix: sources_device is null");
        if (!dst_device) return set_last_error("gsc_crop_binding_mix: dst_device is null");
        const int C = b->channels;
        if (length > (int64_t(1) << 40) / (int64_t(nrows) * C) || length > (int64_t(1) << 40) / b->max_step)
            return set_last_error("gsc_crop_binding_mix: output too large for one call");
        int dev = 0;
        DEC_TRY(hipGetDevice(&dev));
        if (dev != b->device) return set_last_error(other_device("gsc_crop_binding_mix: the binding", b->device, dev));
        // the launch shape comes from the binding alone: no source is read here
        const int64_t tile = std::min<int64_t>(length, mix_tile_len(C, kResampleTile));
        DEC_TRY(gsc_launch_crop_mix(b->streams.p, b->nstreams, reinterpret_cast<const int64_t*>(sources_device), nrows,
                                    nsrc, length, C, dtype == GSC_PCM_FLOAT32, layout == GSC_LAYOUT_CT, b->fmt,
                                    b->fmt ? b->src_samples(tile) : 0, dst_device,
                                    reinterpret_cast<int64_t*>(written_device), static_cast<hipStream_t>(hip_stream)));
        ++stats.launches;
    }
    stats.host_ms = now_ms() - t_begin;
    return 0;
}

void gsc_crop_binding_last_call(gsc_crop_call_stats* s) {
    if (s) *s = t_bstat;
}

int gsc_envelope_layout(const long long* samples, int n, int hop, long long* offsets) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the layout is int64");
    std::string err;
    if (envelope_layout(reinterpret_cast<const int64_t*>(samples), n, hop, reinterpret_cast<int64_t*>(offsets), nullptr,
                        &err) != 0)
        return set_last_error(err);
    return 0;
}

int gsc_crop_binding_envelope(gsc_crop_binding* b, int hop, long long* energy_device, int* peak_device,
                              long long nblocks, void* hip_stream) {
    if (!b) return set_last_error("gsc_crop_binding_envelope: binding is null");
    const int n = b->nstreams;
    // tile0[n + 1], then block0[n + 1], as envelope_kernel reads them
    std::vector<int64_t> layout(2 * (size_t(n) + 1));
    int64_t* tile0 = layout.data();
    int64_t* block0 = tile0 + n + 1;
    std::string err;
    if (envelope_layout(b->samples.data(), n, hop, block0, tile0, &err) != 0) return set_last_error(err);
    if (nblocks != block0[n])
        return set_last_error("gsc_crop_binding_envelope: nblocks " + std::to_string(nblocks) + ", the binding's " +
                              std::to_string(n) + " streams have " + std::to_string(block0[n]) + " blocks of " +
                              std::to_string(hop) + " samples");
    if (n == 0 || nblocks == 0) return 0;
    if (!energy_device) return set_last_error("gsc_crop_binding_envelope: energy_device is null");
    if (!peak_device) return set_last_error("gsc_crop_binding_envelope: peak_device is null");
    int dev = 0;
    DEC_TRY(hipGetDevice(&dev));
    if (dev != b->device)
        return set_last_error(other_device("gsc_crop_binding_envelope: the binding", b->device, dev));
    // once per corpus: the call may ask the runtime where its outputs live
    const std::pair<const void*, const char*> outs[2] = {{energy_device, "energy_device"}, {peak_device, "peak_device"}};
    for (const auto& o : outs)
        if (check_device_memory("gsc_crop_binding_envelope", o.second, o.first, b->device, "the binding") != 0)
            return -1;
    hipStream_t hs = static_cast<hipStream_t>(hip_stream);
    // The layout goes up as the binding's descriptors did: a blocking copy into memory of its own, which has
    // landed when the call launches on whatever stream; the call then waits for that stream before it frees it.
    Dev<int64_t> d_layout;
    DEC_TRY(d_layout.alloc(layout.size()));
    DEC_TRY(hipMemcpy(d_layout.p, layout.data(), layout.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    DEC_TRY(gsc_launch_envelope(b->streams.p, n, d_layout.p, tile0[n], hop, reinterpret_cast<int64_t*>(energy_device),
                                peak_device, nblocks, hs));
    DEC_TRY(hipStreamSynchronize(hs));
    return 0;
}

int gsc_crop_binding_fidelity(gsc_crop_binding* b, int hop, const void* const* ref_device,
                              const long long* ref_samples, long long* err_energy_device,
                              long long* ref_energy_device, int* err_peak_device, long long nblocks, void* hip_stream) {
    const char* who = "gsc_crop_binding_fidelity";
    if (!b) return set_last_error(std::string(who) + ": binding is null");
    const int n = b->nstreams;
    // one upload: tile0[n + 1] and block0[n + 1] as envelope_kernel reads them, then a FidelityRef per stream
    const size_t nlayout = 2 * (size_t(n) + 1);
    std::vector<int64_t> block(nlayout + 2 * size_t(n));
    int64_t* tile0 = block.data();
    int64_t* block0 = tile0 + n + 1;
    std::vector<FidelityRef> refs(static_cast<size_t>(n));
    std::string err;
    if (envelope_layout(b->samples.data(), n, hop, block0, tile0, &err) != 0) return set_last_error(err);
    if (nblocks != block0[n])
        return set_last_error(std::string(who) + ": nblocks " + std::to_string(nblocks) + ", the binding's " +
                              std::to_string(n) + " streams have " + std::to_string(block0[n]) + " blocks of " +
                              std::to_string(hop) + " samples");
    if (n > 0 && !ref_device) return set_last_error(std::string(who) + ": ref_device is null");
    if (n > 0 && !ref_samples) return set_last_error(std::string(who) + ": ref_samples is null");
    if (fidelity_refs(ref_device, reinterpret_cast<const int64_t*>(ref_samples), n, refs.data(), &err) != 0)
        return set_last_error(err);
    if (n == 0 || nblocks == 0) return 0;
    std::memcpy(block.data() + nlayout, refs.data(), refs.size() * sizeof(FidelityRef));
    const std::pair<const void*, const char*> outs[3] = {{err_energy_device, "err_energy_device"},
                                                         {ref_energy_device, "ref_energy_device"},
                                                         {err_peak_device, "err_peak_device"}};
    for (const auto& o : outs)
        if (!o.first) return set_last_error(std::string(who) + ": " + o.second + " is null");
    int dev = 0;
    DEC_TRY(hipGetDevice(&dev));
    if (dev != b->device) return set_last_error(other_device(std::string(who) + ": the binding", b->device, dev));
    // once per corpus: the call may ask the runtime where its outputs and its references live
    for (const auto& o : outs)
        if (check_device_memory(who, o.second, o.first, b->device, "the binding") != 0) return -1;
    for (int i = 0; i < n; ++i)
        if (refs[size_t(i)].pcm && check_device_memory(who, "stream " + std::to_string(i) + ": the reference",
                                                       refs[size_t(i)].pcm, b->device, "the binding") != 0)
            return -1;
    hipStream_t hs = static_cast<hipStream_t>(hip_stream);
    // as the envelope's layout: a blocking copy into memory of the call's own, freed after the stream's work
    Dev<int64_t> d_block;
    DEC_TRY(d_block.alloc(block.size()));
    DEC_TRY(hipMemcpy(d_block.p, block.data(), block.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    DEC_TRY(gsc_launch_fidelity(b->streams.p, n, d_block.p, tile0[n],
                                reinterpret_cast<const FidelityRef*>(d_block.p + nlayout), hop,
                                reinterpret_cast<int64_t*>(err_energy_device),
                                reinterpret_cast<int64_t*>(ref_energy_device), err_peak_device, nblocks, hs));
    DEC_TRY(hipStreamSynchronize(hs));
    return 0;
}

void gsc_crop_binding_free(gsc_crop_binding* b) {
    if (b) free_on_device(b);
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
