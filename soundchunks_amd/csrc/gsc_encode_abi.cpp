// The encode C ABI of include/soundchunks.h: options, prepared encoders
// (gsc_prepare*), the gsc_encode_* entry points, and the drop-in calls
// gsc_frame_dsp and gsc_birch_labels.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <strings.h>
#include <vector>

#include "../../include/soundchunks.h"
#include "fpc_math.h"
#include "gsc_decode.h"
#include "gsc_encode_host.h"
#include "gsc_encoder.h"

using namespace gsc;

// a WAV after Load + PrepareFrames: the frame boundaries of the whole file,
// computed once per job and shared by every frame-range encode (sharding)
struct gsc_prepared {
    Encoder enc;
    double prepare_ms = 0;
    int loaded_begin = 0, loaded_end = -1;  // frames whose samples are held (-1: all)
    explicit gsc_prepared(const gsc_options& o) : enc(o) {}
};

namespace {

int opt_start(int argc, const char* const* argv, const char* pfx) {
    const size_t l = std::strlen(pfx);
    for (int i = 0; i < argc; ++i)
        if (std::strncmp(argv[i], pfx, l) == 0) return i;
    return -1;
}
double opt_value(int argc, const char* const* argv, const char* pfx, double def) {
    const int i = opt_start(argc, argv, pfx);
    if (i < 0) return def;
    const char* s = argv[i] + std::strlen(pfx);
    if (!*s) return def;
    char* end = nullptr;
    const double v = std::strtod(s, &end);
    return (end && !*end) ? v : def;  // StrToFloatDef
}
bool opt_has(int argc, const char* const* argv, const char* p) {
    for (int i = 0; i < argc; ++i)
        if (strcasecmp(argv[i], p) == 0) return true;
    return false;
}

// n elements at src as malloc memory the caller frees with gsc_free (never NULL on success)
template <typename T>
T* to_malloc(const T* src, size_t n) {
    T* p = static_cast<T*>(std::malloc(std::max<size_t>(n, 1) * sizeof(T)));
    if (p && n) std::memcpy(p, src, n * sizeof(T));
    return p;
}

// a gsc_prepared whose encoder `prep` has prepared, or NULL with the error slot set
template <typename Prep>
gsc_prepared* make_prepared(const char* who, const gsc_options& o, Prep prep) {
    const double t0 = now_ms();
    gsc_prepared* p = new (std::nothrow) gsc_prepared(o);
    if (!p) {
        set_last_error(std::string(who) + ": out of host memory");
        return nullptr;
    }
    std::string err;
    if (prep(p->enc, &err) != 0) {
        delete p;
        set_last_error(err);
        return nullptr;
    }
    p->prepare_ms = now_ms() - t0;
    return p;
}

// encode frames [frame_begin, frame_end) of a prepared encoder into a
// library-allocated buffer; timing lands in the timing slot (host_prepare_ms excluded).
// file_bytes: the range's bytes of every file of the batch; frame_bytes: each
// frame's SaveStream bytes (frame_end - frame_begin entries)
// table: the seek table of the returned bytes (with no frames in the range, of no stream: empty)
int encode_prepared(Encoder& enc, int frame_begin, int frame_end, uint8_t** out, size_t* out_len,
                    size_t* file_bytes = nullptr, size_t* frame_bytes = nullptr,
                    std::vector<uint8_t>* table = nullptr) {
    const double t0 = now_ms();
    const int fc = enc.frame_count();
    frame_begin = std::max(0, frame_begin);
    frame_end = std::min(fc, frame_end < 0 ? fc : frame_end);
    std::vector<uint8_t> bytes;
    std::vector<size_t> fb;
    std::string err;
    if (frame_end > frame_begin) {
        if (enc.encode_range(frame_begin, frame_end, &bytes, &err, &last_timing(), nullptr, &fb, table) != 0)
            return set_last_error(err);
    }
    if (file_bytes) {
        const std::vector<int>& ff = enc.file_first();
        for (size_t f = 0; f + 1 < ff.size(); ++f) {
            size_t n = 0;
            for (int i = std::max(ff[f], frame_begin); i < std::min(ff[f + 1], frame_end); ++i)
                n += fb[size_t(i - frame_begin)];
            file_bytes[f] = n;
        }
    }
    if (frame_bytes)
        for (int i = frame_begin; i < frame_end; ++i) frame_bytes[i - frame_begin] = fb[size_t(i - frame_begin)];
    *out = to_malloc(bytes.data(), bytes.size());
    if (!*out) return set_last_error("out of host memory");
    *out_len = bytes.size();
    last_timing().total_ms = now_ms() - t0;
    return 0;
}

// every prepared entry point: a bounds-prepared encoder (gsc_prepare_frames)
// holds only the samples of frames [loaded_begin, loaded_end)
int check_loaded(const gsc_prepared* p, int frame_begin, int frame_end, const char* who) {
    if (p->loaded_end < 0) return 0;
    const int fe = frame_end < 0 ? p->enc.frame_count() : std::min(frame_end, p->enc.frame_count());
    const int fb = std::max(0, frame_begin);
    if (fe > fb && (fb < p->loaded_begin || fe > p->loaded_end))
        return set_last_error(std::string(who) + ": frames outside the range gsc_prepare_frames loaded");
    return 0;
}

}  // namespace

extern "C" {

void gsc_default_options(gsc_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->bit_rate = -1;
    o->precision = 3;
    o->low_cut = 0.0;
    o->high_cut = 24000.0;
    o->chunk_bit_depth = 8;
    o->chunk_size = 4;
    o->chunks_per_frame = 4096;
    o->reduce_bass_band = 1;
    o->vfr = 1.0;
    o->chunk_blend = 0;
    o->frame_length = 4000.0;
}

void gsc_parse_options(gsc_options* o, int argc, const char* const* argv) {
    auto clampi = [](int64_t v, int64_t lo, int64_t hi) { return int(std::min(hi, std::max(lo, v))); };
    o->bit_rate = int(fpc::round(opt_value(argc, argv, "-br", o->bit_rate)));
    o->precision = int(fpc::round(opt_value(argc, argv, "-pr", o->precision)));
    o->low_cut = opt_value(argc, argv, "-lc", o->low_cut);
    o->high_cut = opt_value(argc, argv, "-hc", o->high_cut);
    o->vfr = std::min(1.0, std::max(0.0, opt_value(argc, argv, "-vfr", o->vfr)));
    o->frame_length = std::max(opt_value(argc, argv, "-fl", o->frame_length), 1.0);
    o->chunk_bit_depth = clampi(fpc::round(opt_value(argc, argv, "-cbd", o->chunk_bit_depth)), 1, 16);
    o->chunk_size = int(fpc::round(opt_value(argc, argv, "-cs", o->chunk_size)));
    o->chunks_per_frame = clampi(fpc::round(opt_value(argc, argv, "-cpf", o->chunks_per_frame)), 256, 4096);
    o->verbose = opt_has(argc, argv, "-v");
    o->reduce_bass_band = !opt_has(argc, argv, "-pbb");
    o->chunk_blend = clampi(fpc::round(opt_value(argc, argv, "-cb", o->chunk_blend)), 0, o->chunk_size / 2);
    o->python_reduce = opt_has(argc, argv, "-py");
}

int gsc_count_frames(const uint8_t* wav, size_t wav_len, const gsc_options* o, int* frame_count) {
    Encoder enc(*o);
    std::string err;
    if (enc.prepare(wav, wav_len, &err) != 0) return set_last_error(err);
    *frame_count = enc.frame_count();
    return 0;
}

int gsc_encode_wav_frames(const uint8_t* wav, size_t wav_len, const gsc_options* o, int frame_begin, int frame_end,
                          uint8_t** out, size_t* out_len, int* frame_count) {
    const double t0 = now_ms();
    last_timing() = gsc_timing{};
    Encoder enc(*o);
    std::string err;
    if (enc.prepare(wav, wav_len, &err) != 0) return set_last_error(err);
    const double t1 = now_ms();
    if (frame_count) *frame_count = enc.frame_count();
    if (encode_prepared(enc, frame_begin, frame_end, out, out_len) != 0) return -1;
    last_timing().host_prepare_ms = t1 - t0;
    last_timing().total_ms = now_ms() - t0;
    return 0;
}

gsc_prepared* gsc_prepare(const uint8_t* wav, size_t wav_len, const gsc_options* o) {
    if (!wav || !o) {
        set_last_error("gsc_prepare: null argument");
        return nullptr;
    }
    return make_prepared("gsc_prepare", *o, [&](Encoder& e, std::string* err) { return e.prepare(wav, wav_len, err); });
}

int gsc_prepared_frame_count(const gsc_prepared* p) { return p ? p->enc.frame_count() : -1; }

int gsc_prepared_frame_chunks(const gsc_prepared* p, int* chunks) {
    if (!p || !chunks) return set_last_error("gsc_prepared_frame_chunks: null argument");
    for (int i = 0; i < p->enc.frame_count(); ++i) chunks[i] = p->enc.frame_chunks(i);
    return 0;
}

int gsc_prepared_frame_bounds(const gsc_prepared* p, int* starts, int* ends) {
    if (!p || !starts || !ends) return set_last_error("gsc_prepared_frame_bounds: null argument");
    const auto& s = p->enc.frame_starts();
    const auto& e = p->enc.frame_ends();
    std::copy(s.begin(), s.end(), starts);
    std::copy(e.begin(), e.end(), ends);
    return 0;
}

gsc_prepared* gsc_prepare_frames(const uint8_t* wav, size_t wav_len, const gsc_options* o, const int* starts,
                                 const int* ends, int frame_count, int frame_begin, int frame_end) {
    if (!wav || !o || !starts || !ends) {
        set_last_error("gsc_prepare_frames: null argument");
        return nullptr;
    }
    if (frame_end < 0) frame_end = frame_count;
    gsc_prepared* p = make_prepared("gsc_prepare_frames", *o, [&](Encoder& e, std::string* err) {
        return e.prepare_bounds(wav, wav_len, starts, ends, frame_count, frame_begin, frame_end, err);
    });
    if (p) {
        p->loaded_begin = frame_begin;
        p->loaded_end = frame_end;
    }
    return p;
}

gsc_prepared* gsc_prepare_many(const uint8_t* const* wavs, const size_t* lens, int nfiles, const gsc_options* o) {
    if (!wavs || !lens || !o || nfiles <= 0) {
        set_last_error("gsc_prepare_many: invalid argument");
        return nullptr;
    }
    return make_prepared("gsc_prepare_many", *o,
                         [&](Encoder& e, std::string* err) { return e.prepare_many(wavs, lens, nfiles, err); });
}

int gsc_encode_prepared(gsc_prepared* p, int frame_begin, int frame_end, uint8_t** out, size_t* out_len) {
    return gsc_encode_prepared_frames(p, frame_begin, frame_end, out, out_len, nullptr);
}

int gsc_encode_prepared_frames(gsc_prepared* p, int frame_begin, int frame_end, uint8_t** out, size_t* out_len,
                               size_t* frame_bytes) {
    if (!p || !out || !out_len) return set_last_error("gsc_encode_prepared: null argument");
    if (check_loaded(p, frame_begin, frame_end, "gsc_encode_prepared") != 0) return -1;
    last_timing() = gsc_timing{};
    if (encode_prepared(p->enc, frame_begin, frame_end, out, out_len, nullptr, frame_bytes) != 0) return -1;
    last_timing().host_prepare_ms = 0;  // paid once, in gsc_prepare
    return 0;
}

int gsc_encode_prepared_with_table(gsc_prepared* p, int frame_begin, int frame_end, uint8_t** out, size_t* out_len,
                                   uint8_t** table, size_t* table_len) {
    if (!p || !out || !out_len || !table || !table_len)
        return set_last_error("gsc_encode_prepared_with_table: null argument");
    if (p->enc.file_first().size() != 2)
        return set_last_error(
            "gsc_encode_prepared_with_table: a batch of files has no single table; index each file's bytes");
    if (check_loaded(p, frame_begin, frame_end, "gsc_encode_prepared_with_table") != 0) return -1;
    last_timing() = gsc_timing{};
    std::vector<uint8_t> t;
    *table = nullptr;
    if (encode_prepared(p->enc, frame_begin, frame_end, out, out_len, nullptr, nullptr, &t) != 0) return -1;
    last_timing().host_prepare_ms = 0;  // paid once, in gsc_prepare
    *table = to_malloc(t.data(), t.size());
    if (!*table) {
        std::free(*out);
        *out = nullptr;
        return set_last_error("out of host memory");
    }
    *table_len = t.size();
    return 0;
}

int gsc_encode_prepared_files_with_tables(gsc_prepared* p, int frame_begin, int frame_end, uint8_t** out,
                                          size_t* out_len, size_t* file_bytes, uint8_t** tables, size_t* tables_len,
                                          size_t* table_bytes) {
    if (!p || !out || !out_len || !file_bytes || !tables || !tables_len || !table_bytes)
        return set_last_error("gsc_encode_prepared_files_with_tables: null argument");
    if (check_loaded(p, frame_begin, frame_end, "gsc_encode_prepared_files_with_tables") != 0) return -1;
    last_timing() = gsc_timing{};
    std::vector<uint8_t> t;
    if (encode_prepared(p->enc, frame_begin, frame_end, out, out_len, file_bytes, nullptr, &t) != 0) return -1;
    last_timing().host_prepare_ms = 0;  // paid once, in gsc_prepare
    // the range's table, cut at the files' byte counts and rebased to each file's first byte
    const int nfiles = int(p->enc.file_first().size()) - 1;
    std::vector<std::vector<uint8_t>> per;
    std::string err;
    if (t.empty()) {
        per.assign(size_t(nfiles), std::vector<uint8_t>());
    } else if (index_table_split(*out, *out_len, t.data(), t.size(), file_bytes, nfiles, &per, &err) != 0) {
        std::free(*out);
        *out = nullptr;
        return set_last_error(err);
    }
    std::vector<uint8_t> all;
    for (int f = 0; f < nfiles; ++f) {
        all.insert(all.end(), per[size_t(f)].begin(), per[size_t(f)].end());
        table_bytes[f] = per[size_t(f)].size();
    }
    *tables = to_malloc(all.data(), all.size());
    if (!*tables) {
        std::free(*out);
        *out = nullptr;
        return set_last_error("out of host memory");
    }
    *tables_len = all.size();
    return 0;
}

double gsc_prepared_prepare_ms(const gsc_prepared* p) { return p ? p->prepare_ms : 0.0; }

int gsc_prepared_file_count(const gsc_prepared* p) { return p ? int(p->enc.file_first().size()) - 1 : -1; }

int gsc_prepared_file_frames(const gsc_prepared* p, int* first_frame) {
    if (!p || !first_frame) return set_last_error("gsc_prepared_file_frames: null argument");
    const auto& ff = p->enc.file_first();
    std::copy(ff.begin(), ff.end(), first_frame);
    return 0;
}

int gsc_encode_prepared_files(gsc_prepared* p, int frame_begin, int frame_end, uint8_t** out, size_t* out_len,
                              size_t* file_bytes) {
    if (!p || !out || !out_len || !file_bytes) return set_last_error("gsc_encode_prepared_files: null argument");
    if (check_loaded(p, frame_begin, frame_end, "gsc_encode_prepared_files") != 0) return -1;
    last_timing() = gsc_timing{};
    if (encode_prepared(p->enc, frame_begin, frame_end, out, out_len, file_bytes) != 0) return -1;
    return 0;
}

void gsc_prepared_free(gsc_prepared* p) { delete p; }

int gsc_frame_dsp(const uint8_t* wav, size_t wav_len, const gsc_options* o, int frame, int* atten_div, float** feat,
                  int* n_chunks) {
    Encoder enc(*o);
    std::string err;
    if (enc.prepare(wav, wav_len, &err) != 0) return set_last_error(err);
    std::vector<float> f;
    if (enc.dsp_frame(frame, atten_div, &f, &err) != 0) return set_last_error(err);
    *n_chunks = int(f.size() / size_t(2 * o->chunk_size));
    *feat = to_malloc(f.data(), f.size());
    return 0;
}

int gsc_encode_wav(const uint8_t* wav, size_t wav_len, const gsc_options* o, uint8_t** out, size_t* out_len) {
    return gsc_encode_wav_frames(wav, wav_len, o, 0, -1, out, out_len, nullptr);
}

int gsc_encode_wav_recon(const uint8_t* wav, size_t wav_len, const gsc_options* o, uint8_t** out, size_t* out_len,
                         int16_t** recon, size_t* recon_len, double* psy_a_delta) {
    if (!wav || !o || !out || !out_len || !recon || !recon_len || !psy_a_delta)
        return set_last_error("gsc_encode_wav_recon: null argument");
    *out = nullptr;
    *recon = nullptr;
    gsc_timing& tim = last_timing();
    tim = gsc_timing{};
    const double t0 = now_ms();
    Encoder enc(*o);
    std::string err;
    if (enc.prepare(wav, wav_len, &err) != 0) return set_last_error(err);
    tim.host_prepare_ms = now_ms() - t0;
    const int ch = enc.channels();
    const size_t n = size_t(enc.sample_count()) * size_t(ch);
    ReconOut ro;
    ro.pcm = static_cast<int16_t*>(std::calloc(std::max<size_t>(n, 1), sizeof(int16_t)));
    if (!ro.pcm) return set_last_error("out of host memory");
    ro.wav = wav;
    ro.wav_len = wav_len;
    std::vector<uint8_t> bytes;
    const int fc = enc.frame_count();
    if (fc > 0 && enc.encode_range(0, fc, &bytes, &err, &tim, &ro) != 0) {
        std::free(ro.pcm);
        return set_last_error(err);
    }
    *out = to_malloc(bytes.data(), bytes.size());
    if (!*out) {
        std::free(ro.pcm);
        return set_last_error("out of host memory");
    }
    *out_len = bytes.size();
    // ComputePsyADelta = CompareEuclidean over Double copies (encoder.lpr:1803-1814,1862-1880): every
    // partial sum is an integer, exact in f64 below 2^53, where it equals the device's exact sum
    double acc = 0.0;
    if (ro.sq < (1ull << 53)) {
        acc = double(ro.sq);
    } else {  // the reference's sequential f64 sum, channel-major
        const size_t psc = wav_len >= 44 ? (wav_len - 44) / (2 * size_t(ch)) : 0;
        for (int j = 0; j < ch; ++j)
            for (size_t i = 0; i < size_t(enc.sample_count()); ++i) {
                int16_t sv = 0;
                if (i < psc) std::memcpy(&sv, wav + 44 + (i * ch + j) * 2, 2);
                const double d = double(sv) - double(ro.pcm[i * ch + j]);
                acc += d * d;
            }
    }
    *psy_a_delta = n ? std::sqrt(acc / double(n)) : 0.0;
    *recon = ro.pcm;
    *recon_len = n;
    tim.total_ms = now_ms() - t0;
    return 0;
}

int gsc_birch_labels(int n, int d, const float* x, int k, int* labels) {
    if (!x || !labels || n <= 0 || d <= 0 || k <= 0) return set_last_error("gsc_birch_labels: invalid argument");
    if (require_device() != 0) return -1;
    std::string err;
    if (birch_reduce_labels(n, d, x, k, labels, &err) != 0) return set_last_error(err);
    return 0;
}

}  // extern "C"
