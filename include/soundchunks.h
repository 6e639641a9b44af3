/*
 * soundchunks_amd -- MI355X-native SoundChunks encode hot path, C ABI.
 *
 * Two layers, both plain C (pointers + sizes, no torch types):
 *
 * 1. The drop-in boundary: exactly the numeric-library surface the reference
 *    binds in encoder/extern.pas:112-123 (yakmo_single.dll + ANN.dll).  On
 *    x86-64 Linux stdcall/cdecl collapse to the SysV ABI.
 *      yakmo_create / yakmo_destroy / yakmo_load_train_data /
 *      yakmo_train_on_data / yakmo_get_centroids    -> extern.pas:112-116
 *      ann_kdtree_create / ann_kdtree_destroy / ann_kdtree_search /
 *      ann_kdtree_pri_search / ann_kdtree_search_multi /
 *      ann_kdtree_pri_search_multi                   -> extern.pas:118-123
 *    Data layout is the reference's: 2-D arrays are float** row-pointer
 *    arrays; ann_kdtree_* keep the caller's row pointers and read the
 *    *current* point values at every search (encoder.lpr:729-745 mutates
 *    centroids between searches of one tree).  All arithmetic runs on the GPU.
 *
 * 2. Frame-level batched entry points (gsc_*): the per-query ANN ABI costs
 *    one host<->device round trip per search, so the encoder itself calls
 *    these, which own the whole Reduce (yakmo + KNNScanReduce) and KNNFit
 *    loops of many frames in one launch each.
 *
 * Errors: functions returning int return 0 on success, <0 on failure;
 * gsc_last_error() describes the last failure of the calling thread.  There is
 * no CPU fallback: without a usable gfx950 device every compute call fails.
 */
#ifndef SOUNDCHUNKS_AMD_H
#define SOUNDCHUNKS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- extern.pas:112-116 (yakmo_single.dll) ----------------------------- */
typedef struct yakmo_t yakmo_t;
/* replaces yakmo_single.dll!yakmo_create @0x180003230 (extern.pas:112) */
yakmo_t *yakmo_create(unsigned int k, unsigned int restartCount, int maxIter, int initType, int initSeed,
                      int doNormalize, int isVerbose);
/* replaces yakmo_destroy @0x180003340 (extern.pas:113) */
void yakmo_destroy(yakmo_t *ay);
/* replaces yakmo_load_train_data @0x180003430 (extern.pas:114); copies rows */
void yakmo_load_train_data(yakmo_t *ay, unsigned int rowCount, unsigned int colCount, float **dataset);
/* replaces yakmo_train_on_data @0x1800034b0 (extern.pas:115); writes labels */
void yakmo_train_on_data(yakmo_t *ay, int *pointToCluster);
/* replaces yakmo_get_centroids @0x180003510 (extern.pas:116) */
void yakmo_get_centroids(yakmo_t *ay, float **centroids);

/* ---- extern.pas:118-123 (ANN.dll) -------------------------------------- */
typedef struct ann_kdtree_t ann_kdtree_t;
/* replaces ANN.dll!ann_kdtree_create @0x180003c50 (extern.pas:118); split 0 = ANN_KD_STD */
ann_kdtree_t *ann_kdtree_create(float **pa, int n, int dd, int bs, int split);
/* replaces ann_kdtree_destroy @0x180003cb0 (extern.pas:119) */
void ann_kdtree_destroy(ann_kdtree_t *akd);
/* replaces ann_kdtree_search @0x180003cd0 (extern.pas:120): k = 1, returns index */
int ann_kdtree_search(ann_kdtree_t *akd, float *q, float eps, float *err);
/* replaces ann_kdtree_pri_search @0x180003d30 (extern.pas:121) */
int ann_kdtree_pri_search(ann_kdtree_t *akd, float *q, float eps, float *err);
/* replaces ann_kdtree_search_multi @0x180003d90 (extern.pas:122) */
void ann_kdtree_search_multi(ann_kdtree_t *akd, int *idxs, float *errs, int cnt, float *q, float eps);
/* replaces ann_kdtree_pri_search_multi @0x180003db0 (extern.pas:123) */
void ann_kdtree_pri_search_multi(ann_kdtree_t *akd, int *idxs, float *errs, int cnt, float *q, float eps);

/* ---- frame-level batched entry points ---------------------------------- */
/* TEncoder options (encoder.lpr:1486-1509, 1985-1998) */
typedef struct {
    int bit_rate;         /* -br, default -1 */
    int precision;        /* -pr, default 3 */
    double low_cut;       /* -lc, default 0 (band-pass filtering unsupported) */
    double high_cut;      /* -hc, default 24000 */
    int chunk_bit_depth;  /* -cbd, default 8 (8 or 12) */
    int chunk_size;       /* -cs, default 4 (1 .. 16) */
    int chunks_per_frame; /* -cpf, default 4096, clamped [256, 4096] */
    int reduce_bass_band; /* !-pbb, default 1 */
    double vfr;           /* -vfr, default 1.0 */
    int chunk_blend;      /* -cb, default 0 (only 0 supported) */
    double frame_length;  /* -fl, default 4000 ms */
    int python_reduce;    /* -py: cluster.py's Birch reducer instead of yakmo + KNNScanReduce */
    int verbose;          /* -v */
} gsc_options;

void gsc_default_options(gsc_options *o);
/* encoder.lpr argv semantics (prefix match, values glued to the flag) */
void gsc_parse_options(gsc_options *o, int argc, const char *const *argv);

/* Whole-file encode: in-memory WAV (44-byte header + PCM16) -> .gsc bytes.
 * *out is allocated by the library; release with gsc_free(). */
int gsc_encode_wav(const uint8_t *wav, size_t wav_len, const gsc_options *o, uint8_t **out, size_t *out_len);

/* Encode plus the reconstruction the reference builds after MakeFrames
 * (encoder.lpr:2019-2031: TEncoder.MakeDstData, ComputePsyADelta, SaveWAV):
 * *recon = the 16-bit signal the .gsc encodes, interleaved [sample][channel]
 * over the padded SampleCount (*recon_len samples; free with gsc_free), as
 * TEncoder.SaveWAV writes it (encoder.lpr:1154-1179); *psy_a_delta =
 * ComputePsyADelta(srcData, dstData) (encoder.lpr:1862-1880).  Reconstruction
 * and the PsyADelta sum run on the device. */
int gsc_encode_wav_recon(const uint8_t *wav, size_t wav_len, const gsc_options *o, uint8_t **out, size_t *out_len,
                         int16_t **recon, size_t *recon_len, double *psy_a_delta);
/* Frame-range encode (multi-GPU sharding): runs the host pre-pass on the
 * whole file, encodes frames [frame_begin, frame_end) only and returns their
 * concatenated TFrame.SaveStream bytes; *frame_count = total frame count. */
int gsc_encode_wav_frames(const uint8_t *wav, size_t wav_len, const gsc_options *o, int frame_begin, int frame_end,
                          uint8_t **out, size_t *out_len, int *frame_count);
int gsc_count_frames(const uint8_t *wav, size_t wav_len, const gsc_options *o, int *frame_count);

/* Prepared WAV: TEncoder.Load + PrepareFrames (encoder.lpr:1111-1152,
 * 1294-1429) run once per job; the frame boundaries of the whole file are then
 * shared by every frame-range encode of that job (one rank per GPU encodes its
 * range without rescanning the file).  gsc_prepare returns NULL on failure
 * (gsc_last_error).  gsc_prepared_frame_chunks writes the chunkRefs count
 * (chunks x channels) of every frame: the weights of the LPT frame sharding. */
typedef struct gsc_prepared gsc_prepared;
gsc_prepared *gsc_prepare(const uint8_t *wav, size_t wav_len, const gsc_options *o);
int gsc_prepared_frame_count(const gsc_prepared *p);
int gsc_prepared_frame_chunks(const gsc_prepared *p, int *chunks);
int gsc_encode_prepared(gsc_prepared *p, int frame_begin, int frame_end, uint8_t **out, size_t *out_len);
/* gsc_encode_prepared, plus each frame's share of the returned bytes.  The
 * range is clamped first (as in gsc_encode_prepared): b = max(frame_begin, 0),
 * e = frame_end < 0 ? frame_count : min(frame_end, frame_count); frame_bytes
 * receives max(e - b, 0) entries, frame_bytes[i - b] for frame i.  A .gsc is
 * the concatenation of its frames' TFrame.SaveStream bytes
 * (encoder.lpr:980-1107, 1181-1215), so the caller can split it per frame
 * (bench.py's per-frame bit-exactness digests).  Every prepared entry point
 * refuses frames outside the range a gsc_prepare_frames handle loaded. */
int gsc_encode_prepared_frames(gsc_prepared *p, int frame_begin, int frame_end, uint8_t **out, size_t *out_len,
                               size_t *frame_bytes);
double gsc_prepared_prepare_ms(const gsc_prepared *p);
/* The frame boundaries PrepareFrames chose: sample index of every frame's
 * first and last sample (gsc_prepared_frame_count entries each). */
int gsc_prepared_frame_bounds(const gsc_prepared *p, int *starts, int *ends);
/* A prepared encoder over boundaries computed elsewhere (one rank runs
 * PrepareFrames on the whole file and broadcasts them): no power scans, and
 * only the samples of frames [frame_begin, frame_end) are loaded, so only
 * that range may be encoded.  frame_end = -1: up to frame_count.  The bounds
 * must be contiguous, block-aligned and cover the file (else NULL). */
gsc_prepared *gsc_prepare_frames(const uint8_t *wav, size_t wav_len, const gsc_options *o, const int *starts,
                                 const int *ends, int frame_count, int frame_begin, int frame_end);
void gsc_prepared_free(gsc_prepared *p);

/* Batch of WAVs as one job (the reference encodes a corpus file by file;
 * encoder.lpr:1431-1451 runs each file's frames on its thread pool): every
 * file gets its own Load + PrepareFrames, then the frames of ALL files form
 * one frame list, so every stage runs one device launch for the whole batch.
 * The files must share channel count, sample rate and the resulting
 * ChunksPerFrame.  A gsc_prepare / gsc_prepare_frames handle is one file
 * (file_count 1).  gsc_prepared_file_frames writes file_count + 1 entries: the
 * first frame of every file, then the total.  gsc_encode_prepared_files
 * encodes frames [frame_begin, frame_end) of the list and also writes, per
 * file, how many of the returned bytes belong to it (files in order; a file's
 * .gsc is its bytes from every range, in range order). */
gsc_prepared *gsc_prepare_many(const uint8_t *const *wavs, const size_t *wav_lens, int file_count,
                               const gsc_options *o);
int gsc_prepared_file_count(const gsc_prepared *p);
int gsc_prepared_file_frames(const gsc_prepared *p, int *first_frame);
int gsc_encode_prepared_files(gsc_prepared *p, int frame_begin, int frame_end, uint8_t **out, size_t *out_len,
                              size_t *file_bytes);

/* Device DSP of one frame (FindAttenuationDivider, encoder.lpr:566-605, and the
 * MakeChunks features, encoder.lpr:467-485): *feat = n_chunks x 2*ChunkSize
 * floats, allocated by the library (gsc_free).  Parity tests. */
int gsc_frame_dsp(const uint8_t *wav, size_t wav_len, const gsc_options *o, int frame, int *atten_div, float **feat,
                  int *n_chunks);

/* Stage entry points on host buffers (row-major), used by parity tests. */
int gsc_yakmo_seed_means(int n, int d, const float *x, int k, float *centroids);
/* The same for nf frames in one launch, an n and a k per frame: x, centroids
 * and labels (the seeding assignment; may be NULL) hold the frames' arrays one
 * after another (ns[i] x d, ks[i] x d, ns[i]). */
int gsc_yakmo_seed_means_frames(int nf, int d, const int *ns, const float *x, const int *ks, float *centroids,
                                int *labels);
int gsc_scan_reduce(int n, int d, const float *x, int k, float *centroids, int *clusters, int precision, int *iters);
/* -py reducer stage (cluster.py Birch labels, extern.pas:350-437): n x d
 * Single features of one frame -> labels[n] in [0, k). */
int gsc_birch_labels(int n, int d, const float *x, int k, int *labels);
int gsc_knnfit_assign(int r, int cs, const float *cand_fwd, int n, const float *q, float eps, int *best);
/* The same for nf frames in one launch, an r, an n and an eps per frame:
 * cand_fwd, q and best hold the frames' arrays one after another (rs[i] x cs,
 * ns[i] x cs, ns[i]).  overflow[i] (may be NULL) is the number of frame i's
 * queries whose tie set exceeded the 64-NN bucket (answered by the ANN replay). */
int gsc_knnfit_assign_frames(int nf, int cs, const int *rs, const float *cand_fwd, const int *ns, const float *q,
                             const float *eps, int *best, int *overflow);
/* yakmo's prefix-chain fast path (gsc_yakmo.hip chain_fast, ppl = 8 or 16
 * points per lane) on 64*nbk points from *run: the accepted block count, the
 * run after them, and per accepted block the checkpoint / min / max of the
 * running f32 total (the DLL's sequential cum[], App. C.1).  Parity tests. */
int gsc_yakmo_chain_test(int ppl, const float *pts, int nbk, float run, int *accepted, float *run_out, float *ck,
                         float *bmn, float *bmx);

/* Timing of the last gsc_encode_* call on the calling thread (milliseconds),
 * split per stage, plus average device time per launch of each kernel. */
typedef struct {
    double host_prepare_ms, host_frames_ms, gpu_yakmo_ms, gpu_scan_ms, gpu_knnfit_ms, host_post_ms, total_ms;
    int frames, reduce_frames;
    long long points, scan_passes, scan_slow;
    long long scan_point_passes; /* sum over frames of passes * N (searches) */
    long long knnfit_pairs;      /* sum over frames of N * 4R (query x candidate) */
    int scan_launches, knnfit_launches;
    long long scan_restarts;     /* batched KNNScanReduce pipeline restarts */
    double gpu_dsp_ms;           /* device DSP incl. sample upload (attenuation divider, features) */
    double post_overlap_ms;      /* KNNFit + prune/sort + packing run while other frames were still scanning */
    int post_groups;             /* frame groups the post-processing pipeline ran */
    double gpu_recon_ms;         /* gsc_encode_wav_recon only: reconstruction + PsyADelta sum */
    long long knnfit_overflow;   /* queries whose tie set exceeded the 64-NN bucket (ANN replay) */
} gsc_timing;
void gsc_last_timing(gsc_timing *t);

/* ---- decode: .gsc bytes -> PCM16 (decoder/decoder.lpr:37-220) ------------ */
/* The index of a stream: one sequential host pass over the bytes (frame k + 1
 * starts where frame k's bitstream ends; a symbol's bit offset depends on
 * every earlier symbol of its frame).  It records every frame's offsets and
 * fields, a checkpoint (bit offset, header state) every
 * gsc_decode_checkpoint_symbols() symbols, and the per-frame CAttrLookup and
 * codebook tables, and it validates everything: a truncated frame,
 * ChunkBlend != 0, a ChunkBitDepth other than 8 / 12, ChunkSize 0, a symbol
 * that needs bits past the end, a chunk index >= ChunkCount, or a frame whose
 * ChannelCount / SampleRate differ from frame 0 are refused (NULL / <0 and
 * gsc_last_error), never a fault.  Host only: works without a GPU. */
typedef struct gsc_index gsc_index;
gsc_index *gsc_index_create(const uint8_t *gsc, size_t len);
int gsc_index_frame_count(const gsc_index *ix);
int gsc_index_info(const gsc_index *ix, int *channels, int *sample_rate, long long *samples_per_channel);
/* per frame (any pointer may be NULL): byte_offset and first_sample (per
 * channel) receive frame_count + 1 entries, the last one the stream's length
 * and its sample count; the others frame_count entries */
int gsc_index_frames(const gsc_index *ix, size_t *byte_offset, int *frame_length, int *chunk_size, int *chunk_count,
                     long long *first_sample);
void gsc_index_free(gsc_index *ix);
int gsc_decode_checkpoint_symbols(void);
/* Where per-channel sample position `sample` in [0, samples) lives (any
 * pointer may be NULL): the frame that contains it (frames of FrameLength 0
 * contain nothing and are skipped), the symbol row inside that frame,
 * (sample - first_sample) / ChunkSize, the position inside the chunk, and the
 * index of the checkpoint the row's first symbol belongs to, counted over the
 * whole stream: cp_first + row * ChannelCount / checkpoint_symbols.  A
 * position outside [0, samples) is refused (<0 and gsc_last_error).  Host only. */
int gsc_index_locate(const gsc_index *ix, long long sample, int *frame, long long *row, int *within,
                     long long *checkpoint);

/* Frames [frame_begin, frame_end) (clamped; frame_end = -1: to the end) of an
 * indexed stream -> PCM16 interleaved [sample][channel]: *pcm_len int16 values
 * in *pcm (release with gsc_free).  The symbols are unpacked and the samples
 * synthesised on the device, all frames in one launch per stage.  Ranks of a
 * multi-GPU decode split the frames by first_sample. */
int gsc_decode_indexed(const uint8_t *gsc, size_t len, const gsc_index *ix, int frame_begin, int frame_end,
                       int16_t **pcm, size_t *pcm_len);
/* index + decode of a whole stream */
int gsc_decode(const uint8_t *gsc, size_t len, int16_t **pcm, size_t *pcm_len, int *channels, int *sample_rate);
/* A batch of streams as one job (one launch per stage for all frames of all
 * files; they must share ChannelCount and SampleRate): *pcm holds the files'
 * samples back to back, file_samples[i] int16 values each. */
int gsc_decode_many(const uint8_t *const *gscs, const size_t *lens, int file_count, int16_t **pcm,
                    size_t *file_samples, int *channels, int *sample_rate);

/* ---- resident streams: sample ranges into device memory --------------------- */
/* gsc_stream_open walks the stream (as gsc_index_create) and uploads, once, the
 * byte slab, the checkpoints, the int16 codebooks, the attenuations and the
 * frame table to the calling thread's device, where they stay until
 * gsc_stream_free (which first waits for the device's queued work).  NULL and
 * gsc_last_error on a malformed stream or without a device. */
typedef struct gsc_stream gsc_stream;
gsc_stream *gsc_stream_open(const uint8_t *gsc, size_t len);
void gsc_stream_free(gsc_stream *st);
int gsc_stream_info(const gsc_stream *st, int *channels, int *sample_rate, long long *samples_per_channel,
                    int *frames);
/* the index inside (owned by the stream; do not free) */
const gsc_index *gsc_stream_index(const gsc_stream *st);
/* the HIP device the stream's memory lives on (a caller checks its output
 * buffer against it; gsc_decode_crops refuses a stream of another device) */
int gsc_stream_device(const gsc_stream *st);

/* `count` samples per channel from position `begin` of streams[stream] */
typedef struct {
    int stream;
    long long begin;
    long long count;
} gsc_crop;
enum { GSC_PCM_INT16 = 0, GSC_PCM_FLOAT32 = 1 };  /* float32 = int16 * 2^-15, exact */
enum { GSC_LAYOUT_TC = 0, GSC_LAYOUT_CT = 1 };    /* [B][T][C] interleaved, [B][C][T] planar; T = length */
/* Crop i fills row i of dst_device (device memory of ncrops * length *
 * channels elements of `dtype` in `layout`).  A crop that runs past the end of
 * its stream is clipped there: written[i] (may be NULL) is the clipped length,
 * and the rest of the row up to `length` is zero.  Refused, with nothing
 * launched (<0 and gsc_last_error): begin < 0, begin > samples, count < 0,
 * count > length, a stream index outside [0, nstreams), streams whose channel
 * counts differ, a NULL dst_device, an unknown dtype or layout, a stream of
 * more than 2^40 samples per channel or a length of more than 2^40 (both "too
 * long for one call", whatever the crops), and a stream that lives on another
 * device than the calling thread's.  Streams may differ
 * in sample rate, ChunkSize and bit depth.  All crops run in one launch
 * (unpack of the checkpoint segments the crops touch and synthesis, fused),
 * enqueued on hip_stream (a hipStream_t; NULL: the default stream) and ordered
 * with it: the call contains no device synchronisation and copies no sample
 * to the host.  It uploads only its job descriptors and has no other scratch:
 * that one block is allocated and freed in stream order, so calls on
 * different streams share nothing.
 * The descriptors are uploaded with hipMemcpyAsync from pageable memory: the
 * runtime stages a copy that small (about 100 bytes per crop), but where it
 * cannot, HIP may complete the copy before returning, and the call then waits
 * for the work queued earlier on hip_stream (never for other streams).
 * written[] is filled only when everything was enqueued. */
int gsc_decode_crops(gsc_stream *const *streams, int nstreams, const gsc_crop *crops, int ncrops, int dtype,
                     int layout, long long length, void *dst_device, void *hip_stream, long long *written);
/* [begin, begin + count) of one stream -> count * channels int16 in host
 * memory `pcm`, interleaved: the crop decode into device scratch and one
 * download.  The range must lie inside the stream. */
int gsc_stream_decode_samples(gsc_stream *st, long long begin, long long count, int16_t *pcm);

/* ---- crops at a common sample rate and channel count -------------------------- */
/* gsc_decode_crops with an output format: every row of the batch comes out at
 * out_rate and with out_channels channels, whatever its stream's own.
 * out_rate 0: no resampling, every stream keeps its rate; out_channels 0: the
 * streams' count, which must then agree as in gsc_decode_crops.
 *
 * Units.  A crop's `begin` stays in source samples of its stream; `count` and
 * `length` are output samples at out_rate.  With Fi the stream's rate, Fo =
 * out_rate, g = gcd(Fi, Fo), L = Fo / g (the phases) and M = Fi / g, output n
 * of a crop sits at source position (begin L + n M) / L: i0 its floor, phase
 * p = (begin L + n M) mod L, in 64-bit integers.  The crop is clipped at the
 * first n whose position is >= the stream's samples: written[i] = min(count,
 * ceil((samples - begin) L / M)); the rest of the row is zero.  Source samples
 * outside [0, samples) read as zero in the filter, those before `begin` are
 * read from the stream: a crop is a slice of the resampled stream.
 *
 * Filter.  A windowed sinc under the exact Blackman window w(u) = 7938/18608 +
 * 9240/18608 cos(pi u) + 1430/18608 cos(2 pi u) on |u| <= 1, 0 outside.  rho =
 * min(1, Fo / Fi), Z = 16 zero crossings per side, W = Z / rho, T = ceil(W).
 * Tap k in [-T + 1, T] of phase p has d = k - p / L and the ideal value h =
 * rho sinc(rho d) w(d / W), sinc(x) = sin(pi x) / (pi x).  Per phase, in f64 on
 * the host: c_k = round-half-even(2^24 h_k / sum_k h_k), then the remainder
 * 2^24 - sum c_k is added to the tap of largest |h| (lowest k on a tie), so
 * every phase sums to exactly 2^24 and a constant passes unchanged.  Per
 * source channel acc = sum_k c_k x[i0 + k] in int64 and y = clamp((acc + 2^23)
 * >> 24, -32768, 32767), an arithmetic shift; float32 output is y 2^-15.  A
 * stream with Fi == Fo takes no filter: its int16 samples pass unchanged.
 *
 * Channels, applied to the int16 results y: equal counts copy; a mono stream
 * is duplicated to every output channel; a mono output is m = floor((2 sum_k
 * y_k + Cs) / (2 Cs)), floor toward -infinity (the mean, rounded half up).
 * Any other pair of counts is refused, the stream and both counts named.
 *
 * Refused besides what gsc_decode_crops refuses, with nothing launched and
 * both rates named: a rate <= 0, 2 T > 512 (Fo / Fi < 1/16), a table of more
 * than 16 MiB (phases x taps x 4 bytes, e.g. 44101 -> 192000), and a filter
 * whose 2 T + 2 samples times the stream's channels exceed the 24576 source
 * samples a workgroup keeps.
 *
 * One launch: a workgroup takes gsc_resample_tile() output samples of a crop,
 * decodes the source samples they read into LDS and filters from there.
 * Stream order is gsc_decode_crops': no synchronisation, no sample copied to
 * the host, with one exception: the first use of a pair of rates on a device
 * builds its table on the host, uploads it with a blocking copy and keeps it
 * for the life of the process.  The tables are never written again, so later
 * calls on any stream use them unordered.  gsc_resample_prepare does that
 * ahead of time. */
typedef struct {
    int dtype;         /* GSC_PCM_* */
    int layout;        /* GSC_LAYOUT_* */
    long long length;  /* output samples per row */
    int out_rate;      /* Hz; 0: none */
    int out_channels;  /* 0: the streams' */
} gsc_crop_format;
int gsc_decode_crops_fmt(gsc_stream *const *streams, int nstreams, const gsc_crop *crops, int ncrops,
                         const gsc_crop_format *fmt, void *dst_device, void *hip_stream, long long *written);
/* The table of a pair of rates: *phases rows of *taps int32, *coeff pointing
 * into the process-wide cache (valid for the life of the process; do not
 * free).  Host only, needs no device.  Equal rates give the one-phase table
 * that gsc_decode_crops_fmt never applies. */
int gsc_resample_table(int in_rate, int out_rate, int *phases, int *taps, const int32_t **coeff);
/* the table of a pair on the calling thread's device, now instead of on first use */
int gsc_resample_prepare(int in_rate, int out_rate);
/* output samples of one workgroup of the resampling kernel */
int gsc_resample_tile(void);

/* ---- seek tables: opening a stream without the host walk -------------------- */
/* A seek table is a side blob that holds what the walk finds by following the
 * stream's two chains: where every frame starts, how many bits its bitstream
 * has, and every checkpoint.  The .gsc bytes are not touched.  Little-endian,
 * version 1, exactly 32 + 16 F + 8 P bytes:
 *
 *   offset      field
 *   0           magic "GSCT"
 *   4           u32 version = 1
 *   8           u32 S, gsc_decode_checkpoint_symbols() of the writer
 *   12          u32 F, frame count
 *   16          u64 stream length in bytes
 *   24          u64 P, checkpoints of all frames
 *   32          F x { u64 byte offset of the frame, u64 bits of its bitstream }
 *   32 + 16 F   P x u64 checkpoint, frames in order: bit offset within the
 *               frame's bitstream << 3 | (variableCodingHeader on entry + 1);
 *               a frame has ceil(FrameLength * ChannelCount / S) of them
 *
 * A table is never trusted.  The host checks what needs no symbol walk (the
 * sizes, S, the stream length, every frame header at its claimed offset with
 * the validations of gsc_index_create, the checkpoint counts and ranges, and
 * that the claimed bit counts chain the frames exactly to the stream's end);
 * then one device lane per checkpoint walks its segment and must land exactly
 * on the next checkpoint, or on the frame's bit count, without meeting a chunk
 * index >= ChunkCount.  A frame's first checkpoint is (0, -1) by definition,
 * so a table that passes is the one the walk would have written: opening with
 * a table succeeds if and only if gsc_index_create accepts the stream and
 * gsc_index_table of that index equals the table byte for byte, and the index
 * is then the same.  Otherwise NULL and gsc_last_error, which names the frame
 * and the checkpoint; nothing stays allocated.  A table written with another S
 * is refused. */
/* the table of any index: *table (release with gsc_free), *len bytes.  Host only. */
int gsc_index_table(const gsc_index *ix, uint8_t **table, size_t *len);
/* gsc_index_create without the walk.  Needs the device: the stream's bytes and
 * the checkpoints are uploaded for the check and freed again.
 * gsc_index_create remains the way that needs none. */
gsc_index *gsc_index_create_with_table(const uint8_t *gsc, size_t len, const uint8_t *table, size_t table_len);
/* gsc_stream_open without the walk: one upload, checked against the resident slabs */
gsc_stream *gsc_stream_open_with_table(const uint8_t *gsc, size_t len, const uint8_t *table, size_t table_len);
/* gsc_encode_prepared that also returns the table of the bytes it returns
 * (offsets relative to them: a frame range is a stream of its own), straight
 * from the index packer, which knows every checkpoint.  One file only. */
int gsc_encode_prepared_with_table(gsc_prepared *p, int frame_begin, int frame_end, uint8_t **out, size_t *out_len,
                                   uint8_t **table, size_t *table_len);
/* Timing of the last gsc_stream_open, gsc_stream_open_with_table or
 * gsc_index_create_with_table on the calling thread (milliseconds): host_ms is
 * the walk, or with a table the frame headers and the codebook / attenuation
 * tables; verify_ms the check on the device (0 without a table). */
typedef struct {
    double host_ms, upload_ms, verify_ms, total_ms;
    long long uploaded_bytes, checkpoints;
} gsc_open_timing;
void gsc_last_open_timing(gsc_open_timing *t);

/* ---- stream sets: many streams opened as one ---------------------------------- */
/* A loader's corpus is thousands of short files.  gsc_stream_set_open opens
 * `count` streams as one resident set: one set of slabs holds every stream's
 * bytes, checkpoints, int16 codebooks, attenuations and frame table, back to
 * back.  tables may be NULL (every stream is walked on the host); tables[i] may
 * be NULL (stream i is walked).  Stream i with tables[i] is accepted and
 * refused exactly as gsc_stream_open_with_table(gscs[i], tables[i]) would be.
 * The streams are indexed in parallel on the host; only the raw bytes, the
 * checkpoints and the frame descriptors are uploaded, and one kernel launch
 * expands every frame's codebook and attenuations on the device, one more
 * checks every table.  The number of device allocations, launches and
 * synchronisations does not depend on `count`, the number of copies only on
 * the bytes; the work runs on the default stream and the call waits for that
 * stream, once, never for the device.  A refusal fails the whole call
 * and frees everything: NULL and gsc_last_error, "stream <i>: " followed by
 * that stream's own message, i the lowest refused stream (a stream the host
 * refuses is reported before one only the device check refuses).  count <= 0
 * and 2^31 or more frames or checkpoints in all are refused.
 *
 * A member is an ordinary gsc_stream, borrowed from the set and valid until
 * gsc_stream_set_free: gsc_stream_info, _index, _device, _decode_samples and
 * gsc_decode_crops take it, and one gsc_decode_crops call may mix members of
 * several sets and streams opened on their own.  gsc_stream_free on a member
 * frees nothing and sets gsc_last_error.  A member's index keeps no host copy
 * of its codebooks; gsc_decode_indexed builds one on first use. */
typedef struct gsc_stream_set gsc_stream_set;
gsc_stream_set *gsc_stream_set_open(const uint8_t *const *gscs, const size_t *lens, const uint8_t *const *tables,
                                    const size_t *table_lens, int count);
int gsc_stream_set_count(const gsc_stream_set *set);
gsc_stream *gsc_stream_set_stream(gsc_stream_set *set, int i);
/* waits for the device's queued work first, as gsc_stream_free */
void gsc_stream_set_free(gsc_stream_set *set);
/* Timing of the last gsc_stream_set_open on the calling thread (milliseconds):
 * host_ms the indexes and the layout, upload_ms allocation, staging and copies
 * (host clock), expand_ms and verify_ms the two kernels (device events).  The
 * last four fields count runtime calls where they are made. */
typedef struct {
    double host_ms, upload_ms, expand_ms, verify_ms, total_ms;
    long long uploaded_bytes, streams, frames, checkpoints;
    int device_allocations, h2d_copies, launches, synchronisations;
} gsc_set_open_timing;
void gsc_last_set_open_timing(gsc_set_open_timing *t);
/* Stage entry point, parity tests: the device tables of one frame of a
 * resident stream (a set's member or not), downloaded: ChunkCount * ChunkSize
 * int16 rounded up to a multiple of 8 (the padding is zero) to cb_out,
 * ChunkCount attenuations to att_out. */
int gsc_stream_tables(const gsc_stream *st, int frame, int16_t *cb_out, uint8_t *att_out);
/* gsc_encode_prepared_files that also returns every file's seek table:
 * tables_len bytes in *tables (release with gsc_free), table_bytes[i] of them
 * file i's, in file order.  Each is the table of that file's returned bytes,
 * cut from the packer's checkpoints and rebased to the file's first byte; a
 * file with no frame in the range gets an empty table. */
int gsc_encode_prepared_files_with_tables(gsc_prepared *p, int frame_begin, int frame_end, uint8_t **out,
                                          size_t *out_len, size_t *file_bytes, uint8_t **tables, size_t *tables_len,
                                          size_t *table_bytes);

/* ---- bound streams: crops whose list lives on the device ----------------------- */
/* gsc_decode_crops and gsc_decode_crops_fmt plan every crop on the host and
 * upload the plan, so the crop list must exist on the host and every call
 * allocates and copies.  A binding describes the streams of a loader once on
 * the device; gsc_crop_binding_decode then takes the crops from device memory
 * and does nothing on the host but check its arguments and launch one kernel,
 * which plans each crop itself.
 *
 * gsc_crop_binding_create may block, allocate and copy: it uploads one
 * descriptor per stream (its slabs and their sizes, its frames, samples and
 * channels, its resampler for out_rate) and, for every distinct source rate,
 * the resampler's table (as gsc_resample_prepare).  out_rate and out_channels
 * are gsc_crop_format's: out_rate 0 resamples nothing, out_channels 0 takes
 * the streams' count, which must then agree; with both 0 the binding runs the
 * fused kernel of gsc_decode_crops, otherwise the kernel of
 * gsc_decode_crops_fmt.  Refused (NULL and gsc_last_error, the stream named):
 * what gsc_decode_crops and gsc_decode_crops_fmt refuse per stream, i.e.
 * channel counts that do not agree or do not map, a pair of rates without a
 * resampler, a filter too wide for a workgroup, a stream of more than 2^40
 * samples, and a stream on another device than the calling thread's; also no
 * streams at all.  Members of sets and streams opened on their own mix
 * freely.  The binding borrows the streams: they must stay open until
 * gsc_crop_binding_free, which first waits for the device's queued work.
 *
 * gsc_crop_binding_decode.  crops_device is ncrops x {stream, begin, count} as
 * int64 in device memory, stream counting the binding's streams.  Units are
 * gsc_decode_crops_fmt's: `begin` in source samples of the crop's stream,
 * `count` and `length` in output samples at out_rate (the stream's own rate
 * without one).  dst_device, dtype, layout and the clipping at a stream's end
 * are gsc_decode_crops'.  written_device (may be NULL) is ncrops int64 in
 * device memory: the clipped length of each crop, as gsc_decode_crops reports
 * it on the host, stored once per crop.
 *
 * Bad crops.  The call cannot refuse a value it never reads, so a bad crop
 * costs its own row and nothing else: the row is zero over the whole length,
 * written[i] is -1, every other row is what it would be without it.  A crop is
 * bad when its stream is outside [0, nstreams), when begin < 0 or begin > its
 * stream's samples, or when count < 0 or count > length: gsc_decode_crops'
 * per-crop refusals.  The kernels check or clamp every index they derive.
 *
 * The call contract.  The call reads no crop on the host, allocates nothing,
 * copies nothing, synchronises nothing and keeps no scratch between calls:
 * calls with one binding on several HIP streams share only memory that nobody
 * writes.  It checks dtype, layout, the pointers and that ncrops x length x
 * channels and length x the largest decimation step stay within 2^40, that the
 * calling thread is on the binding's device, and launches on hip_stream;
 * ncrops == 0 or length == 0 launches nothing and leaves written_device as it
 * is.  Everything is ordered with hip_stream alone, so crops_device may be
 * written by earlier work of that stream, and the call may be recorded into a
 * HIP graph and replayed with new crops in the same memory (the library has no
 * capture helper and tests none).
 *
 * gsc_crop_binding_last_call: the runtime calls of the calling thread's last
 * gsc_crop_binding_decode, counted where they are made, and its host time. */
typedef struct gsc_crop_binding gsc_crop_binding;
typedef struct {
    int launches, allocations, copies, synchronisations;
    double host_ms;
} gsc_crop_call_stats;
gsc_crop_binding *gsc_crop_binding_create(gsc_stream *const *streams, int nstreams, int out_rate, int out_channels);
int gsc_crop_binding_decode(gsc_crop_binding *b, const long long *crops_device, int ncrops, int dtype, int layout,
                            long long length, void *dst_device, long long *written_device, void *hip_stream);
void gsc_crop_binding_last_call(gsc_crop_call_stats *stats);
void gsc_crop_binding_free(gsc_crop_binding *b);
/* The planner of the bound kernels for one crop, on the host and without a
 * device (parity tests): crop (stream, begin, count) of a call over nstreams
 * streams with `length`, the crop's stream being ix, at out_rate (0: its own).
 * Returns 0 for a good crop, 1, 2 or 3 for a bad stream index, begin or count
 * (*written = -1 then), < 0 and gsc_last_error for a pair of rates without a
 * resampler.  For a good crop *written is the clipped count, [*src_begin,
 * *src_end) the source samples its filter reads inside the stream and [*f0,
 * *f1) the frames that hold them; all 0 when nothing is written. */
int gsc_crop_plan_model(const gsc_index *ix, int nstreams, int stream, long long begin, long long count,
                        long long length, int out_rate, long long *written, int *f0, int *f1, long long *src_begin,
                        long long *src_end);

/* ---- mixing crops: gain-weighted sums of crops of bound streams ------------------- */
/* Noise and reverb augmentation, overlapped speakers, "speech + music + noise":
 * every output row is a weighted sum of several crops.  gsc_crop_binding_mix
 * forms the rows in one kernel launch straight from the resident compressed
 * slabs; no source's PCM and no intermediate row is written to memory.
 *
 * Definition.  A source is {stream, begin, count, gain}, all int64.  stream,
 * begin and count are exactly a crop of gsc_crop_binding_decode: the same units
 * (begin in source samples of the stream, count and length in output samples at
 * the binding's rate), the same clipping at the stream's end, the same
 * conversion to the binding's out_rate and out_channels.  gain is Q15: 32768 is
 * unity, -32768 inverts; -2^20 <= gain <= 2^20.  With x_k[t][c] the int16 value
 * gsc_crop_binding_decode would write for source k at output sample t and
 * channel c (zero at and after the source's clipped count), row r with sources
 * k = 0 .. nsrc - 1 is
 *   s       = sum over k of gain_k * x_k[t][c]            exact, in 64 bits
 *   y[t][c] = clamp((s + 16384) >> 15, -32768, 32767)     arithmetic shift: floor
 * int16 output is y, float32 output y / 32768 (exact), the relation of
 * gsc_decode_crops.  |s| stays below 2^43.  written[r] is the largest clipped
 * count among the row's sources, 0 when all are empty; elements at or past
 * every source's clipped count are 0, and the whole length of every row is
 * written.  A slot with count == 0 adds nothing and reads no stream data: that
 * is how a row uses fewer than nsrc sources (its stream, begin and gain must
 * still be valid).
 *
 * Bad rows.  A row is bad when one of its sources is a bad crop by
 * gsc_crop_binding_decode's rules (stream outside the binding, begin < 0 or
 * past the stream's samples, count < 0 or > length) or has a gain outside
 * [-2^20, 2^20].  A bad row is zero over its whole length, written[r] is -1,
 * and every other row is what it would be without it.
 *
 * gsc_crop_binding_mix.  sources_device is nrows x nsrc x {stream, begin,
 * count, gain}, contiguous int64 in device memory; 1 <= nsrc <= 256.
 * dst_device, dtype, layout and written_device (nrows int64, may be NULL) are
 * gsc_crop_binding_decode's, and so is the call contract: the call reads no
 * source on the host, allocates nothing, copies nothing, synchronises nothing
 * and keeps no scratch between calls; it checks dtype, layout, the pointers,
 * nsrc, that nrows x length x channels and length x the largest decimation step
 * stay within 2^40 and that the calling thread is on the binding's device, and
 * launches one kernel on hip_stream; nrows == 0 or length == 0 launches nothing
 * and leaves written_device as it is.  Everything is ordered with hip_stream
 * alone.  gsc_crop_binding_last_call reports the calling thread's last
 * gsc_crop_binding_decode or gsc_crop_binding_mix.
 *
 * gsc_mix_model: the arithmetic alone, on the host and without a device (parity
 * tests): *y from n pairs (x[i], gain[i]), 1 <= n <= 256.  Returns 0, or -1 for
 * a null pointer, another n or a gain outside the range (nothing is written). */
int gsc_crop_binding_mix(gsc_crop_binding *b, const long long *sources_device, int nrows, int nsrc, int dtype,
                         int layout, long long length, void *dst_device, long long *written_device,
                         void *hip_stream);
int gsc_mix_model(const int16_t *x, const long long *gain, int n, int16_t *y);

/* ---- stream envelopes: block energy and peak of bound streams -------------------- */
/* A sampler that draws crops on the device needs to know where a stream holds
 * sound.  The envelope of a stream is computed straight from its resident
 * compressed slabs by one kernel launch; no PCM is written to memory.
 *
 * Definition.  A stream has S samples per channel and C channels and decodes to
 * int16 x[t][k], 0 <= t < S, 0 <= k < C, exactly as gsc_decode gives them.
 * For a hop H, 64 <= H <= 65536 (any integer), the stream has nb = ceil(S / H)
 * blocks; block b covers samples [b H, min((b + 1) H, S)) of every channel:
 *   energy[b] = sum of x[t][k]^2 over the block's samples and all channels, as
 *               int64 (it does not fit 32 bits);
 *   peak[b]   = max of |x[t][k]| over the same, as int32, so that |-32768| =
 *               32768 is representable.
 * The last block is partial when H does not divide S; S = 0 gives no blocks.
 * Blocks count source samples of the stream: a binding's out_rate and
 * out_channels play no part, which is the unit of a crop's `begin`.  For
 * several streams the blocks are concatenated in the binding's order:
 * offsets[i] is the first block of stream i, offsets[n] the total.  All of it
 * is integer arithmetic, so the results do not depend on the order of the sums.
 *
 * gsc_envelope_layout: offsets[0 .. n] for n streams of samples[i] samples per
 * channel.  Host only, no device needed.  Refused (-1 and gsc_last_error): hop
 * outside [64, 65536], n < 0, a negative length (the stream named), and 2^31
 * or more blocks in all.
 *
 * gsc_crop_binding_envelope: energy_device (int64) and peak_device (int32) are
 * nblocks elements each in device memory; nblocks must equal the layout's
 * total for the binding's streams.  Every block is written, zero where nothing
 * decodes.  A once-per-corpus call like gsc_crop_binding_create: it may
 * allocate, copy and block.  It uploads its own small layout with a blocking
 * copy, launches one kernel on hip_stream and waits for that stream before it
 * returns.  A total of 0 blocks launches nothing.  Refused: a null binding, a
 * hop gsc_envelope_layout refuses, another nblocks, null outputs, outputs that
 * are not device memory of the binding's device, and a calling thread bound to
 * another device.  The streams must still be open. */
int gsc_envelope_layout(const long long *samples, int n, int hop, long long *offsets);
int gsc_crop_binding_envelope(gsc_crop_binding *b, int hop, long long *energy_device, int *peak_device,
                              long long nblocks, void *hip_stream);

/* ---- stream fidelity: block error energy of bound streams against source PCM ------ */
/* How good an encode is, and where it is bad: per block and per stream the
 * energy of the difference between what a resident stream decodes to and its
 * source PCM, straight from the compressed slabs by one kernel launch; no PCM
 * is written to memory.
 *
 * Definition.  A stream of S samples per channel and C channels decodes to
 * int16 x[t][k], 0 <= t < S, 0 <= k < C, exactly as gsc_decode gives them.  Its
 * reference is int16 r[t][k], interleaved [R, C] in device memory, with the
 * stream's own C and at the stream's own rate: stream sample t corresponds to
 * reference sample t.  R may be any value >= 0, and r[t][k] = 0 for t >= R.
 * The encoder pads streams past their WAV, so S may exceed the source's length;
 * reference samples at t >= S are ignored.  With d = x - r (|d| <= 65535),
 * every block of a hop H has three results, hops and blocks being exactly
 * those of gsc_envelope_layout (64 <= H <= 65536, block b covers samples
 * [b H, min((b + 1) H, S)) of every channel, S = 0 gives no blocks) and the
 * concatenation over streams the same:
 *   err_energy[b] = sum of d^2 over the block's samples and all channels, as
 *                   int64 (d^2 reaches 4,294,836,225: it does not fit a signed
 *                   32-bit product);
 *   ref_energy[b] = sum of r^2 over the same samples, as int64;
 *   err_peak[b]   = max of |d| over the same samples, as int32.
 * Every block of every stream is written.  Every sample of [0, S) contributes,
 * including those that decode to zero.  A binding's out_rate and out_channels
 * play no part.  All of it is integer arithmetic, so the results do not depend
 * on the order of the sums.  The SNR of a block or a stream is 10 log10 of a
 * sum of ref_energy over a sum of err_energy, which the caller forms.
 *
 * gsc_crop_binding_fidelity: ref_device and ref_samples are host arrays with
 * one entry per bound stream: a device pointer to that stream's reference and
 * the reference's samples per channel (R).  A null pointer with 0 samples is an
 * all-zero reference.  References need no more than 2-byte alignment and are
 * only read.  err_energy_device, ref_energy_device (int64) and err_peak_device
 * (int32) are nblocks elements each in device memory; nblocks must equal the
 * layout's total for the binding's streams.  A once-per-corpus call under
 * gsc_crop_binding_envelope's licence: it may allocate, uploads its layout and
 * the per-stream reference descriptors with a blocking copy, launches one
 * kernel on hip_stream and waits for that stream before it returns.  A total
 * of 0 blocks launches nothing.  Refused (-1 and gsc_last_error, the stream
 * named where one is at fault): everything gsc_crop_binding_envelope refuses,
 * null ref_device or ref_samples, a negative reference length, a null
 * reference with a positive length, and a reference or an output that is not
 * device memory of the binding's device.  The streams must still be open. */
int gsc_crop_binding_fidelity(gsc_crop_binding *b, int hop, const void *const *ref_device,
                              const long long *ref_samples, long long *err_energy_device,
                              long long *ref_energy_device, int *err_peak_device, long long nblocks,
                              void *hip_stream);

/* Timing of the last gsc_decode*, gsc_stream_open or crop call on the calling
 * thread (milliseconds).  h2d_bytes: the bytes that call uploaded.  After
 * gsc_decode_crops or gsc_decode_crops_fmt h2d_bytes is the job descriptors
 * alone, frames the sum over the crops of the frames each one crosses, and
 * symbols 0: the crop kernels unpack into LDS, no symbol scratch exists. */
typedef struct {
    double host_index_ms, h2d_ms, gpu_unpack_ms, gpu_synth_ms, d2h_ms, total_ms;
    int frames;
    long long symbols, samples; /* symbols unpacked, int16 values written */
    long long h2d_bytes;
} gsc_decode_timing;
void gsc_last_decode_timing(gsc_decode_timing *t);

int gsc_device_count(void);
/* bind the calling thread to a HIP device (one process per GPU) */
int gsc_set_device(int device);
const char *gsc_last_error(void);
void gsc_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
