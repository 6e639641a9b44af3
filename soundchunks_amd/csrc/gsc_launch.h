// The one declaration of every kernel launcher and kernel-side helper that a
// host .cpp calls, grouped by the .hip file that defines it.  The defining
// file includes this header too, so a definition that disagrees with what the
// callers see is a compile error (the functions have C linkage: the linker
// checks no signature).  No default arguments.
//
// Not here: gsc_birch.hip's two entry points, which gsc_birch_host.cpp declares
// itself as plain C (it also builds with a host compiler alone).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gsc {
struct ReduceFrame;  // gsc_device.h
struct DspFrame;
struct ReconFrame;
struct FitFrame;
struct PackFrame;
struct DecFrame;  // gsc_decode.h
struct DecJob;
struct ResFrame;
struct TableSrc;
struct CropJob;
struct BoundStream;
struct FidelityRef;  // gsc_envelope.h
}  // namespace gsc

extern "C" {

// ---- gsc_yakmo.hip
hipError_t gsc_launch_yakmo(int D, const gsc::ReduceFrame* frames, int nframes, const float* X, float* C, float* fs,
                            int* is, float* gsum, uint32_t* gbits, int max_n, hipStream_t st);
hipError_t gsc_launch_yakmo_chain_test(int ppl, const float* pts, int nbk, float run, int* k_out, float* out);
size_t gsc_yakmo_big_floats(int64_t total_points, int nframes);
size_t gsc_yakmo_big_words(int64_t total_points, int nframes);
int gsc_yakmo_max_lds_points(void);

// ---- gsc_scan.hip
hipError_t gsc_launch_scan_batch(int D, int logk, gsc::ReduceFrame* frames, int nframes, const float* X, float* C,
                                 int* is, const float* rate_tab, double tol, int max_passes, int opts, float* tails,
                                 int kinds, hipStream_t st, hipStream_t st_general, hipEvent_t fork, hipEvent_t join);
hipError_t gsc_launch_scan_classify(int D, int logk, gsc::ReduceFrame* frames, int nframes, const float* C,
                                    hipStream_t st);
int gsc_scan_has_experiments(void);
int gsc_scan_has_plain(int D, int logk);
size_t gsc_scan_tail_floats_per_frame(int D, int logk);

// ---- gsc_kernels.hip
hipError_t gsc_launch_scan_pass(int D, gsc::ReduceFrame* frames, int nframes, int K, const float* X, float* C, int* is,
                                float* fs, const float* rate_tab, double tol, int max_passes, int only_flagged,
                                hipStream_t st);
hipError_t gsc_launch_knnfit(int CS, gsc::FitFrame* frames, int nframes, int max_n, int max_r, const float* cand,
                             const float* q, int* out, hipStream_t st);

// ---- gsc_ann.hip
hipError_t gsc_launch_ann_build(const float* pts, int n, int dd, int* pidx, int* cd, float* cv, float* lo, float* hi,
                                float* bnd, float* val, hipStream_t st);
hipError_t gsc_launch_ann_query(const float* pts, int n, int dd, int* pidx, int* cd, float* cv, float* lo, float* hi,
                                float* bnd, const float* q, int k, int mode, float eps, int* idxs, float* errs,
                                float* dist, float* mk_key, int* mk_info, float* pq_key, int* pq_h, int* pq_s,
                                int* pq_n, hipStream_t st);
hipError_t gsc_launch_ann_build_many(const void* trees, int ntrees, hipStream_t st);
hipError_t gsc_launch_knnfit_ann(const void* trees, const void* jobs, int njobs, const float* q, int* out,
                                 float* pq_key, void* pq_node, int pq_cap, hipStream_t st);

// ---- gsc_dsp.hip
hipError_t gsc_launch_pcm(const int16_t* pcm, int64_t span, int ch, double* samp, hipStream_t st);
hipError_t gsc_launch_atten(int cs, gsc::DspFrame* frames, int nframes, const double* samp, int64_t span, int ch,
                            int obd, hipStream_t st);
hipError_t gsc_launch_features(int cs, const gsc::DspFrame* frames, int nframes, int max_n, const double* samp,
                               int64_t span, int ch, const double* trig, double s0, double scale, float* X,
                               uint8_t* nr, float* Q, hipStream_t st);

// ---- gsc_recon.hip
hipError_t gsc_launch_recon(const gsc::ReconFrame* frames, int nframes, int max_n, int cs, int ch, int bd,
                            const uint32_t* chunk, const int16_t* rdst, const uint8_t* ratten, int16_t* out,
                            hipStream_t st);
hipError_t gsc_launch_sqdiff(const int16_t* a, const int16_t* b, int64_t n, unsigned long long* acc, hipStream_t st);

// ---- gsc_pack.hip
hipError_t gsc_launch_usecount(const gsc::PackFrame* frames, int nframes, const int* best, int* counts,
                               hipStream_t st);
hipError_t gsc_launch_pack(gsc::PackFrame* frames, int nframes, const int* best, const int* remap, uint32_t* words,
                           uint32_t* codes, uint64_t* cps, hipStream_t st);

// ---- gsc_decode.hip
hipError_t gsc_launch_decode_unpack(const gsc::DecFrame* frames, int nframes, const uint64_t* cps, int64_t ncp,
                                    const uint32_t* words, int64_t nwords, uint16_t* sym, int64_t nsym,
                                    hipStream_t st);
hipError_t gsc_launch_decode_verify(const gsc::ResFrame* frames, const uint64_t* frame_bits, int nframes,
                                    const uint64_t* cps, int64_t ncp, const uint32_t* words, int64_t nwords,
                                    unsigned long long* status, hipStream_t st, int* launched);
hipError_t gsc_launch_expand_tables(const gsc::ResFrame* frames, const gsc::TableSrc* src, int nframes,
                                    int64_t ncb_used, const uint8_t* bytes, int64_t nbytes, int16_t* cb, int64_t ncb,
                                    uint8_t* att, int64_t natt, hipStream_t st, int* launched);
hipError_t gsc_launch_decode_synth(const gsc::DecFrame* frames, int nframes, const gsc::DecJob* jobs, int njobs,
                                   int lds_bytes, const uint16_t* sym, int64_t nsym, const int16_t* cb, int64_t ncb,
                                   const uint8_t* att, int64_t natt, int16_t* out, int64_t nout, hipStream_t st);

// ---- gsc_decode_crops.hip
hipError_t gsc_launch_crop_fused(const gsc::CropJob* jobs, int ncrops, int64_t length, int channels, int is_float,
                                 int planar, int tile_len, void* out, hipStream_t st);
hipError_t gsc_launch_crop_fused_bound(const gsc::BoundStream* streams, int nstreams, const int64_t* crops, int ncrops,
                                       int64_t length, int channels, int is_float, int planar, int tile_len, void* out,
                                       int64_t* written, hipStream_t st);

// ---- gsc_decode_resample.hip
hipError_t gsc_launch_crop_resample(const gsc::CropJob* jobs, int ncrops, int64_t length, int channels, int is_float,
                                    int planar, int src_samples, void* out, hipStream_t st);
hipError_t gsc_launch_crop_resample_bound(const gsc::BoundStream* streams, int nstreams, const int64_t* crops,
                                          int ncrops, int64_t length, int channels, int is_float, int planar,
                                          int src_samples, void* out, int64_t* written, hipStream_t st);
hipError_t gsc_prepare_crop_resample_bound(int src_samples);

// ---- gsc_decode_mix.hip
hipError_t gsc_launch_crop_mix(const gsc::BoundStream* streams, int nstreams, const int64_t* sources, int nrows,
                               int nsrc, int64_t length, int channels, int is_float, int planar, int resample,
                               int src_samples, void* out, int64_t* written, hipStream_t st);
hipError_t gsc_prepare_crop_mix(int channels, int src_samples);

// ---- gsc_decode_envelope.hip
hipError_t gsc_launch_envelope(const gsc::BoundStream* streams, int nstreams, const int64_t* layout, int64_t ntiles,
                               int hop, int64_t* energy, int32_t* peak, int64_t nblocks, hipStream_t st);

// ---- gsc_decode_fidelity.hip
hipError_t gsc_launch_fidelity(const gsc::BoundStream* streams, int nstreams, const int64_t* layout, int64_t ntiles,
                               const gsc::FidelityRef* refs, int hop, int64_t* err_energy, int64_t* ref_energy,
                               int32_t* err_peak, int64_t nblocks, hipStream_t st);

}  // extern "C"
