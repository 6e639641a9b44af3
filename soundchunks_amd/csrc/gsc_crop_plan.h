// The arithmetic of one crop, for the host and the device alike, as functions
// that compile with and without HIP.  The host planner (plan_crops,
// gsc_resample.cpp) calls crop_plan_one for every crop of a call and refuses
// the whole call for one bad crop; a crop list that lives on the device
// (gsc_crop_binding) is planned by the decode kernels themselves with the same
// functions, and there a bad crop costs its own row only.
// tools/decode/crop_check.cpp holds them against a model of its own.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GSC_HD __host__ __device__
#else
#define GSC_HD
#endif

namespace gsc {

// Why a crop is bad; the three pairs of plan_crops' per-crop refusals.
enum CropStatus : int {
    kCropGood = 0,
    kCropBadStream = 1,  // stream < 0, stream >= nstreams
    kCropBadBegin = 2,   // begin < 0, begin > samples
    kCropBadCount = 3,   // count < 0, count > length
};

// A good crop, clipped: `count` output samples, the source samples
// [src_begin, src_end) its filter reads inside the stream and the frames
// [f0, f1) that hold them.  count 0: everything else is 0, nothing is read.
struct CropSpan {
    int64_t count, src_begin, src_end;
    int32_t f0, f1;
};

GSC_HD inline int crop_stream_status(int64_t stream, int64_t nstreams) {
    return stream >= 0 && stream < nstreams ? kCropGood : kCropBadStream;
}

// The frame that holds sample s: the last of [0, nframes) whose first sample
// is <= s.  Of a run of frames that start at the same sample that is the last
// one, the others being empty (index_locate).  first_sample(i) reads frame i's;
// nframes >= 1.
template <typename FirstSample>
GSC_HD inline int32_t crop_frame_at(int32_t nframes, int64_t s, FirstSample first_sample) {
    int32_t lo = 0, hi = nframes - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (first_sample(mid) <= s) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

// One crop of a stream of `samples` samples per channel in nframes frames,
// resampled by rate_up / rate_down with half_taps taps per side (1, 1, 0: at
// the stream's own rate).  `begin` is in source samples, `count` and `length`
// in output samples.  The caller made sure that samples <= 2^40, rate_up <=
// 2^17 and length * rate_down <= 2^40, so that no product below leaves 64 bits.
template <typename FirstSample>
GSC_HD inline int crop_plan_one(int64_t begin, int64_t count, int64_t length, int64_t samples, int32_t nframes,
                                int32_t rate_up, int32_t rate_down, int32_t half_taps, FirstSample first_sample,
                                CropSpan* out) {
    *out = CropSpan{0, 0, 0, 0, 0};
    if (begin < 0 || begin > samples) return kCropBadBegin;
    if (count < 0 || count > length) return kCropBadCount;
    // outputs before the source position reaches the stream's end (resample_outputs)
    const int64_t avail = begin >= samples ? 0 : ((samples - begin) * rate_up + rate_down - 1) / rate_down;
    const int64_t n = count < avail ? count : avail;
    if (n <= 0 || nframes <= 0) return kCropGood;
    out->count = n;
    // outputs 0 .. n - 1 sit at source samples begin .. last; the filter reads T - 1 before and T after
    const int64_t last = (begin * rate_up + (n - 1) * rate_down) / rate_up;
    const int64_t before = half_taps > 0 ? half_taps - 1 : 0;
    out->src_begin = begin - before > 0 ? begin - before : 0;
    out->src_end = last + half_taps + 1 < samples ? last + half_taps + 1 : samples;
    out->f0 = crop_frame_at(nframes, out->src_begin, first_sample);
    out->f1 = crop_frame_at(nframes, out->src_end - 1, first_sample) + 1;
    return kCropGood;
}

}  // namespace gsc
