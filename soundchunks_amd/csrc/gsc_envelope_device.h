// What the kernels that reduce a stream's tiles share (envelope_kernel in
// gsc_decode_envelope.hip, fidelity_kernel in gsc_decode_fidelity.hip), each in
// one place: which tile of which stream a workgroup owns and where its blocks
// go (tile_plan), and the walk over the tile's frames (tile_walk), which hands
// every decoded run to the kernel's own reduction.
//
// A workgroup of kFusedThreads lanes owns one tile of one stream, a whole number
// of hops (envelope_tile_len, gsc_envelope.h), so every block has one owner:
// nothing is combined across workgroups and no global atomic is used.  Lane 0
// finds the stream and the tile from the call's layout (the first workgroup and
// the first block of every stream), plans the tile as a crop of the stream at
// its own rate (crop_plan_one) and leaves the job in LDS, as the bound crop
// kernels do.  The tile is then decoded as crop_fused_kernel decodes it
// (fused_frame: per frame and per stretch of checkpoint segments, unpack into
// LDS, then table_sample with the codebook from global memory), but a sample
// goes into a reduction where the crop kernels store it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsc_decode.h"
#include "gsc_decode_device.h"
#include "gsc_envelope.h"

namespace gsc {

// where a workgroup's results go: blocks [first, first + count) of the output; the stream they belong to
struct alignas(16) TilePlace {
    int64_t first;
    int32_t count, stream;
};

// One lane: the tile of workgroup wg as a crop of its stream, and its place.
// layout: tile0[nstreams + 1] (stream i's first workgroup), then
// block0[nstreams + 1] (its first block).  A workgroup the layout does not
// cover, or a stream whose descriptor does not plan, gets an empty job (f0 ==
// f1) and, for the first, no blocks.  nstreams > 0; hop is in range.
__device__ __forceinline__ void tile_plan(const BoundStream* __restrict__ streams, int nstreams,
                                          const int64_t* __restrict__ layout, int hop, int64_t wg, CropJob* job,
                                          TilePlace* place) {
    const int tile_len = envelope_tile_len(hop);
    const int bpt = tile_len / hop;  // 1 .. kEnvelopeMaxBlocks
    const int64_t* tile0 = layout;
    const int64_t* block0 = layout + nstreams + 1;
    const int s = last_le(0, nstreams - 1, wg, [&](int i) { return tile0[i]; });
    const int64_t tile = wg - tile0[s], ntiles = tile0[s + 1] - tile0[s];
    const int64_t b0 = block0[s], nb = block0[s + 1] - b0;
    CropJob j{};
    TilePlace pl{0, 0, s};
    if (tile >= 0 && tile < ntiles && b0 >= 0 && nb > 0 && tile * bpt < nb) {
        const int64_t left = nb - tile * bpt;
        pl.first = b0 + tile * bpt;
        pl.count = (int32_t)(left < bpt ? left : bpt);
        const BoundStream& d = streams[s];
        const ResFrame* frames = d.frames;
        CropSpan sp;
        // the tile as a crop of the stream at its own rate, whatever the binding's
        if (d.channels > 0 && d.channels <= 255 &&
            crop_plan_one(tile * tile_len, tile_len, tile_len, d.samples, d.nframes, 1, 1, 0,
                          [&](int i) { return frames[i].first_sample; }, &sp) == kCropGood &&
            sp.count > 0) {
            j = CropJob{frames,     d.cps,   d.words,  d.cb,      d.att, d.ncp, d.nwords, d.ncb,
                        d.natt,     tile * tile_len,   sp.count,  d.nframes,    sp.f0,    sp.f1,
                        sp.src_begin,      sp.src_end, nullptr,     1,        1,
                        0,          d.channels,        d.channels};
        }
    }
    *job = j;
    *place = pl;
}

// the samples of its tile that a job decodes: [0, tile_samples) of the tile, 0 for an empty or stale job
__device__ __forceinline__ int64_t tile_samples(const CropJob& job, int tile_len) {
    const int ch = job.src_ch;
    const bool span_ok = job.f0 >= 0 && job.f0 < job.f1 && job.f1 <= job.nframes && ch > 0 && ch <= 255;
    return !span_ok ? 0 : (job.count < tile_len ? job.count : tile_len);
}

// Every lane of a workgroup: crop_walk_job's walk over the frames of samples
// [0, tc) of the job's tile, tc = tile_samples.  run(ua, ub, value) takes the
// samples [ua, ub) of the tile that a frame decodes, value(t, k) being sample
// t's channel k; gap(ua, ub) takes what no frame covers, which decodes to zero.
// ssym holds kFusedSegs segments, slut 32 words (fused_frame).
template <typename Run, typename Gap>
__device__ __forceinline__ void tile_walk(const CropJob& job, int64_t tc, uint16_t* ssym, int* slut, int tid, Run run,
                                          Gap gap) {
    if (tc <= 0) return;
    auto add = [&](int64_t ua, int64_t ub, auto value) {
        if (ua < 0) ua = 0;
        if (ub > tc) ub = tc;
        if (ua < ub) run(ua, ub, value);
    };
    auto frame = fused_frame(ssym, slut, tid);
    const int fa = crop_frame_of(job, job.f0, job.f1, job.begin);
    const int fb = crop_frame_of(job, job.f0, job.f1, job.begin + tc - 1);
    int64_t done = 0;  // every sample of [0, done) went to run or gap
    for (int fr = fa; fr <= fb; ++fr) {
        const ResFrame& f = job.frames[fr];
        if (f.cs <= 0 || f.ch <= 0 || f.ch > 255 || f.count <= 0 || f.nsym <= 0) continue;
        int64_t ta = f.first_sample - job.begin, tb = ta + f.nsym / f.ch * f.cs;
        ta = ta < done ? done : ta;
        tb = tb > tc ? tc : tb;
        if (ta >= tb) continue;
        gap(done, ta);
        frame(job, f, fr, ta, tb, add);
        done = tb;
    }
    gap(done, tc);
}

}  // namespace gsc
